// transformer.cpp -- see transformer.h.  (compiled by hipcc as HIP: contains the load-time repack kernel)
#include "transformer.h"
#include <cstdlib>
#include <cmath>
#include <algorithm>

namespace q3 {

// ---- load-time repack: GGUF Q8_0 rows ([n][K/32]{f16 d; i8 qs[32]}) -> Q8Mat tiles (kernels.h) ----
__global__ void k_repack_q8(const uint8_t* __restrict__ raw, int n, int K, int row_off, uint8_t* __restrict__ qs,
                            uint16_t* __restrict__ sc, int sc_row_extra) { // quants go to row row_off + r of qs, scales to row row_off + sc_row_extra + r
    const int nb = K >> 5, nseg = K >> 8;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)n * nb) return;
    const int r = (int)(id / nb), b = (int)(id % nb);
    const uint8_t* src = raw + id * 34;
    const int row = row_off + r, rg = row >> 5, r32 = row & 31;
    uint16_t d;
    memcpy(&d, src, 2);
    const int srow = row + sc_row_extra;
    sc[(((size_t)(srow >> 5) * nseg + (b >> 3)) * 32 + (srow & 31)) * 8 + (b & 7)] = d;
    uint8_t* dst = qs + ((size_t)rg * nb + b) * 1024 + r32 * 16;
    for (int i = 0; i < 16; i++) { dst[i] = src[2 + i]; dst[512 + i] = src[18 + i]; }
}

// Q5_K super-block {f16 d, dmin; u8 scales[12]; u8 qh[32]; u8 qs[128]} -> packed planes (kernels.h) + {d,dmin} + {sc[8], m[8]}
__global__ void k_repack_q5k(const uint8_t* __restrict__ raw, int n, int K, int row_off, uint8_t* __restrict__ qs, const uint32_t* __restrict__ rg_off,
                             uint16_t* __restrict__ sc, uint8_t* __restrict__ meta) {
    const int nseg = K >> 8;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)n * nseg) return;
    const int r = (int)(id / nseg), s = (int)(id % nseg);
    const uint8_t* blk = raw + id * 176;
    const int row = row_off + r, rg = row >> 5, r32 = row & 31;
    const size_t vidx = ((size_t)rg * nseg + s) * 32 + r32;
    uint16_t d, dm;
    memcpy(&d, blk, 2); memcpy(&dm, blk + 2, 2);
    for (int i = 0; i < 8; i++) sc[vidx * 8 + i] = i == 0 ? d : i == 1 ? dm : 0;
    const uint8_t *scales = blk + 4, *qh = blk + 16, *ql = blk + 48;
    uint8_t* base = qs + (size_t)rg_off[rg] * 16 + (size_t)s * 5120;
    for (int j = 0; j < 8; j++) {
        int scv, mv;
        if (j < 4) { scv = scales[j] & 63; mv = scales[j + 4] & 63; }
        else { scv = (scales[j + 4] & 0xF) | ((scales[j - 4] >> 6) << 4); mv = (scales[j + 4] >> 4) | ((scales[j] >> 6) << 4); }
        meta[vidx * 16 + j] = (uint8_t)scv; meta[vidx * 16 + 8 + j] = (uint8_t)mv;
        const int jj = j >> 1, hi = j & 1;
        uint8_t q[32];
        uint32_t H = 0;
        for (int l = 0; l < 32; l++) {
            q[l] = (uint8_t)(hi ? (ql[32 * jj + l] >> 4) : (ql[32 * jj + l] & 0xF));
            H |= (uint32_t)((qh[l] >> (2 * jj + hi)) & 1) << (8 * (l & 3) + (l >> 2));
        }
        for (int h = 0; h < 2; h++)
            for (int w = 0; w < 2; w++)
                for (int bb = 0; bb < 4; bb++) base[j * 512 + h * 256 + r32 * 8 + w * 4 + bb] = (uint8_t)(q[16 * h + 8 * w + bb] | (q[16 * h + 8 * w + 4 + bb] << 4));
        memcpy(base + 4096 + r32 * 32 + j * 4, &H, 4);
    }
}
// Q6_K super-block {u8 ql[128]; u8 qh[64]; i8 scales[16]; f16 d} -> packed planes (values kept +32, unsigned 6 bit) + d + 16 sub-block scales
__global__ void k_repack_q6k(const uint8_t* __restrict__ raw, int n, int K, int row_off, uint8_t* __restrict__ qs, const uint32_t* __restrict__ rg_off,
                             uint16_t* __restrict__ sc, uint8_t* __restrict__ meta) {
    const int nseg = K >> 8;
    const size_t id = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (id >= (size_t)n * nseg) return;
    const int r = (int)(id / nseg), s = (int)(id % nseg);
    const uint8_t* blk = raw + id * 210;
    const int row = row_off + r, rg = row >> 5, r32 = row & 31;
    const size_t vidx = ((size_t)rg * nseg + s) * 32 + r32;
    uint16_t d;
    memcpy(&d, blk + 208, 2);
    for (int i = 0; i < 8; i++) sc[vidx * 8 + i] = i == 0 ? d : 0;
    for (int i = 0; i < 16; i++) meta[vidx * 16 + i] = blk[192 + i];
    uint8_t* base = qs + (size_t)rg_off[rg] * 16 + (size_t)s * 6144;
    for (int j = 0; j < 8; j++) {
        const int half = j >> 2, grp = j & 3;
        const uint8_t* L = blk + 64 * half;
        const uint8_t* Hq = blk + 128 + 32 * half;
        uint8_t q[32];
        uint32_t H0 = 0, H1 = 0;
        for (int l = 0; l < 32; l++) {
            int lo, hb;
            switch (grp) {
                case 0: lo = L[l] & 0xF; hb = (Hq[l] >> 0) & 3; break;
                case 1: lo = L[l + 32] & 0xF; hb = (Hq[l] >> 2) & 3; break;
                case 2: lo = L[l] >> 4; hb = (Hq[l] >> 4) & 3; break;
                default: lo = L[l + 32] >> 4; hb = (Hq[l] >> 6) & 3; break;
            }
            q[l] = (uint8_t)lo;
            H0 |= (uint32_t)(hb & 1) << (8 * (l & 3) + (l >> 2));
            H1 |= (uint32_t)(hb >> 1) << (8 * (l & 3) + (l >> 2));
        }
        for (int h = 0; h < 2; h++)
            for (int w = 0; w < 2; w++)
                for (int bb = 0; bb < 4; bb++) base[j * 512 + h * 256 + r32 * 8 + w * 4 + bb] = (uint8_t)(q[16 * h + 8 * w + bb] | (q[16 * h + 8 * w + 4 + bb] << 4));
        memcpy(base + 4096 + r32 * 64 + j * 8, &H0, 4);
        memcpy(base + 4096 + r32 * 64 + j * 8 + 4, &H1, 4);
    }
}

// The one device builder: allocates and zeroes the blob wlayout.h planned, uploads the row-group map of a mapped matrix and repacks every tensor
// (raw[i] = host GGUF rows of L.tensors[i]) into its row groups.
Q8Mat build_q8mat(const WLayout& L, const void* const* raw, DevBuf<uint8_t>& blob) {
    blob.alloc(L.total());
    blob.zero();
    uint8_t* base = blob.p;
    uint16_t* sc = reinterpret_cast<uint16_t*>(base + L.sc_at());
    uint8_t* meta = base + L.meta_at();
    uint32_t* off = reinterpret_cast<uint32_t*>(base + L.off_at());
    Q8Mat m;
    m.N = L.N; m.Npad = L.Npad; m.K = L.K; m.qs = base; m.sc = sc;
    if (L.mapped) {
        Q3_HIP(hipMemcpy(base + L.ty_at(), L.rg_type.data(), L.rg_type.size(), hipMemcpyHostToDevice));
        Q3_HIP(hipMemcpy(off, L.rg_off.data(), L.rg_off.size() * 4, hipMemcpyHostToDevice));
        m.meta = meta; m.rg_type = base + L.ty_at(); m.rg_off = off; m.qbytes = L.qbytes;
        m.nparts = L.nparts; m.p1_rg0 = L.p1_rg0; m.p2_rg0 = L.p2_rg0; m.p0_type = L.p0_type; m.p1_type = L.p1_type; m.p2_type = L.p2_type;
        m.p0_off = L.p0_off; m.p1_off = L.p1_off; m.p2_off = L.p2_off;
    }
    for (size_t i = 0; i < L.tensors.size(); i++) {
        const WTensor& t = L.tensors[i];
        const size_t raw_bytes = (size_t)t.rows * q3_gguf_row_bytes(t.type, L.K);
        DevBuf<uint8_t> d(raw_bytes);
        d.upload((const uint8_t*)raw[i], raw_bytes);
        const size_t nblk = (size_t)t.rows * (L.K / (t.type == Q3_T_Q8_0 ? 32 : 256));
        const dim3 grid((unsigned)((nblk + 255) / 256));
        // Q8_0 tiles are laid out the same in both layouts: the kernel is based on the tensor's first row group and counts rows from there
        if (t.type == Q3_T_Q8_0) hipLaunchKernelGGL(k_repack_q8, grid, dim3(256), 0, 0, d.p, t.rows, L.K, t.row0 & 31, base + (size_t)L.rg_off[(size_t)(t.row0 / 32)] * 16, sc, t.row0 & ~31);
        else if (t.type == Q3_T_Q5_K) hipLaunchKernelGGL(k_repack_q5k, grid, dim3(256), 0, 0, d.p, t.rows, L.K, t.row0, base, off, sc, meta);
        else hipLaunchKernelGGL(k_repack_q6k, grid, dim3(256), 0, 0, d.p, t.rows, L.K, t.row0, base, off, sc, meta);
        Q3_HIP(hipDeviceSynchronize());
    }
    return m;
}
Q8Mat q8mat_from_host(const void* raw_q8_0, int n, int k, DevBuf<uint8_t>& storage) { return build_q8mat(plan_wlayout({{Q3_T_Q8_0, 0, n}}, n, k, false), &raw_q8_0, storage); }
Q8Mat kqmat_from_host(const void* const* raw, const int32_t* types, const int32_t* rows, int nw, int k, DevBuf<uint8_t>& storage) {
    std::vector<WTensor> t;
    int n = 0;
    for (int i = 0; i < nw; i++) { t.push_back({types[i], n, rows[i]}); n += rows[i]; }
    return build_q8mat(plan_wlayout(t, n, k, true), raw, storage);
}

Q8Mat Transformer::make_mat(const Gguf& g, const std::vector<std::pair<std::string, int>>& rows, int N, int K) {
    std::vector<WTensor> tensors; std::vector<const void*> raw;
    for (auto& r : rows) {
        const GgufTensor& t = g.need(r.first);
        if (t.type != Q3_T_Q8_0 && t.type != Q3_T_Q5_K && t.type != Q3_T_Q6_K)
            throw Error("tensor " + r.first + ": ggml type " + std::to_string(t.type) + " is not supported by the HIP path (Q8_0, Q5_K, Q6_K)");
        Q3_CHECK(t.ne[0] == K, "unexpected K for " + r.first);
        tensors.push_back({t.type, r.second, (int)t.ne[1]}); raw.push_back(t.data);
    }
    const WLayout L = plan_wlayout(tensors, N, K, false);
    blobs_.emplace_back();
    return build_q8mat(L, raw.data(), blobs_.back());
}

FMat Transformer::make_fmat(const Gguf& g, const std::vector<std::string>& names, int K_expect) {
    FMat m;
    size_t total = 0;
    for (auto& n : names) {
        const GgufTensor& t = g.need(n);
        Q3_CHECK(t.ne[0] == K_expect && (t.type == Q3_T_F32 || t.type == Q3_T_F16 || t.type == Q3_T_BF16), "bad float tensor " + n);
        if (m.N == 0) m.type = t.type;
        Q3_CHECK(t.type == m.type, "mixed float types in one fused matrix: " + n);
        m.N += (int)t.ne[1]; total += t.nbytes;
    }
    m.K = K_expect;
    blobs_.emplace_back(total);
    size_t off = 0;
    for (auto& n : names) { const GgufTensor& t = g.need(n); Q3_HIP(hipMemcpy(blobs_.back().p + off, t.data, t.nbytes, hipMemcpyHostToDevice)); off += t.nbytes; }
    m.w = blobs_.back().p;
    if (K_expect % 256 == 0) { // tiled copy for the many-token kernel (k_gemm_float_mfma)
        const size_t esz = m.type == Q3_T_F32 ? 4 : 2;
        blobs_.emplace_back((size_t)((m.N + 63) / 64) * 64 * K_expect * esz);
        launch_tile_float(nullptr, m.w, blobs_.back().p, m.type, m.N, K_expect);
        Q3_HIP(hipDeviceSynchronize());
        m.wt = blobs_.back().p;
    }
    return m;
}

float* Transformer::load_f32(const Gguf& g, const std::string& name, int64_t n_expect) {
    const GgufTensor& t = g.need(name);
    Q3_CHECK(t.type == Q3_T_F32 && t.ne[0] * t.rows() == n_expect, "bad f32 tensor " + name);
    blobs_.emplace_back((size_t)n_expect * 4);
    blobs_.back().upload(t.data, (size_t)n_expect * 4);
    return reinterpret_cast<float*>(blobs_.back().p);
}

Transformer::Transformer(const std::string& path, int n_ctx, int max_tok) : n_ctx_(n_ctx), max_tok_(max_tok) {
    init_kernel_attributes();
    if (const char* e = std::getenv("Q3_UNFUSED")) fused = !(e[0] == '1'); // A/B switch for the parity tests (9 launches/layer)
    Gguf g(path);
    hp_.arch = g.kv_str("general.architecture", "qwen3");
    auto K = [&](const char* s) { return hp_.arch + "." + s; };
    hp_.n_embd = (int)g.kv_int(K("embedding_length"), 0);
    hp_.n_layer = (int)g.kv_int(K("block_count"), 0);
    hp_.n_head = (int)g.kv_int(K("attention.head_count"), 0);
    hp_.n_kv = (int)g.kv_int(K("attention.head_count_kv"), hp_.n_head);
    const int head_dim = (int)g.kv_int(K("attention.key_length"), hp_.n_head ? hp_.n_embd / hp_.n_head : 0);
    hp_.n_ff = (int)g.kv_int(K("feed_forward_length"), 0);
    hp_.eps = (float)g.kv_float(K("attention.layer_norm_rms_epsilon"), 1e-6);
    hp_.rope_base = (float)g.kv_float(K("rope.freq_base"), 1e6);
    if (auto* s = g.kv(K("rope.dimension_sections")))
        for (size_t i = 0; i < s->arr_i.size() && i < 4; i++) hp_.mrope_sec[i] = (int32_t)s->arr_i[i];
    Q3_CHECK(hp_.n_embd > 0 && hp_.n_layer > 0 && hp_.n_head > 0 && head_dim == Q3_HEAD_DIM, "unsupported hparams");
    Q3_CHECK(hp_.n_embd % 256 == 0 && hp_.n_embd <= 2048 && hp_.n_ff % 256 == 0 && hp_.n_head % hp_.n_kv == 0, "unsupported dims");
    Q3_CHECK(hp_.n_head * 128 <= 2048, "n_head*128 must be <= 2048 (single super-segment o-proj)");
    const int d = hp_.n_embd, dq = hp_.n_head * 128, dkv = hp_.n_kv * 128, ff = hp_.n_ff;
    layers_.resize(hp_.n_layer);
    {
        const int t0 = g.need("blk.0.attn_q.weight").type;
        float_mode_ = (t0 == Q3_T_F32 || t0 == Q3_T_F16 || t0 == Q3_T_BF16);
    }
    for (int l = 0; l < hp_.n_layer; l++) {
        Layer& L = layers_[l];
        const std::string p = "blk." + std::to_string(l) + ".";
        if (float_mode_) { // bf16 / f16 / f32 files: rows stay as stored, activations stay f32 (spec S3 float form)
            L.fqkv = make_fmat(g, {p + "attn_q.weight", p + "attn_k.weight", p + "attn_v.weight"}, d);
            L.fo = make_fmat(g, {p + "attn_output.weight"}, dq);
            L.fgu = make_fmat(g, {p + "ffn_gate.weight", p + "ffn_up.weight"}, d);
            L.fdown = make_fmat(g, {p + "ffn_down.weight"}, ff);
            L.attn_norm = load_f32(g, p + "attn_norm.weight", d);
            L.q_norm = load_f32(g, p + "attn_q_norm.weight", 128);
            L.k_norm = load_f32(g, p + "attn_k_norm.weight", 128);
            L.ffn_norm = load_f32(g, p + "ffn_norm.weight", d);
            const size_t lb = L.fqkv.bytes() + L.fo.bytes() + L.fgu.bytes() + L.fdown.bytes();
            if (l == 0) layer_weight_bytes_ = lb;
            weight_bytes_ += lb;
            continue;
        }
        L.wqkv = make_mat(g, {{p + "attn_q.weight", 0}, {p + "attn_k.weight", dq}, {p + "attn_v.weight", dq + dkv}}, dq + 2 * dkv, d);
        L.wo = make_mat(g, {{p + "attn_output.weight", 0}}, d, dq);
        L.wgu = make_mat(g, {{p + "ffn_gate.weight", 0}, {p + "ffn_up.weight", ff}}, 2 * ff, d);
        L.wdown = make_mat(g, {{p + "ffn_down.weight", 0}}, d, ff);
        if (L.wgu.nparts > 1) fused = false; // k_gateup_swiglu takes the type of the up rows from the gate rows; a file that mixes them runs the unfused sequence
        L.attn_norm = load_f32(g, p + "attn_norm.weight", d);
        L.q_norm = load_f32(g, p + "attn_q_norm.weight", 128);
        L.k_norm = load_f32(g, p + "attn_k_norm.weight", 128);
        L.ffn_norm = load_f32(g, p + "ffn_norm.weight", d);
        if (l == 0) layer_weight_bytes_ = L.wqkv.bytes() + L.wo.bytes() + L.wgu.bytes() + L.wdown.bytes();
        weight_bytes_ += L.wqkv.bytes() + L.wo.bytes() + L.wgu.bytes() + L.wdown.bytes();
    }
    if (const char* e = std::getenv("Q3_SPEC")) ggml_mode_ = std::string(e) == "ggml";
    if (ggml_mode_) {
        Q3_CHECK(!float_mode_, "Q3_SPEC=ggml serves Q8_0 / Q5_K_M files (float-weight files have no ggml-mode kernels)");
        gg_layers_.resize(hp_.n_layer);
        for (int l = 0; l < hp_.n_layer; l++) {
            const std::string p = "blk." + std::to_string(l) + ".";
            GgLayer& G = gg_layers_[l];
            G.wq = gg_load(g, p + "attn_q.weight", dq, d); G.wk = gg_load(g, p + "attn_k.weight", dkv, d); G.wv = gg_load(g, p + "attn_v.weight", dkv, d);
            G.wo = gg_load(g, p + "attn_output.weight", d, dq);
            G.gate = gg_load(g, p + "ffn_gate.weight", ff, d); G.up = gg_load(g, p + "ffn_up.weight", ff, d); G.down = gg_load(g, p + "ffn_down.weight", d, ff);
        }
    }
    output_norm_ = load_f32(g, "output_norm.weight", d);
    const GgufTensor& ot = g.need("output.weight");
    hp_.n_vocab = (int)ot.ne[1];
    if (float_mode_) { foutput_ = make_fmat(g, {"output.weight"}, d); fused = false; }
    else output_ = make_mat(g, {{"output.weight", 0}}, hp_.n_vocab, d);
    if (ggml_mode_) gg_output_ = gg_load(g, "output.weight", hp_.n_vocab, d);
    std::vector<float> c, s;
    build_rope_tables(hp_.rope_base, n_ctx, c, s);
    rope_cos_.alloc(c.size()); rope_cos_.upload(c.data(), c.size());
    rope_sin_.alloc(s.size()); rope_sin_.upload(s.data(), s.size());
    d_mrope_.alloc(4); d_mrope_.upload(hp_.mrope_sec, 4);
    alloc_workspace();
}

// RoPE tables: same double-precision expressions as the oracle (spec S5)
void build_rope_tables(float rope_base, int n_ctx, std::vector<float>& c, std::vector<float>& s) {
    c.assign((size_t)n_ctx * 64, 0.0f); s.assign((size_t)n_ctx * 64, 0.0f);
    for (int p = 0; p < n_ctx; p++)
        for (int i = 0; i < 64; i++) {
            const double inv = std::pow((double)rope_base, -(double)i / 64.0);
            const double ang = (double)p * inv;
            c[(size_t)p * 64 + i] = (float)std::cos(ang);
            s[(size_t)p * 64 + i] = (float)std::sin(ang);
        }
}

int plan_attention(const AttnPlanIn& a) {
    if (a.ggml_mode) return ATTN_GGML;
    // the single-wave form: wide steps of one token per sequence, two q heads per kv head
    if (a.short_attn_min > 0 && a.ntok >= a.short_attn_min && !a.same_seq && a.n_head == 2 * a.n_kv)
        return a.ntok <= a.hpw1_max ? ATTN_SHORT1 : ATTN_SHORT2;
    // k_attention_fused belongs to the 5-launch layer path (quantised weights, at most fused_max_tok tokens, one token per sequence)
    if (!a.float_mode && a.fused && a.ntok <= a.fused_max_tok && !a.same_seq) return ATTN_FUSED;
    return ATTN_UNFUSED;
}

int Transformer::attention_form(int ntok) const {
    AttnPlanIn a;
    a.ntok = ntok; a.fused = fused; a.fused_max_tok = fused_max_tok_; a.same_seq = same_seq_; a.short_attn_min = short_attn_min_;
    a.n_head = hp_.n_head; a.n_kv = hp_.n_kv; a.hpw1_max = short_attn_hpw1_max(); a.float_mode = float_mode_; a.ggml_mode = ggml_mode_;
    return plan_attention(a);
}

// second context over the same weights: see transformer.h
Transformer::Transformer(const Transformer& o, int max_tok)
    : fused(o.fused), float_mode_(o.float_mode_), foutput_(o.foutput_), hp_(o.hp_), n_ctx_(o.n_ctx_), max_tok_(max_tok), layers_(o.layers_), output_(o.output_),
      output_norm_(o.output_norm_), ws_(o.ws_), weight_bytes_(o.weight_bytes_), layer_weight_bytes_(o.layer_weight_bytes_),
      ggml_mode_(o.ggml_mode_), gg_layers_(o.gg_layers_), gg_output_(o.gg_output_) {
    alloc_workspace();
}

void Transformer::alloc_workspace() {
    const int d = hp_.n_embd, dq = hp_.n_head * 128, dkv = hp_.n_kv * 128, ff = hp_.n_ff;
    nparts_d_ = ((ff >> 8) + 7) / 8;
    const size_t T = (size_t)max_tok_;
    scratch_.alloc(T * 32); hid_.alloc(T * d); big_logits_.alloc(T * 2176);
    if (float_mode_) { xnf_.alloc(T * d); attf_.alloc(T * dq); actf_.alloc(T * ff); }
    h_.alloc(T * d); h2_.alloc(T * d); parts_o_.alloc(T * d); parts_d_.alloc((size_t)nparts_d_ * T * d);
    qkv_.alloc(T * (dq + 2 * dkv)); qrot_.alloc(T * dq); gu_.alloc(T * 2 * ff);
    const size_t mx = (size_t)(d > dq ? d : dq);
    xq_.alloc(T * mx); xd_.alloc(T * mx / 32); aq_.alloc(T * dq); ad_.alloc(T * dq / 32); fq_.alloc(T * ff); fd_.alloc(T * ff / 32);
    if (ggml_mode_) {
        const size_t kmax = (size_t)std::max(std::max(d, dq), ff);
        gg_q8_.alloc(T * kmax); gg_qk_.alloc(T * kmax); gg_d8_.alloc(T * kmax / 32); gg_dk_.alloc(T * kmax / 256); gg_bs_.alloc(T * kmax / 16);
        gg_xn_.alloc(T * kmax); gg_att_.alloc(T * dq); gg_act_f_.alloc(T * ff); gg_scores_.alloc(T * hp_.n_head * (size_t)n_ctx_);
        gg_act_ = GgAct{gg_q8_.p, gg_d8_.p, gg_qk_.p, gg_dk_.p, gg_bs_.p};
    }
}

// ---- ggml-arithmetic mode (ggml_mode.hip): raw GGUF matrices, llama.cpp's portable arithmetic, bit-exact with the test suite's CPU restatement of the mode ----
GgMat Transformer::gg_load(const Gguf& g, const std::string& name, int n_expect, int k_expect) {
    const GgufTensor& t = g.need(name);
    Q3_CHECK((int)t.ne[0] == k_expect && (int)t.ne[1] == n_expect, "ggml mode: shape of " + name);
    Q3_CHECK(t.type == Q3_T_Q8_0 || t.type == Q3_T_Q5_K || t.type == Q3_T_Q6_K, "ggml mode: type of " + name);
    GgMat m; m.type = t.type; m.n = n_expect; m.k = k_expect;
    m.row_bytes = q3_gguf_row_bytes(t.type, k_expect);
    blobs_.emplace_back(m.row_bytes * (size_t)n_expect);
    blobs_.back().upload(reinterpret_cast<const uint8_t*>(t.data), m.row_bytes * (size_t)n_expect);
    m.p = blobs_.back().p;
    return m;
}
void Transformer::gg_linear(hipStream_t st, const GgMat& w, int row0, int nrows, const float* x, float* out, int out_stride, int ntok) {
    gg_quant(st, x, w.k, gg_act_, ntok);   // (ggml quantises the activations once per matmul call, to the weight type's vec_dot_type)
    gg_matvec(st, w, row0, nrows, gg_act_, out, out_stride, ntok);
}
void Transformer::forward_ggml(hipStream_t st, const Input& in, int ntok, const TokMeta& tm, const KvCache& kv, float* hidden_out) {
    const int d = hp_.n_embd, dq = hp_.n_head * 128, dkv = hp_.n_kv * 128, ff = hp_.n_ff, qs = dq + 2 * dkv;
    gg_load_rows(st, in.x, in.x_stride, nullptr, in.idx_stride, in.idx_keys, d, h_.p, ntok);
    for (int l = 0; l < hp_.n_layer; l++) {
        const Layer& L = layers_[l];
        const GgLayer& G = gg_layers_[l];
        gg_rmsnorm(st, h_.p, L.attn_norm, d, hp_.eps, gg_xn_.p, ntok);
        gg_quant(st, gg_xn_.p, d, gg_act_, ntok);
        gg_matvec(st, G.wq, 0, dq, gg_act_, qkv_.p, qs, ntok);
        gg_matvec(st, G.wk, 0, dkv, gg_act_, qkv_.p + dq, qs, ntok);
        gg_matvec(st, G.wv, 0, dkv, gg_act_, qkv_.p + dq + dkv, qs, ntok);
        gg_qk_rope_append(st, qkv_.p, qs, hp_.n_head, hp_.n_kv, L.q_norm, L.k_norm, hp_.eps, rope_cos_.p, rope_sin_.p, n_ctx_, d_mrope_.p, tm, kv, l, ntok);
        gg_attention(st, qkv_.p, qs, hp_.n_head, hp_.n_kv, tm, kv, l, gg_att_.p, gg_scores_.p, n_ctx_, ntok);
        gg_linear(st, G.wo, 0, d, gg_att_.p, parts_o_.p, d, ntok);
        gg_add(st, h_.p, parts_o_.p, (size_t)ntok * d);
        gg_rmsnorm(st, h_.p, L.ffn_norm, d, hp_.eps, gg_xn_.p, ntok);
        gg_quant(st, gg_xn_.p, d, gg_act_, ntok);
        gg_matvec(st, G.gate, 0, ff, gg_act_, gu_.p, ff, ntok);
        gg_matvec(st, G.up, 0, ff, gg_act_, gu_.p + (size_t)ntok * ff, ff, ntok);
        gg_swiglu(st, gu_.p, gu_.p + (size_t)ntok * ff, gg_act_f_.p, (size_t)ntok * ff);
        gg_linear(st, G.down, 0, d, gg_act_f_.p, parts_o_.p, d, ntok);
        gg_add(st, h_.p, parts_o_.p, (size_t)ntok * d);
    }
    gg_rmsnorm(st, h_.p, output_norm_, d, hp_.eps, hid_.p, ntok);
    if (hidden_out) launch_copy_f32(st, hid_.p, hidden_out, (size_t)ntok * d);
    Q3_LAUNCH_CHECK();
}


// one launch (or none) bracketed by the optional event timer, accounted as `bytes` of weight traffic
template <class F> static void timed(LaunchTimer* t, hipStream_t st, double bytes, F&& launch) {
    if (t) t->begin(st);
    launch();
    if (t) t->end(st, bytes);
}

void Transformer::gemv(hipStream_t st, const Q8Mat& w, int row0, int nrows, const int8_t* xq, const uint16_t* xd, float* out,
                       int out_stride, int ntok) {
    timed(timer, st, (double)nrows * ((double)w.K + (double)(w.K / 32) * 2.0), [&] { launch_gemv_q8(st, w, row0, nrows, xq, xd, out, out_stride, ntok); });
}

// ---- the layer walk: forward() runs every non-ggml path through these steps; each picks its launch from the Pass ----
void Transformer::norm(const Pass& s, const NormPro& a) {
    if (s.wgnorm) launch_rmsnorm_quant_wg(s.st, a, hp_.n_embd, xq_.p, xd_.p, s.ntok); // batched steps: workgroup-per-token kernel (same arithmetic, one global round trip)
    else launch_rmsnorm_quant(s.st, norm_args(a, hp_.n_embd, xq_.p, xd_.p), s.ntok);  // (the int8 copy is unused in float mode)
}

// out[ntok][N] (super-segment slabs when quantised) = the whole matrix times the step's activations: int8 blocks, or f32 rows in float mode
void Transformer::linear(const Pass& s, const Q8Mat& w, const FMat& fw, const float* xf, const int8_t* xq, const uint16_t* xd, float* out) {
    if (float_mode_) timed(timer, s.st, (double)fw.bytes(), [&] { launch_gemv_float(s.st, fw, 0, fw.N, xf, fw.K, out, fw.N, s.ntok); });
    else gemv(s.st, w, 0, w.N, xq, xd, out, w.N, s.ntok);
}

void Transformer::qkv(const Pass& s, const Layer& L, const NormPro& a) {
    if (!s.fused) { norm(s, a); linear(s, L.wqkv, L.fqkv, xnf_.p, xq_.p, xd_.p, qkv_.p); return; }
    timed(timer, s.st, (double)L.wqkv.bytes(), [&] { launch_gemv_q8_norm(s.st, L.wqkv, 0, L.wqkv.N, a, qkv_.p, L.wqkv.N, s.ntok, nullptr); });
}

void Transformer::attention(const Pass& s, const Layer& L, int l, const QkvRows& rows) {
    float* att = float_mode_ ? attf_.p : nullptr; // f32 rows for the float o-projection; the int8 copy (aq_, ad_) is always written
    if (s.af == ATTN_SHORT1 || s.af == ATTN_SHORT2)
        launch_attention_short(s.st, s.af == ATTN_SHORT1 ? 1 : 2, rows, hp_.n_head, hp_.n_kv, L.q_norm, L.k_norm, hp_.eps, rope_cos_.p, rope_sin_.p,
                               n_ctx_, d_mrope_.p, s.tm, s.kv, l, aq_.p, ad_.p, s.ntok, att);
    else if (s.af == ATTN_FUSED)
        launch_attention_fused(s.st, rows, hp_.n_head, hp_.n_kv, L.q_norm, L.k_norm, hp_.eps, rope_cos_.p, rope_sin_.p, n_ctx_, d_mrope_.p, s.tm,
                               s.kv, l, aq_.p, ad_.p, s.ntok);
    else {
        launch_qk_rope_append(s.st, rows, nullptr, hp_.n_head, hp_.n_kv, L.q_norm, L.k_norm, hp_.eps, rope_cos_.p, rope_sin_.p, n_ctx_, d_mrope_.p,
                              s.tm, s.kv, l, qrot_.p, s.ntok);
        launch_attention(s.st, qrot_.p, hp_.n_head, hp_.n_kv, s.tm, s.kv, l, att, aq_.p, ad_.p, s.ntok);
    }
}

// ffn norm + gate/up + SwiGLU -> the down-projection's activations (fq_ / fd_, or actf_ in float mode)
void Transformer::gate_up(const Pass& s, const Layer& L, const NormPro& b) {
    const int d = hp_.n_embd, ff = hp_.n_ff;
    LaunchTimer* tg = timer_gu ? timer_gu : timer; // the talker's gate/up launch is timed on its own (bench roofline kernel)
    const double bytes = float_mode_ ? (double)L.fgu.bytes() : (double)L.wgu.bytes();
    if (s.fused) { timed(tg, s.st, bytes, [&] { launch_gateup_swiglu(s.st, L.wgu, ff, b, fq_.p, fd_.p, s.ntok); }); return; }
    norm(s, b);
    LinearPlanIn in; // plan first, then run: a fused gate/up form, or the matmul (the timed launch) and k_swiglu_*
    if (float_mode_) {
        in.op = LOP_F_GATEUP; in.K = d; in.nrows = 2 * ff; in.ntok = s.ntok; in.wts = L.fgu.type; in.has_wt = L.fgu.wt != nullptr;
        in.x_stride = d; in.x_addr = (uintptr_t)xnf_.p;
    } else { in = linear_plan_in(LOP_GATEUP, L.wgu, 0, 2 * ff, s.ntok); in.aq_addr = (uintptr_t)fq_.p; in.fused = fused; }
    in.ff = ff;
    const LinearPlan p = plan_linear(in);
    timed(tg, s.st, bytes, [&] {
        if (p.form == LIN_F_GU_MFMA16) run_gateup_float(s.st, p, L.fgu, ff, xnf_.p, d, actf_.p, s.ntok);
        else if (p.form == LIN_F_GU_UNFUSED) launch_gemv_float(s.st, L.fgu, 0, 2 * ff, xnf_.p, d, gu_.p, 2 * ff, s.ntok);
        else if (p.form == LIN_GU_UNFUSED) launch_gemv_q8(s.st, L.wgu, 0, 2 * ff, xq_.p, xd_.p, gu_.p, 2 * ff, s.ntok);
        else run_gateup_q8(s.st, p, L.wgu, ff, xq_.p, xd_.p, fq_.p, fd_.p, s.ntok);
    });
    if (p.form == LIN_F_GU_UNFUSED) launch_swiglu_f32(s.st, gu_.p, ff, actf_.p, s.ntok);
    else if (p.form == LIN_GU_UNFUSED) launch_swiglu_quant(s.st, gu_.p, ff, fq_.p, fd_.p, s.ntok);
}

void Transformer::forward(hipStream_t st, const Input& in, int ntok, const TokMeta& tm, const KvCache& kv, float* hidden_out) {
    Q3_CHECK(ntok >= 1 && ntok <= max_tok_, "ntok out of range");
    Q3_CHECK(!in.qkv0 || (in.idx_keys && !ggml_mode_), "layer-0 q/k/v rows need the argmax keys that select them (and are not for the ggml mode)");
    const int d = hp_.n_embd, qs = (hp_.n_head + 2 * hp_.n_kv) * 128;
    Pass s{st, ntok, tm, kv, attention_form(ntok), false, false};
    last_fused_ = false; last_ntok_ = ntok;
    if (s.af == ATTN_GGML) { forward_ggml(st, in, ntok, tm, kv, hidden_out); return; }
    Q3_CHECK(!float_mode_ || s.af != ATTN_FUSED, "float mode has no fused attention form");
    // 5 launches per layer (norms as GEMV prologues) for quantised decode steps; batched steps (ntok > fused_max_tok_) and float weights take the
    // unfused sequence, whose GEMMs are weight-stationary over the tokens
    last_fused_ = s.fused = !float_mode_ && fused && ntok <= fused_max_tok_;
    LinearPlanIn npi; npi.op = LOP_NORM; npi.ntok = ntok;
    s.wgnorm = plan_linear(npi).form == LIN_NORM_WG;
    // Residual stream.  Fused: it ping-pongs h_ <-> h2_, because a fused prologue may not overwrite what other workgroups still read.  Unfused and
    // float: the norm kernels run in place on h_ (the wg kernel forbids h_out aliasing h_in only across workgroups; there each token is one workgroup).
    float* hb = s.fused ? h2_.p : h_.p;
    const int npd = float_mode_ ? 1 : nparts_d_; // slabs of the down-projection: the float matmul writes whole sums
    float* xn = float_mode_ ? xnf_.p : nullptr;  // float mode: the next matmul reads the f32 norm output
    auto pro = [&](const float* h_in, const float* parts, int nparts, float* h_out, const float* g, float* xn_out) {
        NormPro a{};
        a.h_in = h_in; a.h_stride = d; a.parts = parts; a.nparts = nparts; a.parts_stride = d; a.parts_slab = (size_t)ntok * d;
        a.h_out = h_out; a.g = g; a.eps = hp_.eps; a.xn_out = xn_out;
        return a;
    };
    for (int l = 0; l < hp_.n_layer; l++) {
        const Layer& L = layers_[l];
        NormPro a = pro(hb, parts_d_.p, npd, h_.p, L.attn_norm, xn); // the previous layer's down-projection is consumed here
        if (l == 0) { a.h_in = in.x; a.h_stride = in.x_stride; a.idx_keys = in.idx_keys; a.idx_stride = in.idx_stride; a.parts = nullptr; a.nparts = 0; }
        NormPro b = pro(h_.p, parts_o_.p, 1, hb, L.ffn_norm, xn);
        const bool tab0 = l == 0 && in.qkv0; // layer 0's q/k/v come from the caller's table: no norm, no projection, and h_ is not written
        if (tab0) { b.h_in = in.x; b.h_stride = in.x_stride; b.idx_keys = in.idx_keys; b.idx_stride = in.idx_stride; }
        else qkv(s, L, a);
        attention(s, L, l, tab0 ? QkvRows(in.qkv0, in.qkv0_stride, in.idx_keys, in.idx_stride) : QkvRows(qkv_.p, qs));
        linear(s, L.wo, L.fo, attf_.p, aq_.p, ad_.p, parts_o_.p);
        gate_up(s, L, b);
        linear(s, L.wdown, L.fdown, actf_.p, fq_.p, fd_.p, parts_d_.p);
    }
    if (s.fused) { if (hidden_out) head(st, 0, ntok, 0, 0, nullptr, 0, nullptr, -1, hidden_out); } // the final norm is the prologue of head()
    else {
        norm(s, pro(h_.p, parts_d_.p, npd, nullptr, output_norm_, hidden_out ? hidden_out : hid_.p));
        if (float_mode_ && hidden_out) launch_copy_f32(st, hidden_out, hid_.p, (size_t)ntok * d); // head() reads hid_
    }
    Q3_LAUNCH_CHECK();
}

// out[r] = layer 0's attention norm + q/k/v projection of row r of x, through the unfused steps of the layer walk (norm, linear) in chunks of
// max_tok rows.  The norm works per token and every linear form gives the same bits, so a row equals what forward() computes for that input
// in any step; a caller with a table of possible inputs builds the rows once and passes them as Input::qkv0.
void Transformer::build_layer0_qkv(hipStream_t st, const float* x, int x_stride, int64_t rows, float* out) {
    Q3_CHECK(!ggml_mode_, "the ggml mode takes no layer-0 q/k/v rows");
    const int d = hp_.n_embd, qs = (hp_.n_head + 2 * hp_.n_kv) * 128;
    const Layer& L = layers_[0];
    const TokMeta tm{nullptr, nullptr, nullptr}; const KvCache kv{}; // (the two steps touch neither)
    for (int64_t r0 = 0; r0 < rows; r0 += max_tok_) {
        const int n = (int)std::min<int64_t>(max_tok_, rows - r0);
        Pass s{st, n, tm, kv, ATTN_UNFUSED, false, false};
        LinearPlanIn npi; npi.op = LOP_NORM; npi.ntok = n;
        s.wgnorm = plan_linear(npi).form == LIN_NORM_WG;
        NormPro a{};
        a.h_in = x + (size_t)r0 * x_stride; a.h_stride = x_stride; a.parts_stride = d; a.g = L.attn_norm; a.eps = hp_.eps;
        a.xn_out = float_mode_ ? xnf_.p : nullptr;
        norm(s, a);
        linear(s, L.wqkv, L.fqkv, xnf_.p, xq_.p, xd_.p, out + (size_t)r0 * qs);
    }
    Q3_LAUNCH_CHECK();
}

void Transformer::head(hipStream_t st, int tok0, int tok_count, int row0, int nrows, float* logits, int logits_stride,
                       const ArgmaxEpi* am, int nrows_valid, float* hidden_out) {
    head_impl(st, tok0, tok_count, row0, nrows, logits, logits_stride, am, nrows_valid, hidden_out);
    Q3_LAUNCH_CHECK();
}
void Transformer::head_impl(hipStream_t st, int tok0, int tok_count, int row0, int nrows, float* logits, int logits_stride,
                            const ArgmaxEpi* am, int nrows_valid, float* hidden_out) {
    const int d = hp_.n_embd, nv = nrows_valid > 0 ? nrows_valid : nrows;
    Q3_CHECK(row0 % 32 == 0 && (float_mode_ || row0 + nrows <= output_.Npad), "head row range");
    if (last_fused_) {
        // final RMSNorm (+ last down-proj partials + residual) as the prologue of the output-matrix GEMV
        NormPro f{};
        f.h_in = h2_.p + (size_t)tok0 * d; f.h_stride = d;
        f.parts = parts_d_.p + (size_t)tok0 * d; f.nparts = nparts_d_; f.parts_stride = d;
        f.parts_slab = (size_t)last_ntok_ * d; // slabs are [p][ntok of the forward that wrote them][d]
        f.g = output_norm_; f.eps = hp_.eps; f.xn_out = hidden_out;
        if (nrows <= 0) // hidden only: run the prologue through a 32-row GEMV whose output is discarded
            timed(timer, st, 32.0 * ((double)d * 1.0625), [&] { launch_gemv_q8_norm(st, output_, 0, 32, f, scratch_logits(tok_count), 32, tok_count, nullptr); });
        else
            timed(timer, st, (double)nrows * ((double)d * 1.0625),
                  [&] { launch_gemv_q8_norm(st, output_, row0, am ? nv : nrows, f, am ? nullptr : logits, am ? 0 : logits_stride, tok_count, am); });
        return;
    }
    // the final-norm hidden states are in hid_ (f32) and xq_ / xd_ (int8): one matmul by mode; with an argmax epilogue, logits to scratch, then the keys
    if (hidden_out) launch_copy_f32(st, hid_.p + (size_t)tok0 * d, hidden_out, (size_t)tok_count * d);
    if (nrows <= 0) return;
    float* dst = am ? big_logits_.p : logits;
    const int ls = am ? nrows : logits_stride;
    if (am && big_logits_.n < (size_t)tok_count * nrows) throw Error("head scratch too small");
    int nr = nrows;
    if (ggml_mode_) { // quantise hid_ for the output matrix's type, plain dots
        nr = std::min(nrows, gg_output_.n - row0); // (callers pass row counts padded to 32)
        gg_linear(st, gg_output_, row0, nr, hid_.p + (size_t)tok0 * d, dst, ls, tok_count);
    } else if (float_mode_)
        timed(timer, st, (double)nrows * d * (foutput_.type == Q3_T_F32 ? 4 : 2),
              [&] { launch_gemv_float(st, foutput_, row0, nrows, hid_.p + (size_t)tok0 * d, d, dst, ls, tok_count); });
    else gemv(st, output_, row0, nrows, xq_.p + (size_t)tok0 * d, xd_.p + (size_t)tok0 * (d / 32), dst, ls, tok_count);
    if (am) launch_argmax_keys(st, big_logits_.p, nrows, std::min(nv, nr), am->mask_per_tok, am->keys, am->key_stride, tok_count);
}

// ------------------------------------------------------------------------------------------------
KvPool::KvPool(int n_layer, int n_kv, int n_pages, int n_seq, int max_pages_per_seq)
    : n_layer_(n_layer), n_kv_(n_kv), n_pages_(n_pages), n_seq_(n_seq), max_pages_(max_pages_per_seq) {
    const size_t per_page = (size_t)n_layer * n_kv * 8192;
    k_.alloc(per_page * n_pages); v_.alloc(per_page * n_pages);
    k_.zero(); v_.zero();
    const size_t nt = (size_t)n_seq * max_pages_per_seq;
    Q3_HIP(hipHostMalloc((void**)&table_, nt * sizeof(int32_t)));
    std::fill(table_, table_ + nt, 0);
    d_table_.alloc(nt);
    d_table_.upload(table_, nt);
    for (int p = n_pages - 1; p >= 0; p--) free_.push_back(p);
    used_pages_.assign(n_seq, 0);
}
KvCache KvPool::view() const {
    KvCache c;
    c.k = k_.p; c.v = v_.p; c.page_table = d_table_.p; c.max_pages = max_pages_; c.n_layer = n_layer_; c.n_kv = n_kv_;
    return c;
}
int KvPool::alloc_page() { Q3_CHECK(!free_.empty(), "KV pool exhausted"); int p = free_.back(); free_.pop_back(); return p; }
void KvPool::free_page(int p) { free_.push_back(p); }
void KvPool::assign(int seq, int lp, int pp) {
    table_[(size_t)seq * max_pages_ + lp] = pp;
    Q3_HIP(hipMemcpy(d_table_.p + (size_t)seq * max_pages_ + lp, &pp, 4, hipMemcpyHostToDevice));
}
int KvPool::grow(int seq, int n_positions) {
    const int need = (n_positions + 63) / 64;
    Q3_CHECK(seq >= 0 && seq < n_seq_, "KV sequence index out of range");
    Q3_CHECK(need <= max_pages_ && need <= n_pages_, "sequence exceeds max pages");
    const int first = used_pages_[seq];
    Q3_CHECK(need - first <= (int)free_.size(), "KV pool exhausted"); // all or nothing: a failed call leaves the tables as they were
    while (used_pages_[seq] < need) { table_[(size_t)seq * max_pages_ + used_pages_[seq]] = alloc_page(); used_pages_[seq]++; }
    return first;
}
void KvPool::ensure(int seq, int n_positions) {
    const int first = grow(seq, n_positions);
    for (int lp = first; lp < used_pages_[seq]; lp++) assign(seq, lp, page(seq, lp));
}
void KvPool::ensure(int seq, int n_positions, hipStream_t st) {
    const int first = grow(seq, n_positions), n_new = used_pages_[seq] - first;
    if (n_new > 0) // rows of other sequences are untouched, and this row is not rewritten before `st` is synchronised by the caller
        Q3_HIP(hipMemcpyAsync(d_table_.p + (size_t)seq * max_pages_ + first, table_ + (size_t)seq * max_pages_ + first, (size_t)n_new * 4,
                              hipMemcpyHostToDevice, st));
}
KvPool::~KvPool() { if (table_) (void)hipHostFree(table_); }
void KvPool::release(int seq) {
    Q3_CHECK(seq >= 0 && seq < n_seq_, "KV sequence index out of range");
    for (int i = 0; i < used_pages_[seq]; i++) free_page(table_[(size_t)seq * max_pages_ + i]);
    used_pages_[seq] = 0;
}

} // namespace q3
