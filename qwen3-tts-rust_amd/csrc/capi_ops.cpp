// capi_ops.cpp -- kernel-level C-ABI entry points for the parity tests (host buffers in, host buffers out).
#include "../../include/q3tts.h"
#include "transformer.h"
#include "host_logic.h"
#include "kdev.h"
#include "codec.h"
#include "kernels.h"
#include "out_stages.h"
#include "pcm_out.h"
#include "tsm.h"
#include "pitch.h"
#include "volume.h"
#include "loudness.h"
#include "intake.h"
#include <memory>
#include "mel.h"

using namespace q3;
#define Q3_API_BEGIN try {
#define Q3_API_END(failval) } catch (const std::exception& ex) { set_last_error(ex.what()); return failval; } catch (...) { set_last_error("unknown error"); return failval; }
static void require_gpu() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error("no HIP device available: the HIP path is the only compute path (no CPU fallback)");
}

// ---- q3tts_op_attention: one layer's attention step through the Transformer's launchers ----
static int attention_op_plan(const q3tts_attention_desc& d) {
    AttnPlanIn a;
    a.ntok = d.ntok; a.fused = d.fused != 0; a.fused_max_tok = d.fused_max_tok; a.same_seq = d.same_seq != 0; a.short_attn_min = d.short_attn_min;
    a.n_head = d.n_head; a.n_kv = d.n_kv; a.hpw1_max = d.hpw1_max > 0 ? d.hpw1_max : short_attn_hpw1_max();
    a.float_mode = d.float_mode != 0; a.ggml_mode = d.ggml_mode != 0;
    return plan_attention(a);
}

// every precondition of the form, checked on the host before anything is allocated or launched
static void attention_op_check(const q3tts_attention_desc& d, int form) {
    Q3_CHECK(form >= ATTN_UNFUSED && form <= ATTN_GGML, "unknown attention form");
    Q3_CHECK(d.n_head >= 1 && d.n_kv >= 1 && d.n_head % d.n_kv == 0, "n_head must be a multiple of n_kv");
    Q3_CHECK(d.n_layer >= 1 && d.layer >= 0 && d.layer < d.n_layer && d.ntok >= 1 && d.ntok <= 65535, "bad layer / token count");
    Q3_CHECK(d.qkv && d.q_norm && d.k_norm && d.k_cache && d.v_cache && d.qkv_stride >= (d.n_head + 2 * d.n_kv) * 128, "bad qkv / norm / cache buffers");
    Q3_CHECK(d.n_ctx >= 1 && d.n_pages >= 1, "bad n_ctx / n_pages");
    if (form != ATTN_GGML) Q3_CHECK(d.aq && d.ad, "aq / ad are required");
    else Q3_CHECK(d.att, "the ggml form produces att only");
    if (d.uniform_pos < 0) Q3_CHECK(d.seq && d.slot && d.pos, "per-token seq / slot / pos are required without uniform_pos");
    if (d.page_table) {
        Q3_CHECK(d.n_seq >= 1 && d.max_pages >= 1, "bad page table shape");
        for (int64_t i = 0; i < (int64_t)d.n_seq * d.max_pages; i++)
            Q3_CHECK(d.page_table[i] >= 0 && d.page_table[i] < d.n_pages, "page table entry out of range");
    }
    const bool short_form = form == ATTN_SHORT1 || form == ATTN_SHORT2;
    if (short_form) Q3_CHECK(d.n_head == 2 * d.n_kv, "the short forms need n_head == 2 * n_kv");
    std::map<std::pair<int, int>, int> seen;   // (seq, slot) -> tokens
    std::map<int, int> per_seq;
    for (int t = 0; t < d.ntok; t++) {
        const int seq = d.uniform_pos >= 0 ? t : d.seq[t], slot = d.uniform_pos >= 0 ? d.uniform_pos : d.slot[t];
        Q3_CHECK(slot >= 0 && slot < d.n_ctx, "slot out of [0, n_ctx)");
        if (d.page_table) Q3_CHECK(seq >= 0 && seq < d.n_seq && slot < d.max_pages * 64, "sequence or slot beyond the page table");
        else Q3_CHECK(seq >= 0 && seq < d.n_pages && slot < 64, "identity paging: sequence beyond the cache or slot beyond its one page");
        if (short_form) Q3_CHECK(slot < 64, "the short forms read page 0 only: slot must be < 64");
        Q3_CHECK(seen[std::make_pair(seq, slot)]++ == 0, "two tokens write the same (sequence, slot)");
        if (++per_seq[seq] > 1) Q3_CHECK(form == ATTN_UNFUSED || form == ATTN_GGML, "the fused and short forms need one token per sequence");
    }
}

// keys set (q3tts_op_attention_keyed): d.qkv is a table of qkv_rows rows and token t reads row key_code(keys[t * key_stride]); the table is
// written back whole
static void attention_op_run(q3tts_attention_desc* dp, const uint64_t* keys = nullptr, int key_stride = 0, int qkv_rows = 0) {
    Q3_CHECK(dp, "null attention descriptor");
    q3tts_attention_desc& d = *dp;
    Q3_CHECK(d.ntok >= 1 && d.n_head >= 1 && d.n_kv >= 1, "bad attention shape");
    const int form = d.form == Q3TTS_ATTN_AUTO ? attention_op_plan(d) : d.form;
    attention_op_check(d, form);
    const int nt = d.ntok, dq = d.n_head * 128, qs = d.qkv_stride;
    DevBuf<q3_u64> dkeys;
    if (keys) {
        Q3_CHECK(form != ATTN_GGML, "the ggml form reads no keyed rows");
        Q3_CHECK(key_stride >= 1 && qkv_rows >= 1, "bad key stride / table rows");
        for (int t = 0; t < nt; t++) {
            const int c = key_code(keys[(size_t)t * key_stride]);
            Q3_CHECK(c >= 0 && c < qkv_rows, "a key selects a row outside the table");
        }
        dkeys.alloc((size_t)(nt - 1) * key_stride + 1); dkeys.upload((const q3_u64*)keys, dkeys.n);
    }
    DevBuf<float> qkv((size_t)(keys ? qkv_rows : nt) * qs); qkv.upload(d.qkv, qkv.n);
    const QkvRows rows(qkv.p, qs, dkeys.p, key_stride);
    DevBuf<float> qn(128), kn(128); qn.upload(d.q_norm, 128); kn.upload(d.k_norm, 128);
    std::vector<float> hc, hs;
    build_rope_tables(d.rope_base, d.n_ctx, hc, hs);
    DevBuf<float> rc(hc.size()), rs(hs.size()); rc.upload(hc.data(), hc.size()); rs.upload(hs.data(), hs.size());
    DevBuf<int32_t> sec(4); sec.upload(d.mrope_sec, 4);
    DevBuf<int32_t> dseq, dslot, dpos, dtab;
    TokMeta tm{nullptr, nullptr, nullptr};
    if (d.uniform_pos >= 0) tm.uniform_pos = d.uniform_pos;
    else {
        dseq.alloc(nt); dseq.upload(d.seq, nt); dslot.alloc(nt); dslot.upload(d.slot, nt); dpos.alloc((size_t)nt * 4); dpos.upload(d.pos, (size_t)nt * 4);
        tm.seq = dseq.p; tm.slot = dslot.p; tm.pos = dpos.p;
    }
    const size_t cache_halfs = (size_t)d.n_pages * d.n_layer * d.n_kv * 8192;
    DevBuf<uint16_t> kc(cache_halfs), vc(cache_halfs);
    kc.upload(d.k_cache, cache_halfs); vc.upload(d.v_cache, cache_halfs);
    KvCache kv;
    kv.k = kc.p; kv.v = vc.p; kv.page_table = nullptr; kv.max_pages = d.page_table ? d.max_pages : 1; kv.n_layer = d.n_layer; kv.n_kv = d.n_kv;
    if (d.page_table) { dtab.alloc((size_t)d.n_seq * d.max_pages); dtab.upload(d.page_table, dtab.n); kv.page_table = dtab.p; }
    DevBuf<float> att((size_t)nt * dq), qrot, scores;
    DevBuf<int8_t> aq((size_t)nt * dq); DevBuf<uint16_t> ad((size_t)nt * (dq / 32));
    switch (form) {
    case ATTN_UNFUSED:
        qrot.alloc((size_t)nt * dq);
        launch_qk_rope_append(0, rows, nullptr, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv, d.layer, qrot.p, nt);
        launch_attention(0, qrot.p, d.n_head, d.n_kv, tm, kv, d.layer, att.p, aq.p, ad.p, nt);
        break;
    case ATTN_FUSED:
        launch_attention_fused(0, rows, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv, d.layer, aq.p, ad.p, nt);
        break;
    case ATTN_SHORT1: case ATTN_SHORT2:
        launch_attention_short(0, form == ATTN_SHORT1 ? 1 : 2, rows, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv,
                               d.layer, aq.p, ad.p, nt, att.p);
        break;
    default: // ATTN_GGML: q is rotated in place in the qkv copy
        scores.alloc((size_t)nt * d.n_head * d.n_ctx);
        gg_qk_rope_append(0, qkv.p, qs, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv, d.layer, nt);
        gg_attention(0, qkv.p, qs, d.n_head, d.n_kv, tm, kv, d.layer, att.p, scores.p, d.n_ctx, nt);
        break;
    }
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    kc.download(d.k_cache, cache_halfs); vc.download(d.v_cache, cache_halfs);
    if (d.att && form != ATTN_FUSED) att.download(d.att, att.n);
    if (form != ATTN_GGML) { aq.download(d.aq, aq.n); ad.download(d.ad, ad.n); }
    if (keys) qkv.download(const_cast<float*>(d.qkv), qkv.n);
    d.form_ran = form;
}

// ---- q3tts_op_linear: one linear-layer operation through the same run_* launches as the engine ----
static bool lin_quant(const q3tts_linear_desc& d) { return d.op <= LOP_NORM_GATEUP && d.op != LOP_NORM; }
static bool lin_kq(const q3tts_linear_desc& d) {
    if (d.kq_layout || d.nw > 1) return true;
    return d.type[0] != Q3_T_Q8_0;
}
static int lin_rows(const q3tts_linear_desc& d) { int n = 0; for (int i = 0; i < d.nw; i++) n += d.rows[i]; return n; }
static int lin_wts(const q3tts_linear_desc& d) { // wslice_ts of the matrix kqmat_from_host builds (tensors of one type in a row merge)
    if (d.op >= LOP_F_GEMV) return d.type[0];
    if (!lin_kq(d)) return 0;
    int n = 0, last = -1;
    for (int i = 0; i < d.nw; i++) if (d.type[i] != last) { n++; last = d.type[i]; }
    return n == 1 ? d.type[0] : -1;
}
static LinearPlanIn lin_plan_in(const q3tts_linear_desc& d) {
    LinearPlanIn in;
    in.op = d.op; in.K = d.K; in.row0 = d.row0; in.nrows = d.nrows; in.ntok = d.ntok; in.ff = d.ff;
    in.kq = lin_quant(d) && lin_kq(d); in.wts = lin_wts(d); in.has_wt = true;
    if (in.kq) { int n = 0, last = -1; for (int i = 0; i < d.nw; i++) if (d.type[i] != last) { n++; last = d.type[i]; } in.kq_parts = n; }
    in.out_stride = d.out_stride; in.out_addr = (uintptr_t)d.out_off * 4 + (d.out ? (uintptr_t)d.out : 0);
    in.x_stride = d.x_stride; in.x_addr = (uintptr_t)d.x_off * 4 + (d.x ? (uintptr_t)d.x : 0);
    in.aq_addr = 0; in.fused = d.fused != 0;
    return in;
}
static LinearPlan lin_plan(const q3tts_linear_desc& d) {
    Q3_CHECK(d.op >= LOP_GEMV && d.op <= LOP_F_GATEUP, "unknown linear op");
    Q3_CHECK(d.K >= 256 && d.K % 256 == 0 && d.ntok >= 1 && d.ntok <= 65535 && d.nrows >= 1 && d.row0 >= 0, "bad linear shape");
    return plan_linear(lin_plan_in(d));
}
static bool in_set(int v, std::initializer_list<int> s) { for (int x : s) if (v == x) return true; return false; }
static int op_of_form(int f) {
    if (f == LIN_GEMM_Q8_WIDE) return LOP_GEMV;
    if (f == LIN_GU_Q8_WIDE) return LOP_GATEUP;
    if (f <= LIN_GEMM_KQ_MFMA) return LOP_GEMV;
    if (f <= LIN_GU_UNFUSED) return LOP_GATEUP;
    if (f <= LIN_NORM_WG) return LOP_NORM;
    if (f == LIN_GEMV_NORM) return LOP_NORM_GEMV;
    if (f == LIN_GEMV_NORM_ARGMAX) return LOP_NORM_ARGMAX;
    if (f == LIN_GU_SWIGLU_NORM) return LOP_NORM_GATEUP;
    if (f <= LIN_F_MFMA) return LOP_F_GEMV;
    return LOP_F_GATEUP;
}
// every precondition of the form (include/q3tts.h), checked on the host before anything is allocated or launched
static void lin_check(const q3tts_linear_desc& d, const LinearPlan& p) {
    const int f = p.form, K = d.K, nt = d.ntok, ntiles = (nt + 31) / 32;
    Q3_CHECK(f >= LIN_GEMV_Q8 && f <= LIN_GU_Q8_WIDE && op_of_form(f) == d.op, "the form does not compute this op");
    const bool quant = lin_quant(d), kq = quant && lin_kq(d), norm = d.op >= LOP_NORM && d.op <= LOP_NORM_GATEUP;
    if (d.op != LOP_NORM) {
        Q3_CHECK(d.nw >= 1 && d.nw <= 3, "1 to 3 weight tensors");
        for (int i = 0; i < d.nw; i++) Q3_CHECK(d.raw[i] && d.rows[i] >= 1, "missing weight tensor");
        if (d.op >= LOP_F_GEMV) Q3_CHECK(d.nw == 1 && (d.type[0] == Q3_T_F32 || d.type[0] == Q3_T_F16 || d.type[0] == Q3_T_BF16), "float ops take one f32 / f16 / bf16 tensor");
        else if (kq) for (int i = 0; i < d.nw; i++) Q3_CHECK(in_set(d.type[i], {Q3_T_Q8_0, Q3_T_Q5_K, Q3_T_Q6_K}) && d.rows[i] % 32 == 0, "K-quant layout: Q8_0 / Q5_K / Q6_K tensors of 32-row multiples");
        Q3_CHECK(d.row0 + d.nrows <= lin_rows(d), "rows past the matrix");
    }
    if (d.op == LOP_GATEUP) Q3_CHECK(K <= 2048, "int8 gate/up: K <= 2048 (k_swiglu_quant reads one super-segment slab)");
    if (d.op == LOP_GATEUP || d.op == LOP_NORM_GATEUP || d.op == LOP_F_GATEUP)
        Q3_CHECK(d.row0 == 0 && d.nrows == 2 * d.ff && d.ff >= 1 && d.ff % (d.op == LOP_F_GATEUP ? 1 : 32) == 0, "gate/up: row0 0, nrows 2 * ff, ff % 32 == 0");
    if (quant && !norm) Q3_CHECK(d.xq && d.xd && d.a_rows >= nt, "int8 activations [a_rows >= ntok][K]");
    if (d.op >= LOP_F_GEMV) Q3_CHECK(d.x && d.x_off >= 0 && d.x_stride >= K && d.x_off + (int64_t)(nt - 1) * d.x_stride + K <= d.x_floats, "float activations out of their buffer");
    if (norm) {
        Q3_CHECK(K <= 2048 && d.h_in && d.g && d.h_stride >= K, "norm prologue: K <= 2048, h_in and g required");
        Q3_CHECK(!(d.idx && d.idx_keys), "idx or idx_keys, not both");
        if (d.idx) Q3_CHECK(f == LIN_NORM, "int32 row indices: NORM only");
        for (int t = 0; t < nt; t++) {
            int64_t row = t;
            if (d.idx) row = d.idx[(size_t)t * d.idx_stride];
            else if (d.idx_keys) row = key_code(d.idx_keys[(size_t)t * d.idx_stride]);
            Q3_CHECK(row >= 0 && row * d.h_stride + K <= d.h_floats, "selected h_in row outside h_in");
        }
        Q3_CHECK(d.nparts >= 0 && (d.nparts == 0 || (d.parts && d.parts_stride >= K && d.parts_slab >= 0 &&
                 (int64_t)(d.nparts - 1) * d.parts_slab + (int64_t)(nt - 1) * d.parts_stride + K <= d.parts_floats)), "residual slabs out of their buffer");
        if (f == LIN_NORM && d.nparts > 1) Q3_CHECK(d.parts_slab == (int64_t)nt * d.parts_stride, "NORM: slabs are ntok * parts_stride apart");
        if (d.op == LOP_NORM) Q3_CHECK(d.xq_out && d.xd_out, "NORM: xq_out / xd_out required");
    }
    if (in_set(d.op, {LOP_GEMV, LOP_NORM_GEMV, LOP_F_GEMV, LOP_F_GATEUP})) {
        const int64_t cols = d.op == LOP_F_GATEUP ? d.ff : d.nrows;
        const int64_t slabs = d.op == LOP_GEMV ? (K / 256 + 7) / 8 : 1;
        Q3_CHECK(d.out && d.out_off >= 0 && d.out_stride >= cols && d.out_off + (slabs * nt - 1) * d.out_stride + cols <= d.out_floats, "output out of its buffer");
    }
    if (in_set(d.op, {LOP_GATEUP, LOP_NORM_GATEUP})) Q3_CHECK(d.aq && d.ad, "gate/up: aq / ad required");
    if (f == LIN_GEMV_NORM_ARGMAX) {
        Q3_CHECK(d.keys && d.key_stride >= 1 && (int64_t)(nt - 1) * d.key_stride < d.n_keys, "argmax keys out of their buffer");
        Q3_CHECK(d.nrows_valid >= 1 && d.nrows_valid <= d.nrows, "1 <= nrows_valid <= nrows");
    }
    const bool q8 = quant && !kq;
    switch (f) {
    case LIN_GEMV_Q8: case LIN_GEMV_KQ:
        Q3_CHECK(f == LIN_GEMV_Q8 ? q8 : kq, "GEMV_Q8 takes the Q8_0 layout, GEMV_KQ the K-quant layout");
        Q3_CHECK(in_set(p.lpr, {2, 4, 8}) && in_set(p.mt, {1, 2, 4, 8}), "lpr in {2,4,8}, mt in {1,2,4,8}");
        break;
    case LIN_GEMM_Q8_TOK: Q3_CHECK(q8, "GEMM_Q8_TOK takes the Q8_0 layout"); break;
    case LIN_GEMM_Q8_MFMA: case LIN_GEMM_KQ_MFMA:
        Q3_CHECK(f == LIN_GEMM_Q8_MFMA ? q8 : kq, "GEMM_Q8_MFMA takes the Q8_0 layout, GEMM_KQ_MFMA the K-quant layout");
        Q3_CHECK(p.z >= 1 && p.z <= ntiles, "1 <= ztiles <= token tiles");
        break;
    case LIN_GEMM_Q8_TILE1:
        Q3_CHECK(q8 && K <= 1024 && d.nrows % 4 == 0 && d.out_stride % 4 == 0 && ((uintptr_t)(d.out + d.out_off) & 15) == 0 && p.z == ntiles,
                 "GEMM_Q8_TILE1: Q8_0, K <= 1024, nrows % 4 == 0, out_stride % 4 == 0, 16-byte out, ztiles == token tiles");
        break;
    case LIN_GU_Q8_TILE1: case LIN_GU_Q8_MFMA: case LIN_GU_KQ_MFMA:
        Q3_CHECK(f == LIN_GU_KQ_MFMA ? (kq && lin_wts(d) != -1) : q8, "GU_Q8_*: Q8_0 layout; GU_KQ_MFMA: K-quant layout of one tensor type");
        Q3_CHECK((K == 1024 || K == 2048) && d.ff % 32 == 0, "fused gate/up: K in {1024, 2048}, ff % 32 == 0");
        Q3_CHECK(p.z >= (ntiles + 3) / 4 && p.z <= ntiles && (f != LIN_GU_Q8_TILE1 || p.z == ntiles), "fused gate/up: ceil(tiles/4) <= ztiles <= tiles (TILE1: == tiles)");
        break;
    case LIN_GEMM_Q8_WIDE: case LIN_GU_Q8_WIDE:
        Q3_CHECK(q8, "GEMM_Q8_WIDE / GU_Q8_WIDE take the Q8_0 layout");
        if (f == LIN_GU_Q8_WIDE) Q3_CHECK((K == 1024 || K == 2048) && d.ff % 32 == 0, "fused gate/up: K in {1024, 2048}, ff % 32 == 0");
        Q3_CHECK(p.z == ntiles, "wide forms: ztiles == token tiles");
        break;
    case LIN_GEMV_NORM: case LIN_GEMV_NORM_ARGMAX: case LIN_GU_SWIGLU_NORM:
        Q3_CHECK(f == LIN_GU_SWIGLU_NORM ? (in_set(p.mt, {1, 2, 4}) && lin_wts(d) != -1) : in_set(p.mt, {1, 2, 4, 8}), "mt out of range / GU_SWIGLU_NORM needs one tensor type");
        Q3_CHECK(f == LIN_GU_SWIGLU_NORM || (f == LIN_GEMV_NORM_ARGMAX ? p.lpr == 2 : in_set(p.lpr, {2, 4, 8})), "GEMV_NORM: lpr in {2,4,8}; ARGMAX: lpr 2");
        break;
    case LIN_F_GEMV: Q3_CHECK(in_set(p.mt, {1, 2, 4, 8}), "mt in {1,2,4,8}"); break;
    case LIN_F_MFMA16: case LIN_F_MFMA: case LIN_F_GU_MFMA16:
        Q3_CHECK(d.row0 % 64 == 0 && ((uintptr_t)(d.x + d.x_off) & 15) == 0 && d.x_stride % 4 == 0, "float matrix-core forms: row0 % 64 == 0, 16-byte x, x_stride % 4 == 0");
        if (f == LIN_F_GU_MFMA16) Q3_CHECK(d.ff % 16 == 0, "F_GU_MFMA16: ff % 16 == 0");
        break;
    default: break;
    }
}
static void lin_run(q3tts_linear_desc* dp) {
    Q3_CHECK(dp, "null linear descriptor");
    q3tts_linear_desc& d = *dp;
    LinearPlan p = lin_plan(d);
    if (d.form != LIN_AUTO) { // forced: the plan's parameters unless given
        Q3_CHECK(d.form >= LIN_GEMV_Q8 && d.form <= LIN_GU_Q8_WIDE, "unknown linear form");
        LinearPlan fp; fp.form = d.form; fp.nseg = d.K / 256;
        const int f = d.form, ntiles = (d.ntok + 31) / 32;
        const int mt_def = d.ntok == 1 ? 1 : d.ntok == 2 ? 2 : d.ntok <= 4 ? 4 : 8;
        fp.mt = d.mt ? d.mt : (p.form == f && p.mt ? p.mt : (f == LIN_GU_SWIGLU_NORM ? (mt_def > 4 ? 4 : mt_def) : mt_def));
        fp.lpr = d.lpr ? d.lpr : (p.form == f && p.lpr ? p.lpr : (f == LIN_GEMV_NORM_ARGMAX ? 2 : 8));
        int zdef = p.form == f && p.z ? p.z : ntiles;
        fp.z = d.ztiles ? d.ztiles : zdef;
        if (f == LIN_GEMM_Q8_WIDE || f == LIN_GU_Q8_WIDE) { fp.mt = 0; fp.lpr = 0; } // (one parameter: ztiles == token tiles)
        p = fp;
    }
    lin_check(d, p);
    const int K = d.K, nt = d.ntok, ff = d.ff;
    // weights
    DevBuf<uint8_t> storage, fw, fwt;
    Q8Mat m; FMat fm;
    if (d.op >= LOP_F_GEMV) {
        const int n = d.rows[0];
        const size_t esz = d.type[0] == Q3_T_F32 ? 4 : 2;
        fw.alloc((size_t)n * K * esz); fw.upload((const uint8_t*)d.raw[0], fw.n);
        fwt.alloc((size_t)((n + 63) / 64) * 64 * K * esz);
        launch_tile_float(0, fw.p, fwt.p, d.type[0], n, K);
        fm.w = fw.p; fm.wt = fwt.p; fm.type = d.type[0]; fm.N = n; fm.K = K;
    } else if (d.op != LOP_NORM) {
        m = lin_kq(d) ? kqmat_from_host(d.raw, d.type, d.rows, d.nw, K, storage) : q8mat_from_host(d.raw[0], d.rows[0], K, storage);
    }
    // inputs
    DevBuf<int8_t> dxq; DevBuf<uint16_t> dxd; DevBuf<float> dx, dh, dparts, dg, dhout, dxn, dout, dgu;
    DevBuf<q3_u64> dkeys_in, dkeys; DevBuf<int32_t> didx, dmask; DevBuf<int8_t> daq, dxq_out; DevBuf<uint16_t> dad, dxd_out;
    if (d.xq) { dxq.alloc((size_t)d.a_rows * K); dxq.upload(d.xq, dxq.n); dxd.alloc((size_t)d.a_rows * (K / 32)); dxd.upload(d.xd, dxd.n); }
    if (d.op >= LOP_F_GEMV) { dx.alloc((size_t)d.x_floats); dx.upload(d.x, dx.n); }
    NormPro a{};
    const bool norm = d.op >= LOP_NORM && d.op <= LOP_NORM_GATEUP;
    if (norm) {
        dh.alloc((size_t)d.h_floats); dh.upload(d.h_in, dh.n);
        dg.alloc(K); dg.upload(d.g, K);
        a.h_in = dh.p; a.h_stride = d.h_stride; a.g = dg.p; a.eps = d.eps; a.idx_stride = d.idx_stride;
        if (d.idx_keys) { dkeys_in.alloc((size_t)(nt - 1) * d.idx_stride + 1); dkeys_in.upload((const q3_u64*)d.idx_keys, dkeys_in.n); a.idx_keys = dkeys_in.p; }
        if (d.idx) { didx.alloc((size_t)(nt - 1) * d.idx_stride + 1); didx.upload(d.idx, didx.n); }
        if (d.nparts > 0) { dparts.alloc((size_t)d.parts_floats); dparts.upload(d.parts, dparts.n); }
        a.parts = dparts.p; a.nparts = d.nparts; a.parts_stride = d.parts_stride; a.parts_slab = (size_t)d.parts_slab;
        if (d.h_out) { dhout.alloc((size_t)nt * K); dhout.upload(d.h_out, dhout.n); a.h_out = dhout.p; }
        if (d.xn_out) { dxn.alloc((size_t)nt * K); dxn.upload(d.xn_out, dxn.n); a.xn_out = dxn.p; }
    }
    if (d.out) { dout.alloc((size_t)d.out_floats); dout.upload(d.out, dout.n); }
    // gate/up outputs: LIN_GUARD elements of 0x5A bytes in front of and behind [ntok][ff] / [ntok][ff/32] on the device; a form that writes one is refused below
    constexpr size_t LIN_GUARD = 64;
    const size_t n_aq = d.aq ? (size_t)nt * ff : 0, n_ad = d.aq ? (size_t)nt * (ff / 32) : 0;
    if (d.aq) {
        daq.alloc(n_aq + 2 * LIN_GUARD); dad.alloc(n_ad + 2 * LIN_GUARD);
        Q3_HIP(hipMemset(daq.p, 0x5A, daq.n)); Q3_HIP(hipMemset(dad.p, 0x5A, dad.n * 2));
        Q3_HIP(hipMemcpy(daq.p + LIN_GUARD, d.aq, n_aq, hipMemcpyHostToDevice)); Q3_HIP(hipMemcpy(dad.p + LIN_GUARD, d.ad, n_ad * 2, hipMemcpyHostToDevice));
    }
    int8_t* const aqp = d.aq ? daq.p + LIN_GUARD : nullptr; uint16_t* const adp = d.aq ? dad.p + LIN_GUARD : nullptr;
    float* out = d.out ? dout.p + d.out_off : nullptr;
    switch (p.form) {
    case LIN_GEMV_Q8: case LIN_GEMM_Q8_TOK: case LIN_GEMM_Q8_MFMA: case LIN_GEMM_Q8_TILE1: case LIN_GEMV_KQ: case LIN_GEMM_KQ_MFMA: case LIN_GEMM_Q8_WIDE:
        run_gemv_q8(0, p, m, d.row0, d.nrows, dxq.p, dxd.p, out, d.out_stride, nt);
        break;
    case LIN_GU_Q8_TILE1: case LIN_GU_Q8_MFMA: case LIN_GU_KQ_MFMA: case LIN_GU_Q8_WIDE:
        run_gateup_q8(0, p, m, ff, dxq.p, dxd.p, aqp, adp, nt);
        break;
    case LIN_GU_UNFUSED: { // what Transformer::forward runs when the fused gate/up form does not apply
        dgu.alloc((size_t)((K / 256 + 7) / 8) * nt * 2 * ff);
        LinearPlanIn gi = linear_plan_in(LOP_GEMV, m, 0, 2 * ff, nt);
        gi.out_stride = 2 * ff; gi.out_addr = (uintptr_t)dgu.p;
        const LinearPlan gp = plan_linear(gi);
        run_gemv_q8(0, gp, m, 0, 2 * ff, dxq.p, dxd.p, dgu.p, 2 * ff, nt);
        launch_swiglu_quant(0, dgu.p, ff, aqp, adp, nt);
        p.lpr = gp.lpr; p.mt = gp.mt; p.z = gp.z;
        break;
    }
    case LIN_NORM: {
        dxq_out.alloc((size_t)nt * K); dxq_out.upload(d.xq_out, dxq_out.n); dxd_out.alloc((size_t)nt * (K / 32)); dxd_out.upload(d.xd_out, dxd_out.n);
        launch_rmsnorm_quant(0, norm_args(a, K, dxq_out.p, dxd_out.p, didx.p), nt);
        break;
    }
    case LIN_NORM_WG:
        dxq_out.alloc((size_t)nt * K); dxq_out.upload(d.xq_out, dxq_out.n); dxd_out.alloc((size_t)nt * (K / 32)); dxd_out.upload(d.xd_out, dxd_out.n);
        launch_rmsnorm_quant_wg(0, a, K, dxq_out.p, dxd_out.p, nt);
        break;
    case LIN_GEMV_NORM: case LIN_GEMV_NORM_ARGMAX: {
        ArgmaxEpi am{};
        if (p.form == LIN_GEMV_NORM_ARGMAX) {
            dkeys.alloc((size_t)d.n_keys); dkeys.upload((const q3_u64*)d.keys, dkeys.n);
            if (d.mask_per_tok) { dmask.alloc(nt); dmask.upload(d.mask_per_tok, nt); }
            am.keys = dkeys.p; am.key_stride = d.key_stride; am.mask_per_tok = dmask.p; am.idx_add = d.idx_add;
            run_gemv_q8_norm(0, p, m, d.row0, d.nrows_valid, a, nullptr, 0, nt, &am);
        } else run_gemv_q8_norm(0, p, m, d.row0, d.nrows, a, out, d.out_stride, nt, nullptr);
        break;
    }
    case LIN_GU_SWIGLU_NORM: run_gateup_swiglu(0, p, m, ff, a, aqp, adp, nt); break;
    case LIN_F_GEMV: case LIN_F_MFMA16: case LIN_F_MFMA:
        run_gemv_float(0, p, fm, d.row0, d.nrows, dx.p + d.x_off, d.x_stride, out, d.out_stride, nt);
        break;
    case LIN_F_GU_MFMA16:
        dgu.alloc((size_t)nt * ff);
        run_gateup_float(0, p, fm, ff, dx.p + d.x_off, d.x_stride, dgu.p, nt);
        break;
    case LIN_F_GU_UNFUSED: { // the float matmul the engine would run + k_swiglu_f32
        dgu.alloc((size_t)nt * 2 * ff);
        LinearPlanIn gi = lin_plan_in(d); gi.op = LOP_F_GEMV;
        const LinearPlan gp = plan_linear(gi);
        run_gemv_float(0, gp, fm, 0, 2 * ff, dx.p + d.x_off, d.x_stride, dgu.p, 2 * ff, nt);
        DevBuf<float> act((size_t)nt * ff);
        launch_swiglu_f32(0, dgu.p, ff, act.p, nt);
        Q3_HIP(hipMemcpy2D(out, (size_t)d.out_stride * 4, act.p, (size_t)ff * 4, (size_t)ff * 4, nt, hipMemcpyDeviceToDevice));
        Q3_HIP(hipDeviceSynchronize());
        p.lpr = gp.lpr; p.mt = gp.mt; p.z = gp.z;
        break;
    }
    default: throw Error("unhandled linear form");
    }
    Q3_LAUNCH_CHECK();
    if (p.form == LIN_F_GU_MFMA16) Q3_HIP(hipMemcpy2D(out, (size_t)d.out_stride * 4, dgu.p, (size_t)ff * 4, (size_t)ff * 4, nt, hipMemcpyDeviceToDevice));
    Q3_HIP(hipDeviceSynchronize());
    if (d.out) dout.download(d.out, dout.n);
    if (d.aq) {
        std::vector<int8_t> hq(daq.n); std::vector<uint16_t> hd(dad.n);
        daq.download(hq.data(), hq.size()); dad.download(hd.data(), hd.size());
        for (size_t i = 0; i < LIN_GUARD; i++)
            Q3_CHECK(hq[i] == 0x5A && hq[LIN_GUARD + n_aq + i] == 0x5A && hd[i] == 0x5A5A && hd[LIN_GUARD + n_ad + i] == 0x5A5A, "gate/up form wrote outside aq / ad");
        std::memcpy(d.aq, hq.data() + LIN_GUARD, n_aq); std::memcpy(d.ad, hd.data() + LIN_GUARD, n_ad * 2);
    }
    if (d.h_out) dhout.download(d.h_out, dhout.n);
    if (d.xn_out) dxn.download(d.xn_out, dxn.n);
    if (dxq_out.p) { dxq_out.download(d.xq_out, dxq_out.n); dxd_out.download(d.xd_out, dxd_out.n); }
    if (dkeys.p) dkeys.download((q3_u64*)d.keys, dkeys.n);
    d.form_ran = p.form; d.lpr_ran = p.lpr; d.mt_ran = p.mt; d.z_ran = p.z;
}

// q3tts_op_frame_glue: one guarded in/out buffer.  It goes up whole, the kernel works Q3TTS_GLUE_GUARD elements in, and it comes back whole
// after the launch ran.
template <class T> struct GlueBuf {
    DevBuf<T> d; T* host = nullptr; size_t n = 0;
    // core = the elements the kernel may touch at the least; 0 = the kernel does not use this buffer
    void up(const q3tts_guarded& g, size_t core, const char* what) {
        Q3_CHECK(g.p && g.n >= (int64_t)(core + 2 * Q3TTS_GLUE_GUARD), std::string("guarded buffer too small or missing: ") + what);
        host = (T*)g.p; n = (size_t)g.n;
        d.alloc(n); d.upload(host, n);
    }
    T* p() const { return d.p + Q3TTS_GLUE_GUARD; }
    void down() { if (host) d.download(host, n); }
};

// ---- [EXT] what q3tts_op_pcm_convert, q3tts_op_tsm and q3tts_op_pitch share: every stream's guarded output (and trace) buffer goes whole into
// its region of one device buffer -- regions start on 256 bytes (64 trace entries) -- the chunks are walked with each stream's output
// appended behind its earlier chunks', and everything comes back whole ----
template <class T> struct GuardedStoreOf {   // a whole guarded state store: GLUE_GUARD elements, the store, GLUE_GUARD elements
    T* host; size_t n; DevBuf<T> dev;
    GuardedStoreOf(T* h, size_t core_elems) : host(h), n(core_elems + 2 * Q3TTS_GLUE_GUARD), dev(n) { dev.upload(host, n); }
    T* core() const { return dev.p + Q3TTS_GLUE_GUARD; }
    void download() { dev.download(host, n); }
};
typedef GuardedStoreOf<float> GuardedStore;
struct GuardedRun {
    const int G, n_chunks; const bool flush;
    const int32_t* const chunk_samples; const int32_t* const streams; const int32_t* const reset_before;
    void* const* const out; const int64_t* const out_bytes; int32_t* const* const trace; const int64_t* const trace_len;
    const std::vector<int64_t>& esz;                  // bytes of one output sample of stream g
    std::vector<int64_t> reg, treg, bytes, fr;        // region starts; output bytes and trace entries made so far
    std::vector<int64_t> off, toff;                   // the current chunk's first output byte and trace entry
    DevBuf<uint8_t> d_out; DevBuf<int32_t> d_trace; DevBuf<float> d_in;
    int c = -1, T = 0; const float* x = nullptr; const int32_t* sl = nullptr;   // the current chunk, its samples per stream, its input and slots
    // need[g] = the output bytes the plan gives stream g, frames[g] its trace entries (trace NULL: the call has no traces)
    GuardedRun(const float* in, int G_, const int32_t* chunk_samples_, int n_chunks_, bool flush_, const int32_t* streams_, const int32_t* reset_before_,
               const std::vector<int64_t>& esz_, const std::vector<int64_t>& need, const std::vector<int64_t>* frames, void* const* out_,
               const int64_t* out_bytes_, int32_t* const* trace_, const int64_t* trace_len_)
        : G(G_), n_chunks(n_chunks_), flush(flush_), chunk_samples(chunk_samples_), streams(streams_), reset_before(reset_before_), out(out_),
          out_bytes(out_bytes_), trace(trace_), trace_len(trace_len_), esz(esz_), reg(G_), treg(G_), bytes(G_, 0), fr(G_, 0), off(G_), toff(G_) {
        int64_t total = 0, ttotal = 0, in_floats = 0;
        for (int g = 0; g < G; g++) {
            Q3_CHECK(out[g] && out_bytes[g] >= need[g] + 2 * Q3TTS_GLUE_GUARD * esz[g], "guarded output buffer too small or missing");
            reg[g] = total; total += (out_bytes[g] + 255) / 256 * 256;
            if (!trace) continue;
            Q3_CHECK(trace[g] && trace_len[g] >= (*frames)[g] + 2 * Q3TTS_GLUE_GUARD, "guarded trace buffer too small or missing");
            treg[g] = ttotal; ttotal += (trace_len[g] + 63) / 64 * 64;
        }
        d_out.alloc((size_t)total); d_trace.alloc((size_t)ttotal);
        for (int g = 0; g < G; g++) {
            Q3_HIP(hipMemcpy(d_out.p + reg[g], out[g], (size_t)out_bytes[g], hipMemcpyHostToDevice));
            if (trace) Q3_HIP(hipMemcpy(d_trace.p + treg[g], trace[g], (size_t)trace_len[g] * 4, hipMemcpyHostToDevice));
        }
        for (int i = 0; i < n_chunks; i++) in_floats += (int64_t)G * chunk_samples[i];
        d_in.alloc((size_t)std::max<int64_t>(in_floats, 1)); d_in.upload(in, (size_t)in_floats);
        x = d_in.p;
    }
    bool next() {   // the next chunk, or the flush behind the last one, which follows the last chunk's slots
        if (c >= 0) x += (size_t)G * T;
        if (++c > n_chunks || (c == n_chunks && !flush)) return false;
        T = c < n_chunks ? chunk_samples[c] : 0;
        sl = streams + (size_t)std::min(c, n_chunks - 1) * G;
        for (int g = 0; g < G; g++) { off[g] = reg[g] + Q3TTS_GLUE_GUARD * esz[g] + bytes[g]; toff[g] = treg[g] + Q3TTS_GLUE_GUARD + fr[g]; }
        return true;
    }
    bool flushing() const { return c == n_chunks; }
    bool reset(int g) const { return c < n_chunks && reset_before && reset_before[(size_t)c * G + g]; }
    void copy_native(int g) {   // a stream no stage touches is copied through as f32
        if (T > 0) Q3_HIP(hipMemcpyAsync(d_out.p + off[g], x + (size_t)g * T, (size_t)T * 4, hipMemcpyDeviceToDevice, 0));
        bytes[g] += (int64_t)T * 4;
    }
    void finish(int64_t* n_out, const std::vector<int64_t>* need, const char* differ) {   // need: the plan the launchers' counts must have met
        Q3_LAUNCH_CHECK();
        Q3_HIP(hipDeviceSynchronize());
        for (int g = 0; g < G; g++) {
            if (need) Q3_CHECK(bytes[g] == (*need)[g], differ);
            Q3_HIP(hipMemcpy(out[g], d_out.p + reg[g], (size_t)out_bytes[g], hipMemcpyDeviceToHost));
            if (trace) Q3_HIP(hipMemcpy(trace[g], d_trace.p + treg[g], (size_t)trace_len[g] * 4, hipMemcpyDeviceToHost));
            n_out[g] = bytes[g] / esz[g];
        }
    }
};
// every count of q3tts_op_tsm / q3tts_op_pitch worked out as the launchers will (pitch_pct NULL: no stream has a pitch): frames[g] = the
// stage-1 frames stream g makes, need[g] = its output bytes, esz[g] = the bytes of one of its samples.  A position whose slot is reset starts over
static void prosody_op_plan(int G, const int32_t* chunk_samples, int n_chunks, bool flush, const int32_t* streams, int n_streams, const int32_t* reset_before,
                            const int32_t* rate_pct, const int32_t* pitch_pct, const int32_t* encoding, std::vector<int64_t>& frames,
                            std::vector<int64_t>& need, std::vector<int64_t>& esz) {
    std::vector<int64_t> seen((size_t)n_streams, 0), done((size_t)n_streams, 0);
    frames.assign(G, 0); need.assign(G, 0); esz.assign(G, 4);
    for (int c = 0; c <= n_chunks; c++) {
        if (c == n_chunks && !flush) break;
        const int32_t* sl = streams + (size_t)std::min(c, n_chunks - 1) * G;   // the flush follows the last chunk's slots
        const int64_t T = c < n_chunks ? chunk_samples[c] : 0;
        for (int g = 0; g < G; g++) {
            int64_t& sn = seen[(size_t)sl[g]]; int64_t& dn = done[(size_t)sl[g]];
            const int P = pitch_pct ? pitch_pct[g] : 100;
            if (c < n_chunks && reset_before && reset_before[(size_t)c * G + g]) sn = dn = 0;
            if (P == 100 && rate_pct[g] == 100) { need[g] += T; continue; }
            const int64_t total = std::max<int64_t>(P != 100 ? pitch_frames(rate_pct[g], P, sn + T, c == n_chunks) : tsm_frames(rate_pct[g], sn + T, c == n_chunks), dn);
            if (P != 100) {
                PitchPlan p;
                pitch_plan(P, &p);
                need[g] += pitch_samples_of_z(p, total * Q3_TSM_HOP) - pitch_samples_of_z(p, dn * Q3_TSM_HOP);
            } else need[g] += (total - dn) * Q3_TSM_HOP;
            frames[g] += total - dn; sn += T; dn = total;
        }
    }
    for (int g = 0; g < G; g++) {
        esz[g] = ((pitch_pct && pitch_pct[g] != 100) || rate_pct[g] != 100) && encoding[g] == Q3_PCM_S16 ? 2 : 4;   // a native stream is copied through as f32
        need[g] *= esz[g];
    }
}

extern "C" {

int q3tts_op_attention(q3tts_attention_desc* d) {
    Q3_API_BEGIN
    require_gpu();
    attention_op_run(d);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_attention_keyed(q3tts_attention_desc* d, const uint64_t* keys, int32_t key_stride, int32_t qkv_rows) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(keys, "null keys");
    attention_op_run(d, keys, key_stride, qkv_rows);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_attention_plan(q3tts_attention_desc* d) {
    Q3_API_BEGIN
    Q3_CHECK(d && d->ntok >= 1 && d->n_kv >= 1 && d->n_head >= 1, "bad attention shape");
    d->form_ran = attention_op_plan(*d);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_linear(q3tts_linear_desc* d) {
    Q3_API_BEGIN
    require_gpu();
    lin_run(d);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_linear_plan(q3tts_linear_desc* d) {
    Q3_API_BEGIN
    Q3_CHECK(d, "null linear descriptor");
    const LinearPlan p = lin_plan(*d);
    d->form_ran = p.form; d->lpr_ran = p.lpr; d->mt_ran = p.mt; d->z_ran = p.z;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

uint64_t q3tts_argmax_key(float v, int32_t idx) { return pack_key(v, idx); }

/* [EXT] candidate sets: k_kv_fork over host images of both cache planes; every precondition is checked before anything is uploaded or launched */
int q3tts_op_kv_fork(uint16_t* k_cache, uint16_t* v_cache, int32_t n_pages, int32_t n_layer, int32_t n_kv, const int32_t* page_table,
                     int32_t n_seq, int32_t max_pages, int32_t src_seq, const int32_t* dst_seqs, int32_t n_dst, int32_t n_positions) {
    Q3_API_BEGIN
    Q3_CHECK(k_cache && v_cache && page_table && dst_seqs, "null argument");
    Q3_CHECK(n_pages >= 1 && n_layer >= 1 && n_kv >= 1 && n_seq >= 1 && max_pages >= 1, "bad cache / page table shape");
    Q3_CHECK((int64_t)n_layer * n_kv <= 65536 && (int64_t)n_pages * n_layer * n_kv <= ((int64_t)1 << 24), "cache too large for the test surface");
    Q3_CHECK(n_dst >= 1, "n_dst must be >= 1");
    Q3_CHECK(n_positions >= 1 && (int64_t)n_positions <= (int64_t)max_pages * 64, "n_positions must be in [1, max_pages * 64]");
    Q3_CHECK(src_seq >= 0 && src_seq < n_seq, "source sequence out of range");
    const int np = (n_positions + 63) / 64;
    std::vector<int> owner((size_t)n_pages, -1); // physical page -> the sequence that brought it in
    std::vector<char> listed((size_t)n_seq, 0);
    listed[src_seq] = 1;
    for (int d = -1; d < n_dst; d++) {
        const int seq = d < 0 ? src_seq : dst_seqs[d];
        if (d >= 0) {
            Q3_CHECK(seq >= 0 && seq < n_seq, "destination sequence out of range");
            Q3_CHECK(seq != src_seq, "a destination equals the source");
            Q3_CHECK(!listed[seq], "a destination is listed twice");
            listed[seq] = 1;
        }
        for (int l = 0; l < np; l++) {
            const int pg = page_table[(size_t)seq * max_pages + l];
            Q3_CHECK(pg >= 0 && pg < n_pages, "page table entry out of range");
            Q3_CHECK(owner[pg] < 0, "two of the physical pages involved coincide");
            owner[pg] = seq;
        }
    }
    require_gpu();
    const size_t halfs = (size_t)n_pages * n_layer * n_kv * 8192;
    DevBuf<uint16_t> dk(halfs), dv(halfs);
    dk.upload(k_cache, halfs); dv.upload(v_cache, halfs);
    DevBuf<int32_t> dpt((size_t)n_seq * max_pages), dd((size_t)n_dst);
    dpt.upload(page_table, dpt.n); dd.upload(dst_seqs, dd.n);
    KvCache kv; kv.k = dk.p; kv.v = dv.p; kv.page_table = dpt.p; kv.max_pages = max_pages; kv.n_layer = n_layer; kv.n_kv = n_kv;
    launch_kv_fork(0, kv, src_seq, dd.p, n_dst, np);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    dk.download(k_cache, halfs); dv.download(v_cache, halfs);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] prompt stems: k_kv_stem over host images of both cache planes and of a store arena; every precondition is checked before anything is uploaded or launched */
int q3tts_op_kv_stem(uint16_t* k_cache, uint16_t* v_cache, int32_t n_pages, int32_t n_layer, int32_t n_kv, const int32_t* page_table,
                     int32_t n_seq, int32_t max_pages, uint16_t* store_k, uint16_t* store_v, int32_t n_store_pages, int32_t n_jobs,
                     const int32_t* job_page0, const int32_t* job_n_pages, const int32_t* job_first, const int32_t* job_n_dst,
                     const int32_t* slots, int32_t n_slots, int32_t save) {
    Q3_API_BEGIN
    Q3_CHECK(n_jobs >= 1 && n_jobs <= 4096, "n_jobs must be in [1, 4096]");
    Q3_CHECK(k_cache && v_cache && page_table && store_k && store_v && job_page0 && job_n_pages && job_first && job_n_dst && slots, "null argument");
    Q3_CHECK(n_pages >= 1 && n_layer >= 1 && n_kv >= 1 && n_seq >= 1 && max_pages >= 1 && n_store_pages >= 1 && n_slots >= 1, "bad cache / page table / store shape");
    Q3_CHECK((int64_t)n_layer * n_kv <= 65536 && (int64_t)(n_pages + n_store_pages) * n_layer * n_kv <= ((int64_t)1 << 24), "cache too large for the test surface");
    std::vector<char> pool_hit((size_t)n_pages, 0), store_hit((size_t)n_store_pages, 0);
    int most = 0;
    for (int j = 0; j < n_jobs; j++) {
        const int np = job_n_pages[j];
        Q3_CHECK(np >= 1 && np <= max_pages, "a job's n_pages must be in [1, max_pages]");
        Q3_CHECK(job_page0[j] >= 0 && (int64_t)job_page0[j] + np <= n_store_pages, "a job's store range lies outside the arena");
        Q3_CHECK(job_n_dst[j] >= 1 && (!save || job_n_dst[j] == 1), "a job's n_dst must be >= 1 (save: exactly 1)");
        Q3_CHECK(job_first[j] >= 0 && (int64_t)job_first[j] + job_n_dst[j] <= n_slots, "a job's slot range lies outside slots");
        most = std::max(most, np);
        for (int l = 0; l < np; l++) {
            if (save) { Q3_CHECK(!store_hit[job_page0[j] + l], "two jobs' store ranges overlap"); store_hit[job_page0[j] + l] = 1; }
            for (int d = 0; d < job_n_dst[j]; d++) {
                const int seq = slots[job_first[j] + d];
                Q3_CHECK(seq >= 0 && seq < n_seq, "slot out of range");
                const int pg = page_table[(size_t)seq * max_pages + l];
                Q3_CHECK(pg >= 0 && pg < n_pages, "page table entry out of range");
                if (!save) { Q3_CHECK(!pool_hit[pg], "two destination pages coincide"); pool_hit[pg] = 1; }
            }
        }
    }
    require_gpu();
    const size_t per = (size_t)n_layer * n_kv * 8192, halfs = (size_t)n_pages * per, shalfs = (size_t)n_store_pages * per;
    DevBuf<uint16_t> dk(halfs), dv(halfs), sk(shalfs), sv(shalfs);
    dk.upload(k_cache, halfs); dv.upload(v_cache, halfs); sk.upload(store_k, shalfs); sv.upload(store_v, shalfs);
    DevBuf<int32_t> dpt((size_t)n_seq * max_pages), ds((size_t)n_slots);
    dpt.upload(page_table, dpt.n); ds.upload(slots, ds.n);
    std::vector<StemJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; j++) jobs[j] = StemJob{sk.p + (size_t)job_page0[j] * per, sv.p + (size_t)job_page0[j] * per, job_n_pages[j], job_first[j], job_n_dst[j], 0};
    DevBuf<StemJob> dj((size_t)n_jobs);
    dj.upload(jobs.data(), jobs.size());
    KvCache kv; kv.k = dk.p; kv.v = dv.p; kv.page_table = dpt.p; kv.max_pages = max_pages; kv.n_layer = n_layer; kv.n_kv = n_kv;
    launch_kv_stem(0, kv, dj.p, n_jobs, most, ds.p, save != 0);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    dk.download(k_cache, halfs); dv.download(v_cache, halfs); sk.download(store_k, shalfs); sv.download(store_v, shalfs);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_gemv_q8(const void* w, int32_t n, int32_t k, const int8_t* xq, const uint16_t* xd, int32_t ntok, float* y, int32_t lpr) {
    Q3_API_BEGIN
    require_gpu();
    DevBuf<uint8_t> storage;
    Q8Mat m = q8mat_from_host(w, n, k, storage);
    DevBuf<int8_t> dxq((size_t)ntok * k); dxq.upload(xq, dxq.n);
    DevBuf<uint16_t> dxd((size_t)ntok * (k / 32)); dxd.upload(xd, dxd.n);
    const int nsseg = ((k >> 8) + 7) / 8;
    DevBuf<float> parts((size_t)nsseg * ntok * n);
    launch_gemv_q8(0, m, 0, n, dxq.p, dxd.p, parts.p, n, ntok, lpr);
    Q3_HIP(hipDeviceSynchronize());
    std::vector<float> hp(parts.n);
    parts.download(hp.data(), hp.size());
    for (int t = 0; t < ntok; t++)
        for (int r = 0; r < n; r++) { // spec S3: super-segment sums added in order
            float v = hp[((size_t)0 * ntok + t) * n + r];
            for (int s = 1; s < nsseg; s++) v = v + hp[((size_t)s * ntok + t) * n + r];
            y[(size_t)t * n + r] = v;
        }
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* fused gate/up GEMM + SwiGLU + int8 quantisation of the batched (>= 16 token) layer path; w = [2*ff][k] Q8_0 rows, gate rows first */
int q3tts_op_gateup_q8(const void* w, int32_t ff, int32_t k, const int8_t* xq, const uint16_t* xd, int32_t ntok, int8_t* aq, uint16_t* ad) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(w && xq && xd && aq && ad && ff > 0 && ff % 32 == 0 && k % 256 == 0 && ntok >= 1, "bad gate/up shape");
    DevBuf<uint8_t> storage;
    Q8Mat m = q8mat_from_host(w, 2 * ff, k, storage);
    DevBuf<int8_t> dxq((size_t)ntok * k); dxq.upload(xq, dxq.n);
    DevBuf<uint16_t> dxd((size_t)ntok * (k / 32)); dxd.upload(xd, dxd.n);
    DevBuf<int8_t> daq((size_t)ntok * ff); DevBuf<uint16_t> dad((size_t)ntok * (ff / 32));
    if (!launch_gateup_mfma(0, m, ff, dxq.p, dxd.p, daq.p, dad.p, ntok)) throw Error("shape not served by the fused gate/up matrix-core kernel");
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    daq.download(aq, daq.n); dad.download(ad, dad.n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_gemv_kq(const void* const* raws, const int32_t* types, const int32_t* rows, int32_t nparts, int32_t k, const int8_t* xq, const uint16_t* xd,
                     int32_t ntok, float* y, int32_t lpr) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(raws && types && rows && nparts >= 1 && nparts <= 3 && xq && xd && y && ntok >= 1 && k % 256 == 0, "bad K-quant gemv arguments");
    DevBuf<uint8_t> storage;
    Q8Mat m = kqmat_from_host(raws, types, rows, nparts, k, storage);
    const int n = m.N;
    DevBuf<int8_t> dxq((size_t)ntok * k); dxq.upload(xq, dxq.n);
    DevBuf<uint16_t> dxd((size_t)ntok * (k / 32)); dxd.upload(xd, dxd.n);
    const int nsseg = ((k >> 8) + 7) / 8;
    DevBuf<float> parts_out((size_t)nsseg * ntok * n);
    launch_gemv_q8(0, m, 0, n, dxq.p, dxd.p, parts_out.p, n, ntok, lpr);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    std::vector<float> hp(parts_out.n);
    parts_out.download(hp.data(), hp.size());
    for (int t = 0; t < ntok; t++)
        for (int r = 0; r < n; r++) { // spec S3: super-segment sums added in order
            float v = hp[((size_t)0 * ntok + t) * n + r];
            for (int s2 = 1; s2 < nsseg; s2++) v = v + hp[((size_t)s2 * ntok + t) * n + r];
            y[(size_t)t * n + r] = v;
        }
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_op_gateup_kq(const void* gate_raw, const void* up_raw, int32_t type, int32_t ff, int32_t k, const int8_t* xq, const uint16_t* xd, int32_t ntok,
                       int8_t* aq, uint16_t* ad) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(gate_raw && up_raw && xq && xd && aq && ad && ff > 0 && ff % 32 == 0 && k % 256 == 0 && ntok >= 1, "bad gate/up shape");
    const void* raws[2] = {gate_raw, up_raw}; const int32_t types[2] = {type, type}, rows[2] = {ff, ff};
    DevBuf<uint8_t> storage;
    Q8Mat m = kqmat_from_host(raws, types, rows, 2, k, storage);
    DevBuf<int8_t> dxq((size_t)ntok * k); dxq.upload(xq, dxq.n);
    DevBuf<uint16_t> dxd((size_t)ntok * (k / 32)); dxd.upload(xd, dxd.n);
    DevBuf<int8_t> daq((size_t)ntok * ff); DevBuf<uint16_t> dad((size_t)ntok * (ff / 32));
    if (!launch_gateup_mfma(0, m, ff, dxq.p, dxd.p, daq.p, dad.p, ntok)) throw Error("shape not served by the fused gate/up matrix-core kernel");
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    daq.download(aq, daq.n); dad.download(ad, dad.n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_matmul_float(const void* w, int32_t type, int32_t n, int32_t k, int32_t row0, int32_t nrows, const float* x, int32_t ntok, float* y) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(type == Q3_T_F32 || type == Q3_T_F16 || type == Q3_T_BF16, "float type expected");
    Q3_CHECK(n > 0 && k > 0 && k % 256 == 0 && ntok > 0 && row0 >= 0 && nrows > 0 && row0 + nrows <= n, "bad matmul shape");
    const size_t esz = type == Q3_T_F32 ? 4 : 2;
    DevBuf<uint8_t> dw((size_t)n * k * esz); dw.upload((const uint8_t*)w, dw.n);
    DevBuf<uint8_t> dwt((size_t)((n + 63) / 64) * 64 * k * esz);
    launch_tile_float(0, dw.p, dwt.p, type, n, k);
    FMat m; m.w = dw.p; m.wt = dwt.p; m.type = type; m.N = n; m.K = k;
    DevBuf<float> dx((size_t)ntok * k); dx.upload(x, dx.n);
    DevBuf<float> dy((size_t)ntok * nrows);
    launch_gemv_float(0, m, row0, nrows, dx.p, k, dy.p, nrows, ntok);
    Q3_HIP(hipDeviceSynchronize());
    dy.download(y, dy.n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_rmsnorm_quant(const float* x, const float* g, int32_t d, int32_t ntok, float eps, int8_t* xq, uint16_t* xd, float* xn) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(d % 256 == 0 && d <= 2048, "d must be a multiple of 256 and <= 2048");
    DevBuf<float> dx((size_t)ntok * d), dg(d), dxn((size_t)ntok * d);
    dx.upload(x, dx.n); dg.upload(g, d);
    DevBuf<int8_t> dq((size_t)ntok * d); DevBuf<uint16_t> dd((size_t)ntok * d / 32);
    NormArgs a{};
    a.h_in = dx.p; a.h_stride = d; a.g = dg.p; a.eps = eps; a.d = d; a.xq = dq.p; a.xd = dd.p; a.xn_out = dxn.p;
    launch_rmsnorm_quant(0, a, ntok);
    Q3_HIP(hipDeviceSynchronize());
    if (xq) dq.download(xq, dq.n);
    if (xd) dd.download(xd, dd.n);
    if (xn) dxn.download(xn, dxn.n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_swiglu_quant(const float* gu, int32_t ff, int32_t ntok, int8_t* aq, uint16_t* ad) {
    Q3_API_BEGIN
    require_gpu();
    DevBuf<float> dgu((size_t)ntok * 2 * ff); dgu.upload(gu, dgu.n);
    DevBuf<int8_t> dq((size_t)ntok * ff); DevBuf<uint16_t> dd((size_t)ntok * ff / 32);
    launch_swiglu_quant(0, dgu.p, ff, dq.p, dd.p, ntok);
    Q3_HIP(hipDeviceSynchronize());
    dq.download(aq, dq.n); dd.download(ad, dd.n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_argmax(const float* logits, int32_t n, int32_t start, int32_t end, int32_t mask_idx, int32_t* out) {
    Q3_API_BEGIN
    require_gpu();
    DevBuf<float> dl(n); dl.upload(logits, n);
    DevBuf<int32_t> dm(1), dout(1);
    dm.upload(&mask_idx, 1);
    launch_argmax(0, dl.p, n, start, end, dm.p, dout.p, 1, 0, 1);
    Q3_HIP(hipDeviceSynchronize());
    dout.download(out, 1);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* n_draws consecutive samples of one sequence from the SAME logits (the RNG stream advances between draws) */
int q3tts_op_sample(const float* logits, int32_t n, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t mask_idx,
                    int32_t n_draws, int32_t* out) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(logits && out && n >= 1 && n_draws >= 1, "bad arguments");
    StdRng rng(seed);
    DevBuf<float> dl(n), dt(1), dp(1); DevBuf<int32_t> dk(1), dm(1); DevBuf<uint32_t> dkey(8), ddraw(1); DevBuf<q3_u64> dout(n_draws);
    const uint32_t zero = 0;
    dl.upload(logits, n); dt.upload(&temperature, 1); dp.upload(&top_p, 1); dk.upload(&top_k, 1); dm.upload(&mask_idx, 1);
    dkey.upload(rng.key(), 8); ddraw.upload(&zero, 1);
    for (int i = 0; i < n_draws; i++) {
        SampleArgs a{dl.p, n, n, dt.p, dk.p, dp.p, dm.p, dkey.p, ddraw.p, dout.p + i, 1};
        launch_sample(0, a, 1);
    }
    Q3_HIP(hipDeviceSynchronize());
    std::vector<q3_u64> keys(n_draws);
    dout.download(keys.data(), n_draws);
    for (int i = 0; i < n_draws; i++) out[i] = (int32_t)(~(uint32_t)(keys[i] & 0xFFFFFFFFull));
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_sample_rows(int32_t kernel, const float* logits, int32_t B, int32_t n, const float* temperature, const int32_t* top_k,
                         const float* top_p, const float* penalty, const uint64_t* seed, const int32_t* hist, const int32_t* hist_len,
                         int32_t hist_cap, int32_t n_draws, int32_t* out) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(logits && temperature && top_k && top_p && seed && out && B >= 1 && n >= 1 && n_draws >= 1, "bad arguments");
    Q3_CHECK(kernel == 0 || kernel == 1, "kernel must be 0 (k_sample) or 1 (k_sample_pred)");
    Q3_CHECK(kernel == 0 || !penalty, "the predictor sampler takes no penalty");
    Q3_CHECK(!penalty || (hist && hist_len && hist_cap >= 1), "a penalty needs a history");
    DevBuf<float> dl((size_t)B * n), dt(B), dp(B), dpen(B); DevBuf<int32_t> dk(B); DevBuf<uint32_t> dkey((size_t)8 * B), ddraw(B);
    DevBuf<q3_u64> dout((size_t)n_draws * B);
    dl.upload(logits, dl.n); dt.upload(temperature, B); dp.upload(top_p, B); dk.upload(top_k, B);
    std::vector<uint32_t> keys((size_t)8 * B), zero(B, 0u);
    for (int b = 0; b < B; b++) { StdRng rng(seed[b]); std::copy(rng.key(), rng.key() + 8, keys.begin() + (size_t)b * 8); }
    dkey.upload(keys.data(), keys.size()); ddraw.upload(zero.data(), B);
    // history in the frame graph's layout: code_0 of frame f at hist[b*stride + f*16], the current frame's code_0 as an argmax key
    DevBuf<int32_t> dh, dlen; DevBuf<q3_u64> dcur;
    if (penalty) {
        const int stride = hist_cap * 16;
        std::vector<int32_t> hh((size_t)B * stride, -1), len(B);
        std::vector<q3_u64> cur(B, 0ull); // key 0 = code -1: ignored
        for (int b = 0; b < B; b++) {
            Q3_CHECK(hist_len[b] >= 0 && hist_len[b] <= hist_cap, "hist_len out of range");
            const int nh = hist_len[b];
            for (int f = 0; f + 1 < nh; f++) hh[(size_t)b * stride + (size_t)f * 16] = hist[(size_t)b * hist_cap + f];
            len[b] = nh > 0 ? nh - 1 : 0;
            if (nh > 0) cur[b] = pack_key(0.0f, hist[(size_t)b * hist_cap + nh - 1]);
        }
        dh.alloc(hh.size()); dh.upload(hh.data(), hh.size()); dlen.alloc(B); dlen.upload(len.data(), B); dcur.alloc((size_t)16 * B);
        std::vector<q3_u64> cur16((size_t)16 * B, 0ull);
        for (int b = 0; b < B; b++) cur16[(size_t)b * 16] = cur[b];
        dcur.upload(cur16.data(), cur16.size());
        dpen.upload(penalty, B);
    }
    for (int i = 0; i < n_draws; i++) {
        SampleArgs a{dl.p, n, n, dt.p, dk.p, dp.p, nullptr, dkey.p, ddraw.p, dout.p + (size_t)i * B, 1};
        if (penalty) { a.penalty = dpen.p; a.hist = dh.p; a.hist_stride = hist_cap * 16; a.hist_len = dlen.p; a.cur_key = dcur.p; a.cur_stride = 16; }
        if (kernel == 0) launch_sample(0, a, B);
        else launch_sample_pred(0, a, B);
        Q3_LAUNCH_CHECK();
    }
    Q3_HIP(hipDeviceSynchronize());
    std::vector<q3_u64> res(dout.n);
    dout.download(res.data(), res.size());
    for (size_t i = 0; i < res.size(); i++) out[i] = key_code(res[i]);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] token log-probabilities: k_logprob_rows in its plain form over host rows.  The device outputs carry one guard element on either side. */
int q3tts_op_logprob_rows(const float* logits, int32_t B, int32_t n, int32_t stride, const int32_t* chosen, int32_t extra_idx, float* out_chosen,
                          float* out_extra) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(logits && chosen && out_chosen && B >= 1 && n >= 1 && n <= 4096 && stride >= n, "bad arguments");
    Q3_CHECK(extra_idx < n && (extra_idx < 0 || out_extra), "extra_idx must lie below n and needs out_extra");
    DevBuf<float> dl((size_t)B * stride), dout((size_t)2 * (B + 2)); DevBuf<int32_t> dc(B);
    dl.upload(logits, dl.n); dc.upload(chosen, B);
    const float guard = -777.0f;
    std::vector<float> h(dout.n, guard);
    dout.upload(h.data(), h.size());
    LogprobArgs a; // two columns per row: the chosen code's value and the extra index's, each in its own guarded array
    a.p.logits = dl.p; a.p.stride = stride; a.p.n = n; a.p.chosen = dc.p; a.p.extra_idx = extra_idx; a.p.col = 0; a.p.col_extra = B + 2; a.n_first = 1;
    a.out = dout.p + 1; a.out_stride = 1;
    launch_logprob_rows(0, a, B);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    dout.download(h.data(), h.size());
    Q3_CHECK(h[0] == guard && h[B + 1] == guard && h[B + 2] == guard && h[2 * B + 3] == guard, "k_logprob_rows wrote outside its rows");
    for (int b = 0; b < B; b++) Q3_CHECK(extra_idx >= 0 || h[B + 3 + b] == guard, "k_logprob_rows wrote an extra value nobody asked for");
    std::copy(h.begin() + 1, h.begin() + 1 + B, out_chosen);
    if (extra_idx >= 0) std::copy(h.begin() + B + 3, h.begin() + B + 3 + B, out_extra);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] scoring: k_score_rows and k_score_inputs over host buffers, one guard row on either side of the device output */
int q3tts_op_score_rows(const float* tlogits, int32_t t_stride, const float* plogits, const int32_t* codes, int32_t F, float* out) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(tlogits && plogits && codes && out && F >= 1 && F <= 4096 && t_stride >= Q3_SAMPLE_END, "bad arguments");
    DevBuf<float> dt((size_t)F * t_stride), dp((size_t)15 * F * Q3_CODEBOOK_SIZE), dout((size_t)(F + 2) * Q3_LOGPROB_COLS); DevBuf<int32_t> dc((size_t)F * 16);
    dt.upload(tlogits, dt.n); dp.upload(plogits, dp.n); dc.upload(codes, dc.n);
    const float guard = -777.0f;
    std::vector<float> h(dout.n, guard);
    dout.upload(h.data(), h.size());
    ScoreRowsArgs a;
    a.tlogits = dt.p; a.t_stride = t_stride; a.plogits = dp.p; a.p_head_stride = (size_t)F * Q3_CODEBOOK_SIZE; a.codes = dc.p;
    a.out = dout.p + Q3_LOGPROB_COLS;
    launch_score_rows(0, a, F);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    dout.download(h.data(), h.size());
    for (int i = 0; i < Q3_LOGPROB_COLS; i++)
        Q3_CHECK(h[i] == guard && h[(size_t)(F + 1) * Q3_LOGPROB_COLS + i] == guard, "k_score_rows wrote outside its rows");
    std::copy(h.begin() + Q3_LOGPROB_COLS, h.begin() + (size_t)(F + 1) * Q3_LOGPROB_COLS, out);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_op_score_inputs(const float* hidden_proj, const float* const* tabs, const int64_t* tab_rows, int32_t dP, const int32_t* codes, int32_t F,
                          float* out) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(hidden_proj && tabs && tab_rows && codes && out && F >= 1 && F <= 4096 && dP >= 4 && dP % 4 == 0, "bad arguments");
    std::vector<DevBuf<float>> tab(15);
    std::vector<const float*> ptrs(15);
    for (int q = 0; q < 15; q++) {
        Q3_CHECK(tabs[q] && tab_rows[q] >= 1, "table missing");
        tab[q].alloc((size_t)tab_rows[q] * dP); tab[q].upload(tabs[q], tab[q].n);
        ptrs[q] = tab[q].p;
    }
    DevBuf<const float*> d_ptrs(15); DevBuf<int64_t> d_rows(15); DevBuf<float> dh((size_t)F * dP), dout((size_t)(16 * F + 2) * dP); DevBuf<int32_t> dc((size_t)F * 16);
    d_ptrs.upload(ptrs.data(), 15); d_rows.upload(tab_rows, 15); dh.upload(hidden_proj, dh.n); dc.upload(codes, dc.n);
    const float guard = -12345.0f;
    std::vector<float> h(dout.n, guard);
    dout.upload(h.data(), h.size());
    launch_score_inputs(0, dh.p, d_ptrs.p, d_rows.p, dP, dc.p, F, dout.p + dP);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    dout.download(h.data(), h.size());
    for (int i = 0; i < dP; i++) Q3_CHECK(h[i] == guard && h[(size_t)(16 * F + 1) * dP + i] == guard, "k_score_inputs wrote outside its rows");
    std::copy(h.begin() + dP, h.begin() + (size_t)(16 * F + 1) * dP, out);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] the four token-selection kernels over guarded device buffers (include/q3tts.h).  Only what keeps the launch inside its buffers is
 * checked here; what a launcher refuses is left to that launcher, and nothing is written to the host outputs before the last launch ran. */
int q3tts_op_select_rows(q3tts_select_desc* dp) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(dp, "null select descriptor");
    const q3tts_select_desc& d = *dp;
    const bool sampler = d.kernel == Q3TTS_SEL_SAMPLE || d.kernel == Q3TTS_SEL_SAMPLE_PRED;
    Q3_CHECK(sampler || d.kernel == Q3TTS_SEL_ARGMAX || d.kernel == Q3TTS_SEL_ARGMAX_KEYS, "unknown selection kernel");
    Q3_CHECK(d.logits && d.tokens && d.out_raw && d.B >= 1 && d.B <= 65535 && d.n >= 1 && d.stride >= d.n && d.row_off >= 0, "bad row shape");
    Q3_CHECK(d.out_stride == 1 || d.out_stride == 16, "out_stride must be 1 or 16");
    const int B = d.B, n = d.n, nl = sampler ? d.n_draws : 1;
    if (sampler) Q3_CHECK(d.temperature && d.top_k && d.top_p && d.seed && d.draws_out && d.n_draws >= 1, "the samplers need temperature / top_k / top_p / seed / draws_out");
    if (d.kernel == Q3TTS_SEL_ARGMAX) Q3_CHECK(d.start >= 0 && d.start <= d.end && d.end <= n, "argmax window outside [0, n]");
    if (d.penalty) {
        Q3_CHECK(d.hist && d.hist_len && d.hist_cap >= 1, "a penalty needs a history");
        for (int b = 0; b < B; b++) Q3_CHECK(d.hist_len[b] >= 0 && d.hist_len[b] <= d.hist_cap, "hist_len out of range");
    }
    // logits: guard value everywhere, then the rows
    const float guard = 3e38f;
    std::vector<float> hl((size_t)d.row_off + (size_t)B * d.stride, guard);
    for (int b = 0; b < B; b++) std::copy(d.logits + (size_t)b * n, d.logits + (size_t)(b + 1) * n, hl.begin() + d.row_off + (size_t)b * d.stride);
    DevBuf<float> dl(hl.size()); dl.upload(hl.data(), hl.size());
    const float* rows = dl.p + d.row_off;
    DevBuf<int32_t> dm;
    if (d.mask_idx) { dm.alloc(B); dm.upload(d.mask_idx, B); }
    const size_t slots = (size_t)B * d.out_stride;
    std::vector<q3_u64> raw((size_t)nl * slots);
    if (d.kernel == Q3TTS_SEL_ARGMAX) {
        const int32_t s32 = (int32_t)(uint32_t)(Q3TTS_SELECT_SENTINEL & 0xFFFFFFFFull);
        std::vector<int32_t> ho(slots, s32);
        DevBuf<int32_t> dout(slots); dout.upload(ho.data(), slots);
        launch_argmax(0, rows, d.stride, d.start, d.end, dm.p, dout.p, d.out_stride, d.add, B);
        Q3_LAUNCH_CHECK();
        Q3_HIP(hipDeviceSynchronize());
        dout.download(ho.data(), slots);
        for (size_t i = 0; i < slots; i++) raw[i] = (q3_u64)(uint32_t)ho[i];
        std::copy(raw.begin(), raw.end(), (q3_u64*)d.out_raw);
        for (int b = 0; b < B; b++) d.tokens[b] = ho[(size_t)b * d.out_stride];
        return Q3TTS_OK;
    }
    std::fill(raw.begin(), raw.end(), (q3_u64)Q3TTS_SELECT_SENTINEL);
    DevBuf<q3_u64> dout(raw.size()); dout.upload(raw.data(), raw.size());
    if (d.kernel == Q3TTS_SEL_ARGMAX_KEYS) {
        launch_argmax_keys(0, rows, d.stride, n, dm.p, dout.p, d.out_stride, B);
        Q3_LAUNCH_CHECK();
        Q3_HIP(hipDeviceSynchronize());
        dout.download((q3_u64*)d.out_raw, raw.size());
        for (int b = 0; b < B; b++) d.tokens[b] = key_code(d.out_raw[(size_t)b * d.out_stride]);
        return Q3TTS_OK;
    }
    DevBuf<float> dt(B), dp_(B), dpen; DevBuf<int32_t> dk(B), dh, dlen; DevBuf<uint32_t> dkey((size_t)8 * B), ddraw(B); DevBuf<q3_u64> dcur;
    dt.upload(d.temperature, B); dp_.upload(d.top_p, B); dk.upload(d.top_k, B);
    std::vector<uint32_t> keys((size_t)8 * B), draw(B, 0u);
    for (int b = 0; b < B; b++) { StdRng rng(d.seed[b]); std::copy(rng.key(), rng.key() + 8, keys.begin() + (size_t)b * 8); if (d.draw0) draw[b] = d.draw0[b]; }
    dkey.upload(keys.data(), keys.size()); ddraw.upload(draw.data(), B);
    SampleArgs a{rows, d.stride, n, dt.p, dk.p, dp_.p, dm.p, dkey.p, ddraw.p, dout.p, d.out_stride};
    if (d.penalty) { // the frame graph's layout: code f of row b at hist[b*hist_stride + f*16]; the 15 ints between two codes hold a value in [0, n)
        const size_t hs = (size_t)d.hist_cap * 16;
        std::vector<int32_t> hh((size_t)B * hs, 0);
        for (int b = 0; b < B; b++) for (int f = 0; f < d.hist_cap; f++) hh[(size_t)b * hs + (size_t)f * 16] = d.hist[(size_t)b * d.hist_cap + f];
        dh.alloc(hh.size()); dh.upload(hh.data(), hh.size()); dlen.alloc(B); dlen.upload(d.hist_len, B); dpen.alloc(B); dpen.upload(d.penalty, B);
        a.penalty = dpen.p; a.hist = dh.p; a.hist_stride = (int)hs; a.hist_len = dlen.p;
        if (d.cur_code) {
            std::vector<q3_u64> cur((size_t)16 * B, pack_key(0.0f, 0));
            for (int b = 0; b < B; b++) cur[(size_t)b * 16] = pack_key(0.0f, d.cur_code[b]);
            dcur.alloc(cur.size()); dcur.upload(cur.data(), cur.size());
            a.cur_key = dcur.p; a.cur_stride = 16;
        }
    }
    for (int i = 0; i < nl; i++) {
        a.out_key = dout.p + (size_t)i * slots;
        if (d.kernel == Q3TTS_SEL_SAMPLE) launch_sample(0, a, B);
        else launch_sample_pred(0, a, B);
        Q3_LAUNCH_CHECK();
    }
    Q3_HIP(hipDeviceSynchronize());
    dout.download((q3_u64*)d.out_raw, raw.size());
    ddraw.download(d.draws_out, B);
    for (int i = 0; i < nl; i++) for (int b = 0; b < B; b++) d.tokens[(size_t)i * B + b] = key_code(d.out_raw[(size_t)i * slots + (size_t)b * d.out_stride]);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_codec_gemm(q3tts_codec_gemm_desc* d) {
    Q3_API_BEGIN
    require_gpu();
    codec_gemm_run(d);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_codec_gemm_plan(q3tts_codec_gemm_desc* d) {
    Q3_API_BEGIN
    codec_gemm_plan_only(d);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_codec_gemm_tap_reuse(const q3tts_codec_gemm_desc* d) {
    Q3_API_BEGIN
    return codec_gemm_tap_reuse(d);
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_codec_kernel(q3tts_codec_kernel_desc* d) {
    Q3_API_BEGIN
    require_gpu();
    codec_kernel_run(d);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_op_project(const float* x, const float* w, const float* b, int32_t n_in, int32_t n_out, float* y) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(x && w && b && y && n_in >= 1 && n_out >= 1, "bad arguments");
    const std::vector<float> wb = project_wblk(w, n_in, n_out);   // padded to whole blocks of 16; the launcher refuses what k_project_mt cannot run
    DevBuf<float> dx(n_in), dw(wb.size()), db(n_out), dy(n_out);
    dx.upload(x, n_in); dw.upload(wb.data(), wb.size()); db.upload(b, n_out);
    launch_project_blk(0, dx.p, n_in, dw.p, db.p, n_in, n_out, dy.p, n_out, 1);
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    dy.download(y, n_out);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] the frame-loop glue kernels over guarded device buffers (include/q3tts.h): one launch through the engine's launcher, no dispatch
 * here.  A guarded buffer goes up whole, the kernel works Q3TTS_GLUE_GUARD elements in, and it comes back whole after the launch ran. */
int q3tts_op_frame_glue(q3tts_frame_glue_desc* dp) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(dp, "null frame-glue descriptor");
    const q3tts_frame_glue_desc& d = *dp;
    Q3_CHECK(d.kernel >= Q3TTS_GLUE_PROJECT_MT && d.kernel <= Q3TTS_GLUE_ADVANCE_KEYS_GATED, "unknown frame-glue kernel");
    Q3_CHECK(d.ntok >= 1 && d.ntok <= 65535, "ntok out of [1, 65535]");
    const size_t n = (size_t)d.ntok;
    GlueBuf<float> out, hidden, save_hidden;
    GlueBuf<q3_u64> keys, next_key0;
    GlueBuf<int32_t> finished, n_frames, t_slot, t_pos, hist;
    GlueBuf<uint32_t> draws, pdraws, save_draws;
    if (d.kernel == Q3TTS_GLUE_PROJECT_MT || d.kernel == Q3TTS_GLUE_PROJECT_TABLE) {
        const bool mt = d.kernel == Q3TTS_GLUE_PROJECT_MT;
        Q3_CHECK(d.x && d.w && d.b && d.n_in >= 1 && d.n_out >= 1, "bad projection shape");
        DevBuf<float> dw, db(d.n_out), dx;
        db.upload(d.b, d.n_out);
        if (mt) {
            Q3_CHECK(d.x_off >= 0 && d.x_stride >= d.n_in && d.out_stride >= d.n_out, "bad projection strides");
            Q3_CHECK(d.x_floats >= (int64_t)(n - 1) * d.x_stride + d.n_in, "x does not hold ntok rows");
            out.up(d.out, n * d.out_stride, "out");
            const std::vector<float> wb = project_wblk(d.w, d.n_in, d.n_out);   // whole blocks of 16; the launcher refuses a partial one
            dw.alloc(wb.size()); dw.upload(wb.data(), wb.size());
            // 16 more rows of 3e38 behind the caller's: a fetch that runs past row ntok inside its tile of 16 stays inside the allocation
            std::vector<float> hx((size_t)d.x_off + d.x_floats + (size_t)16 * d.x_stride, 3e38f);
            std::copy(d.x, d.x + d.x_floats, hx.begin() + d.x_off);
            dx.alloc(hx.size()); dx.upload(hx.data(), hx.size());
            launch_project_blk(0, dx.p + d.x_off, d.x_stride, dw.p, db.p, d.n_in, d.n_out, out.p(), d.out_stride, d.ntok);
        } else {
            Q3_CHECK(d.x_floats >= (int64_t)n * d.n_in && d.n_in <= 4096, "the table does not hold ntok rows of n_in <= 4096 floats");
            out.up(d.out, n * d.n_out, "out");
            const std::vector<float> wt = project_wt(d.w, d.n_in, d.n_out);
            dw.alloc(wt.size()); dw.upload(wt.data(), wt.size());
            dx.alloc((size_t)d.x_floats); dx.upload(d.x, (size_t)d.x_floats);
            launch_project_table(0, dx.p, d.ntok, dw.p, db.p, d.n_in, d.n_out, out.p());
        }
        Q3_LAUNCH_CHECK();
        Q3_HIP(hipDeviceSynchronize());
        out.down();
        return Q3TTS_OK;
    }
    if (d.kernel == Q3TTS_GLUE_FEEDBACK_KEYS || d.kernel == Q3TTS_GLUE_GATHER_ROWS_KEYS) {
        const bool fb = d.kernel == Q3TTS_GLUE_FEEDBACK_KEYS;
        const int nt = fb ? 16 : 1, len = fb ? Q3_EMBD : d.row_len;
        Q3_CHECK(d.tables && d.table_rows && len >= 1 && d.key_stride >= nt, "bad tables / row length / key stride");
        std::vector<DevBuf<float>> tab(nt);
        std::vector<const float*> ptrs(nt);
        for (int q = 0; q < nt; q++) {   // a negative code reads row 0: every table has one
            Q3_CHECK(d.tables[q] && d.table_rows[q] >= 1, "table missing");
            std::vector<float> ht((size_t)(d.table_rows[q] + 2) * len, 3e38f);   // one row of 3e38 before and after the table
            std::copy(d.tables[q], d.tables[q] + (size_t)d.table_rows[q] * len, ht.begin() + len);
            tab[q].alloc(ht.size()); tab[q].upload(ht.data(), ht.size());
            ptrs[q] = tab[q].p + len;
        }
        keys.up(d.keys, n * d.key_stride, "keys");
        out.up(d.out, n * len, "out");
        if (!fb) {
            launch_gather_rows_keys(0, ptrs[0], d.table_rows[0], keys.p(), d.key_stride, len, out.p(), d.ntok);
        } else {
            Q3_CHECK(d.tts_pad, "tts_pad missing");
            DevBuf<const float*> d_ptrs(16); DevBuf<int64_t> d_rows(16); DevBuf<float> d_pad(Q3_EMBD), d_text; DevBuf<int32_t> d_ntrail, d_ids;
            d_ptrs.upload(ptrs.data(), 16); d_rows.upload(d.table_rows, 16); d_pad.upload(d.tts_pad, Q3_EMBD);
            if (d.trail) {
                Q3_CHECK(d.n_trail && d.trail_ids && d.ids_stride >= 1 && d.text_table && d.text_rows >= 1, "the trail form needs n_trail / trail_ids / text_table");
                n_frames.up(d.n_frames, n, "n_frames");
                for (size_t t = 0; t < n; t++)   // the kernel reads trail_ids[t][n_frames[t]] while n_frames[t] < n_trail[t]
                    Q3_CHECK(n_frames.host[Q3TTS_GLUE_GUARD + t] >= 0 && d.n_trail[t] <= d.ids_stride, "n_frames < 0 or n_trail > ids_stride");
                d_ntrail.alloc(n); d_ntrail.upload(d.n_trail, n);
                d_ids.alloc(n * d.ids_stride); d_ids.upload(d.trail_ids, d_ids.n);
                d_text.alloc((size_t)d.text_rows * Q3_EMBD); d_text.upload(d.text_table, d_text.n);
                TextTrail tt; tt.n_frames = n_frames.p(); tt.n_trail = d_ntrail.p; tt.ids = d_ids.p; tt.ids_stride = d.ids_stride; tt.table = d_text.p; tt.rows = d.text_rows;
                launch_feedback_keys(0, d_ptrs.p, d_rows.p, keys.p(), d.key_stride, d_pad.p, out.p(), d.ntok, &tt);
            } else {
                launch_feedback_keys(0, d_ptrs.p, d_rows.p, keys.p(), d.key_stride, d_pad.p, out.p(), d.ntok);
            }
        }
        Q3_LAUNCH_CHECK();
        Q3_HIP(hipDeviceSynchronize());
        out.down(); keys.down(); n_frames.down();
        return Q3TTS_OK;
    }
    // the slot state machine
    const bool gate = d.kernel != Q3TTS_GLUE_ADVANCE_KEYS;
    Q3_CHECK(d.max_frames && d.hist_stride >= 16, "max_frames / hist_stride missing");
    keys.up(d.keys, n * 16, "keys"); next_key0.up(d.next_key0, n, "next_key0");
    finished.up(d.finished, n, "finished"); n_frames.up(d.n_frames, n, "n_frames"); t_slot.up(d.t_slot, n, "t_slot");
    t_pos.up(d.t_pos, 4 * n, "t_pos"); hist.up(d.hist, n * d.hist_stride, "hist");
    for (size_t b = 0; b < n; b++)   // a live slot appends 16 codes at n_frames*16 < max_frames*16
        Q3_CHECK(n_frames.host[Q3TTS_GLUE_GUARD + b] >= 0 && d.max_frames[b] >= 0 && (int64_t)d.max_frames[b] * 16 <= d.hist_stride, "history row outside hist_stride");
    DevBuf<int32_t> d_max(n + 1), d_open, d_ntrail;   // read-only per-slot inputs: one zero entry past the last slot
    d_max.zero(); d_max.upload(d.max_frames, n);
    AdvanceKeysArgs a{d.ntok, finished.p(), n_frames.p(), d_max.p, keys.p(), next_key0.p(), hist.p(), d.hist_stride, t_slot.p(), t_pos.p()};
    if (!gate) {
        launch_advance_keys(0, a);
    } else {
        Q3_CHECK(d.open && d.n_trail, "the gated kernels need open / n_trail");
        hidden.up(d.hidden, n * Q3_EMBD, "hidden"); save_hidden.up(d.save_hidden, n * Q3_EMBD, "save_hidden");
        draws.up(d.draws, n, "draws"); pdraws.up(d.pdraws, n, "pdraws"); save_draws.up(d.save_draws, 2 * n, "save_draws");
        d_open.alloc(n + 1); d_open.zero(); d_open.upload(d.open, n); d_ntrail.alloc(n + 1); d_ntrail.zero(); d_ntrail.upload(d.n_trail, n);
        StallArgs s; s.open = d_open.p; s.n_trail = d_ntrail.p; s.hidden = hidden.p(); s.draws = draws.p(); s.pdraws = pdraws.p();
        s.save_hidden = save_hidden.p(); s.save_draws = save_draws.p();
        if (d.kernel == Q3TTS_GLUE_STALL_SAVE) launch_stall_save(0, a, s);
        else launch_advance_keys_gated(0, a, s);
    }
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    keys.down(); next_key0.down(); finished.down(); n_frames.down(); t_slot.down(); t_pos.down(); hist.down();
    hidden.down(); save_hidden.down(); draws.down(); pdraws.down(); save_draws.down();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] the ggml-mode kernels over host buffers (include/q3tts.h): every check first, then the uploads, one launcher of ggml_mode.h (LINEAR:
 * the two gg_linear chains), and every guarded buffer downloaded whole. */
int q3tts_op_ggml(q3tts_ggml_desc* dp) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(dp, "null ggml-mode descriptor");
    const q3tts_ggml_desc& d = *dp;
    Q3_CHECK(d.op >= Q3TTS_GG_LOAD_ROWS && d.op <= Q3TTS_GG_SWIGLU, "unknown ggml-mode op");
    const bool flat = d.op == Q3TTS_GG_ADD || d.op == Q3TTS_GG_SWIGLU;
    const bool mat = d.op == Q3TTS_GG_MATVEC || d.op == Q3TTS_GG_LINEAR, quant = d.op == Q3TTS_GG_QUANT || mat;
    const auto holds = [](const q3tts_guarded& g, size_t core) { return g.p && g.n >= (int64_t)(core + 2 * Q3TTS_GLUE_GUARD); };
    GlueBuf<float> out, dk;
    GlueBuf<int8_t> q8, qk;
    GlueBuf<uint16_t> d8;
    GlueBuf<int16_t> bs;
    DevBuf<float> dx, du;
    if (flat) {
        Q3_CHECK(d.n >= 0 && d.n <= ((int64_t)1 << 31), "n out of [0, 2^31]");
        if (d.n == 0) return Q3TTS_OK;
        const size_t n = (size_t)d.n;
        Q3_CHECK(d.x && d.x_floats >= d.n && holds(d.out, n), "x / out do not hold n elements");
        Q3_CHECK(d.op == Q3TTS_GG_ADD || d.u, "u missing");
        out.up(d.out, n, "out");
        dx.alloc(n); dx.upload(d.x, n);
        if (d.op == Q3TTS_GG_ADD) gg_add(0, out.p(), dx.p, n);
        else { du.alloc(n); du.upload(d.u, n); gg_swiglu(0, dx.p, du.p, out.p(), n); }
        Q3_LAUNCH_CHECK();
        Q3_HIP(hipDeviceSynchronize());
        out.down();
        return Q3TTS_OK;
    }
    Q3_CHECK(d.ntok >= 0 && d.ntok <= 65535 && d.k >= 1, "ntok out of [0, 65535] or k < 1");
    const size_t nt = (size_t)d.ntok, k = (size_t)d.k;
    GgMat w;
    if (mat) { // what gg_matvec refuses, refused here before anything moves
        w.type = d.type; w.n = d.rows; w.k = d.k;
        Q3_CHECK(w.type == Q3_T_Q8_0 || w.type == Q3_T_Q5_K || w.type == Q3_T_Q6_K, "ggml mode serves Q8_0 / Q5_K / Q6_K matrices");
        Q3_CHECK(d.rows >= 0 && d.row0 >= 0 && d.nrows >= 0 && (int64_t)d.row0 + d.nrows <= d.rows, "ggml-mode matvec row range");
        if (d.nrows == 0) return Q3TTS_OK;
    }
    if (nt == 0) return Q3TTS_OK;
    if (quant) {
        Q3_CHECK(d.k % 256 == 0, "k % 256 != 0");
        Q3_CHECK(holds(d.q8, nt * k) && holds(d.d8, nt * k / 32) && holds(d.qk, nt * k) && holds(d.dk, nt * k / 256) && holds(d.bs, nt * k / 16),
                 "a quantised array does not hold ntok rows");
    }
    if (d.op == Q3TTS_GG_LOAD_ROWS) {
        Q3_CHECK(d.x && d.x_rows >= 1 && d.x_stride >= d.k && d.x_floats >= (int64_t)(d.x_rows - 1) * d.x_stride + d.k, "x does not hold x_rows rows");
        Q3_CHECK(!(d.idx && d.idx_keys) && holds(d.out, nt * k), "both index forms given, or out too small");
        if (d.idx || d.idx_keys) {
            Q3_CHECK(d.idx_stride >= 1 && d.idx_n >= (int64_t)(nt - 1) * d.idx_stride + 1, "idx / idx_keys do not hold ntok entries");
            for (size_t t = 0; t < nt; t++) {
                const int64_t row = d.idx_keys ? (int64_t)key_code(d.idx_keys[t * d.idx_stride]) : (int64_t)d.idx[t * d.idx_stride];
                Q3_CHECK(row >= 0 && row < d.x_rows, "a selected row lies outside x");
            }
        } else Q3_CHECK(d.ntok <= d.x_rows, "x holds fewer than ntok rows");
    } else if (d.op != Q3TTS_GG_MATVEC) {
        Q3_CHECK(d.x && d.x_floats >= (int64_t)(nt * k), "x does not hold [ntok][k]");
    }
    if (d.op == Q3TTS_GG_RMSNORM) Q3_CHECK(d.u && holds(d.out, nt * k), "weight missing or out too small");
    if (mat) {
        Q3_CHECK(d.w && d.out_stride >= d.nrows && holds(d.out, (nt - 1) * d.out_stride + d.nrows), "weights missing, out_stride < nrows or out too small");
        w.row_bytes = q3_gguf_row_bytes(w.type, w.k);
    }
    // ---- uploads, the launch, downloads ----
    DevBuf<uint8_t> dw; DevBuf<int32_t> didx; DevBuf<unsigned long long> dkeys;
    if (d.op != Q3TTS_GG_QUANT) out.up(d.out, 0, "out");
    if (quant) { q8.up(d.q8, 0, "q8"); d8.up(d.d8, 0, "d8"); qk.up(d.qk, 0, "qk"); dk.up(d.dk, 0, "dk"); bs.up(d.bs, 0, "bs"); }
    if (d.op != Q3TTS_GG_MATVEC) { dx.alloc((size_t)d.x_floats); dx.upload(d.x, dx.n); }
    if (d.op == Q3TTS_GG_LOAD_ROWS) {
        if (d.idx) { didx.alloc((size_t)d.idx_n); didx.upload(d.idx, didx.n); }
        if (d.idx_keys) { dkeys.alloc((size_t)d.idx_n); dkeys.upload((const unsigned long long*)d.idx_keys, dkeys.n); }
        gg_load_rows(0, dx.p, d.x_stride, didx.p, d.idx_stride, dkeys.p, d.k, out.p(), d.ntok);
    } else if (d.op == Q3TTS_GG_RMSNORM) {
        du.alloc(k); du.upload(d.u, k);
        gg_rmsnorm(0, dx.p, du.p, d.k, d.eps, out.p(), d.ntok);
    } else {
        const GgAct act{q8.p(), d8.p(), qk.p(), dk.p(), bs.p()};
        if (mat) { dw.alloc(w.row_bytes * (size_t)d.rows); dw.upload((const uint8_t*)d.w, dw.n); w.p = dw.p; }
        if (d.op != Q3TTS_GG_MATVEC) gg_quant(0, dx.p, d.k, act, d.ntok);
        if (mat) gg_matvec(0, w, d.row0, d.nrows, act, out.p(), d.out_stride, d.ntok);
    }
    Q3_LAUNCH_CHECK();
    Q3_HIP(hipDeviceSynchronize());
    out.down(); q8.down(); d8.down(); qk.down(); dk.down(); bs.down();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] output formats: the host-only half (pcm_out.h) */
int q3tts_pcm_out_plan(int32_t rate, int32_t* L, int32_t* M, int32_t* n_taps, int32_t* taps_per_phase) {
    Q3_API_BEGIN
    PcmPlan p;
    Q3_CHECK(pcm_plan(rate, &p), "unknown sample rate");
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (n_taps) *n_taps = p.n_taps;
    if (taps_per_phase) *taps_per_phase = p.taps_per_phase;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int64_t q3tts_pcm_out_filter(int32_t rate, float* h32, int64_t cap) {
    Q3_API_BEGIN
    Q3_CHECK(pcm_rate_index(rate) >= 0, "unknown sample rate");
    const std::vector<float> h = pcm_filter(rate);
    Q3_CHECK((h32 || h.empty()) && cap >= (int64_t)h.size(), "h32 is too small for the rate's taps");
    std::copy(h.begin(), h.end(), h32);
    return (int64_t)h.size();
    Q3_API_END(Q3TTS_ERR)
}
int64_t q3tts_pcm_out_samples(int32_t rate, int64_t n_native) { return pcm_samples_of_native(rate, n_native); }
int q3tts_pcm_format_check(const q3tts_pcm_format* f) {
    Q3_API_BEGIN
    Q3_CHECK(f, "null format");
    if (const char* why = pcm_format_why_not(f->sample_rate, f->encoding)) throw Error(why);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] the convert kernel over guarded host buffers (include/q3tts.h): one launch_pcm_convert per chunk, each stream's output appended
 * behind its earlier chunks' inside its guarded buffer on the device, everything downloaded whole. */
int q3tts_op_pcm_convert(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                         const q3tts_pcm_format* fmt, const int32_t* reset_before, void* const* out, const int64_t* out_bytes, int64_t* n_out,
                         float* hist_store) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(in && chunk_samples && streams && fmt && out && out_bytes && n_out && hist_store, "null argument");
    Q3_CHECK(n_chunks >= 1 && n_streams >= 1 && n_streams <= 65536, "bad chunk / stream count");
    // every chunk is checked as its launch will be, before anything is allocated
    for (int c = 0; c < n_chunks; c++)
        if (const char* why = pcm_convert_refusal(G, G, chunk_samples[c], streams + (size_t)c * G, n_streams, fmt)) throw Error(std::string("pcm convert: ") + why);
    std::vector<int64_t> esz(G), need(G, 0);
    for (int g = 0; g < G; g++) {
        esz[g] = fmt[g].encoding == Q3_PCM_S16 ? 2 : 4;
        for (int c = 0; c < n_chunks; c++) need[g] += pcm_samples_of_native(fmt[g].sample_rate, chunk_samples[c]) * esz[g];
    }
    GuardedRun r(in, G, chunk_samples, n_chunks, false, streams, reset_before, esz, need, nullptr, out, out_bytes, nullptr, nullptr);
    GuardedStore hist(hist_store, (size_t)n_streams * 2 * Q3_PCM_HIST);
    PcmConverter conv(n_streams, G);
    conv.hist = hist.core();
    std::vector<int64_t> cnt(G);
    while (r.next()) {
        for (int g = 0; g < G; g++) if (r.reset(g)) conv.reset_async(0, r.sl[g]);
        launch_pcm_convert(0, conv, r.x, G, r.T, r.sl, fmt, r.d_out.p, r.off.data(), cnt.data());
        for (int g = 0; g < G; g++) {
            if (pcm_format_native(fmt[g])) r.copy_native(g);
            else r.bytes[g] += cnt[g] * esz[g];
        }
    }
    r.finish(n_out, nullptr, nullptr);
    hist.download();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] speaking rate: the host-only half (sched_logic.h, tsm.h) */
int64_t q3tts_tsm_samples(int32_t rate_pct, int64_t n_native, int32_t final) { return tsm_out_samples(rate_pct, n_native, final != 0); }
int q3tts_tsm_windows(float* w, float* w2) {
    Q3_API_BEGIN
    Q3_CHECK(w && w2, "null argument");
    tsm_windows(w, w2);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] the stretch kernel over guarded host buffers (include/q3tts.h): one launch_tsm_stretch per chunk and one more for the flush, each
 * stream's hops appended behind its earlier ones inside its guarded buffer on the device, everything downloaded whole. */
int q3tts_op_tsm(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                 const int32_t* rate_pct, const int32_t* encoding, const int32_t* reset_before, int32_t flush, void* const* out,
                 const int64_t* out_bytes, int64_t* n_out, int32_t* const* delta_trace, const int64_t* trace_len, float* hist_store) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(in && chunk_samples && streams && rate_pct && encoding && out && out_bytes && n_out && delta_trace && trace_len && hist_store, "null argument");
    Q3_CHECK(n_chunks >= 1 && n_streams >= 1 && n_streams <= 65536, "bad chunk / stream count");
    // every chunk is checked as its launch will be, and every count is worked out as the launcher will, before anything is allocated
    for (int c = 0; c < n_chunks; c++)
        if (const char* why = tsm_launch_refusal(G, G, chunk_samples[c], false, streams + (size_t)c * G, n_streams, rate_pct, encoding)) throw Error(std::string("tsm stretch: ") + why);
    std::vector<int64_t> frames, need, esz;
    prosody_op_plan(G, chunk_samples, n_chunks, flush != 0, streams, n_streams, reset_before, rate_pct, nullptr, encoding, frames, need, esz);
    GuardedRun r(in, G, chunk_samples, n_chunks, flush != 0, streams, reset_before, esz, need, &frames, out, out_bytes, delta_trace, trace_len);
    GuardedStore hist(hist_store, (size_t)n_streams * Q3_TSM_HIST);
    TsmStretcher ts(n_streams, G);
    ts.hist = hist.core();
    std::vector<int64_t> cnt(G);
    while (r.next()) {
        for (int g = 0; g < G; g++) if (r.reset(g)) ts.reset_async(0, r.sl[g]);
        launch_tsm_stretch(0, ts, r.x, G, r.T, r.flushing(), r.sl, rate_pct, encoding, r.d_out.p, r.off.data(), cnt.data(), r.d_trace.p, r.toff.data());
        for (int g = 0; g < G; g++) {
            if (rate_pct[g] == 100) r.copy_native(g);
            else { r.bytes[g] += cnt[g] * esz[g]; r.fr[g] += cnt[g] / Q3_TSM_HOP; }
        }
    }
    r.finish(n_out, &need, "the launcher's counts differ from the plan");
    hist.download();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] pitch: the host-only half (sched_logic.h, pitch.h) */
int64_t q3tts_pitch_samples(int32_t rate_pct, int32_t pitch_pct, int64_t n_native, int32_t final) { return pitch_out_samples(rate_pct, pitch_pct, n_native, final != 0); }
int q3tts_pitch_plan(int32_t pitch_pct, int32_t* L, int32_t* M, int32_t* n_taps, int32_t* taps_per_output) {
    PitchPlan p;
    if (!pitch_plan(pitch_pct, &p)) { set_last_error("pitch out of range [50, 200]"); return Q3TTS_ERR; }
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (n_taps) *n_taps = p.n_taps;
    if (taps_per_output) *taps_per_output = p.taps_per_output;
    return Q3TTS_OK;
}
int64_t q3tts_pitch_filter(int32_t pitch_pct, float* h32, int64_t cap) {
    Q3_API_BEGIN
    const std::vector<float> h = pitch_filter(pitch_pct);
    Q3_CHECK(!h.empty(), "pitch out of range [50, 200]");
    Q3_CHECK(h32 && cap >= (int64_t)h.size(), "filter buffer too small or missing");
    std::copy(h.begin(), h.end(), h32);
    return (int64_t)h.size();
    Q3_API_END(-1)
}

/* [EXT] the pitch kernel over guarded host buffers (include/q3tts.h): per chunk one launch_tsm_pitch and, when a stream has a rate alone, one
 * launch_tsm_stretch over the same history store, as a decode pass runs them; one more of each for the flush.  Each stream's samples are
 * appended behind its earlier ones inside its guarded buffer on the device, everything downloaded whole. */
int q3tts_op_pitch(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                   const int32_t* rate_pct, const int32_t* pitch_pct, const int32_t* encoding, const int32_t* reset_before, int32_t flush,
                   void* const* out, const int64_t* out_bytes, int64_t* n_out, int32_t* const* delta_trace, const int64_t* trace_len,
                   float* hist_store, float* zhist_store) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(in && chunk_samples && streams && rate_pct && pitch_pct && encoding && out && out_bytes && n_out && delta_trace && trace_len && hist_store && zhist_store, "null argument");
    Q3_CHECK(n_chunks >= 1 && n_streams >= 1 && n_streams <= 65536, "bad chunk / stream count");
    // every chunk is checked as its launch will be, and every count is worked out as the launchers will, before anything is allocated
    for (int c = 0; c < n_chunks; c++)
        if (const char* why = pitch_launch_refusal(G, G, chunk_samples[c], false, streams + (size_t)c * G, n_streams, rate_pct, pitch_pct, encoding)) throw Error(std::string("tsm pitch: ") + why);
    std::vector<int32_t> kind(G), tpct(G, 100);   // 0 native, 1 a rate alone (the stretcher's), 2 a pitch (the shifter's)
    bool any_rate = false;
    for (int g = 0; g < G; g++) {
        kind[g] = pitch_pct[g] != 100 ? 2 : (rate_pct[g] != 100 ? 1 : 0);
        if (kind[g] == 1) { tpct[g] = rate_pct[g]; any_rate = true; }
    }
    std::vector<int64_t> frames, need, esz;
    prosody_op_plan(G, chunk_samples, n_chunks, flush != 0, streams, n_streams, reset_before, rate_pct, pitch_pct, encoding, frames, need, esz);
    GuardedRun r(in, G, chunk_samples, n_chunks, flush != 0, streams, reset_before, esz, need, &frames, out, out_bytes, delta_trace, trace_len);
    GuardedStore hist(hist_store, (size_t)n_streams * Q3_TSM_HIST), zhist(zhist_store, (size_t)n_streams * Q3_PITCH_HIST);
    PitchShifter ps(n_streams, G);
    ps.hist = hist.core(); ps.zhist = zhist.core();
    std::unique_ptr<TsmStretcher> ts;
    if (any_rate) { ts.reset(new TsmStretcher(n_streams, G)); ts->hist = ps.hist; }
    std::vector<int64_t> cnt(G), pcnt(G), kd0(G);
    while (r.next()) {
        for (int g = 0; g < G; g++) {
            if (r.reset(g)) { ps.reset_async(0, r.sl[g]); if (ts) ts->reset_async(0, r.sl[g]); }
            cnt[g] = pcnt[g] = 0;
            kd0[g] = ps.k_done[(size_t)r.sl[g]];
        }
        launch_tsm_pitch(0, ps, r.x, G, r.T, r.flushing(), r.sl, rate_pct, pitch_pct, encoding, r.d_out.p, r.off.data(), pcnt.data(), r.d_trace.p, r.toff.data());
        if (ts) launch_tsm_stretch(0, *ts, r.x, G, r.T, r.flushing(), r.sl, tpct.data(), encoding, r.d_out.p, r.off.data(), cnt.data(), r.d_trace.p, r.toff.data());
        for (int g = 0; g < G; g++) {
            if (kind[g] == 0) r.copy_native(g);
            else if (kind[g] == 1) { r.bytes[g] += cnt[g] * esz[g]; r.fr[g] += cnt[g] / Q3_TSM_HOP; }
            else { r.bytes[g] += pcnt[g] * esz[g]; r.fr[g] += ps.k_done[(size_t)r.sl[g]] - kd0[g]; }
        }
    }
    r.finish(n_out, &need, "the launchers' counts differ from the plan");
    hist.download(); zhist.download();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] volume: the host-only half (sched_logic.h) */
float q3tts_volume_gain(int32_t db10) { return volume_gain(db10); }

/* [EXT] the volume kernel over guarded host buffers (include/q3tts.h): one launch_volume per chunk, in place on the run's copy of the chunk
 * as a decode pass runs it on the output conv's buffer; each stream's samples are then appended behind its earlier ones inside its guarded
 * buffer on the device, everything downloaded whole. */
int q3tts_op_volume(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                    const int32_t* vol_db10, const int32_t* reset_before, float* const* out, const int64_t* out_bytes, int64_t* n_out,
                    float* const* gain_trace, const int64_t* trace_len, float* hist_store) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(in && chunk_samples && streams && vol_db10 && out && out_bytes && n_out && (!gain_trace || trace_len) && hist_store, "null argument");
    Q3_CHECK(n_chunks >= 1 && n_streams >= 1 && n_streams <= 65536, "bad chunk / stream count");
    // every chunk is checked as its launch will be before anything is allocated
    for (int c = 0; c < n_chunks; c++)
        if (const char* why = volume_launch_refusal(G, G, chunk_samples[c], streams + (size_t)c * G, n_streams, vol_db10)) throw Error(std::string("volume: ") + why);
    int64_t total = 0;
    for (int c = 0; c < n_chunks; c++) total += chunk_samples[c];
    const std::vector<int64_t> esz((size_t)G, 4), need((size_t)G, total * 4), entries((size_t)G, total);
    GuardedRun r(in, G, chunk_samples, n_chunks, false, streams, reset_before, esz, need, &entries, reinterpret_cast<void* const*>(out), out_bytes,
                 reinterpret_cast<int32_t* const*>(gain_trace), trace_len);   // a trace entry is four bytes, whatever it holds
    GuardedStore hist(hist_store, (size_t)n_streams * Q3_VOL_HIST);
    VolumeStage vs(n_streams, G);
    vs.hist = hist.core();
    while (r.next()) {
        for (int g = 0; g < G; g++) if (r.reset(g)) vs.reset_async(0, r.sl[g]);
        launch_volume(0, vs, const_cast<float*>(r.x), G, r.T, r.sl, vol_db10, gain_trace ? reinterpret_cast<float*>(r.d_trace.p) : nullptr, r.toff.data());
        for (int g = 0; g < G; g++) { r.copy_native(g); r.fr[g] += r.T; }
    }
    r.finish(n_out, &need, "the chunks differ from the plan");
    hist.download();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] loudness: the host-only half (loudness.h) */
int q3tts_loudness_tables(double* coef, double* m) {
    Q3_API_BEGIN
    Q3_CHECK(coef && m, "null argument");
    LoudTables t;
    loud_tables(&t);
    std::copy(t.coef, t.coef + 10, coef); std::copy(t.m, t.m + 16, m);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_loudness_gate(const double* rows, int32_t n, q3tts_loudness* out) {
    Q3_API_BEGIN
    Q3_CHECK(out && n >= 0 && (rows || n == 0), "null argument or negative count");
    LoudResult r;
    loud_gate(rows, n, &r);
    out->integrated_lufs = r.integrated_lufs; out->momentary_max_lufs = r.momentary_max_lufs; out->peak_dbfs = r.peak_dbfs;
    out->n_blocks = r.n_blocks; out->n_gated = r.n_gated;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int32_t q3tts_loudness_gain_db10(double measured_lufs, double target_lufs) { return loud_gain_db10(measured_lufs, target_lufs); }

/* [EXT] the loudness kernel over guarded host buffers (include/q3tts.h): one launch_loudness per chunk on the run's copy of the chunk, as a
 * decode pass runs it on the output conv's buffer; each stream's rows are appended behind its earlier ones inside its guarded buffer on the
 * device, everything downloaded whole.  The call keeps every slot's position as the decoder thread keeps a job's. */
int q3tts_op_loudness(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                      const int32_t* metered, const int32_t* reset_before, double* const* rows, const int64_t* rows_bytes, int64_t* n_rows,
                      double* state_store) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(in && chunk_samples && streams && metered && rows && rows_bytes && n_rows && state_store, "null argument");
    Q3_CHECK(n_chunks >= 1 && n_streams >= 1 && n_streams <= 65536, "bad chunk / stream count");
    Q3_CHECK(G >= 1 && G <= 65536, "loudness: group size out of range");
    // every chunk is checked as its launch will be, and every row count is worked out as the launcher will, before anything is allocated
    const std::vector<int64_t> esz((size_t)G, 16);
    std::vector<int64_t> need((size_t)G, 0), pos((size_t)n_streams, 0), at((size_t)G, 0), cnt((size_t)G, 0);
    for (int c = 0; c < n_chunks; c++) {
        const int32_t* sl = streams + (size_t)c * G;
        if (const char* why = loudness_launch_refusal(G, G, chunk_samples[c], sl, n_streams, metered, std::vector<int64_t>((size_t)G, 0).data())) throw Error(std::string("loudness: ") + why);
        for (int g = 0; g < G; g++) {
            int64_t& p = pos[(size_t)sl[g]];
            if (reset_before && reset_before[(size_t)c * G + g]) p = 0;
            if (metered[g]) need[(size_t)g] += loud_blocks(p, chunk_samples[c]) * 16;
            p += chunk_samples[c];
        }
    }
    GuardedRun r(in, G, chunk_samples, n_chunks, false, streams, reset_before, esz, need, nullptr, reinterpret_cast<void* const*>(rows), rows_bytes, nullptr, nullptr);
    GuardedStoreOf<double> state(state_store, (size_t)n_streams * Q3_LOUD_STATE);
    LoudnessStage ls(n_streams, G);
    ls.state = state.core();
    std::fill(pos.begin(), pos.end(), 0);
    while (r.next()) {
        for (int g = 0; g < G; g++) {
            if (r.reset(g)) { ls.reset_async(0, r.sl[g]); pos[(size_t)r.sl[g]] = 0; }
            at[(size_t)g] = pos[(size_t)r.sl[g]];
        }
        launch_loudness(0, ls, r.x, G, r.T, r.sl, metered, at.data(), r.d_out.p, r.off.data(), cnt.data());
        for (int g = 0; g < G; g++) { r.bytes[g] += cnt[(size_t)g] * 16; pos[(size_t)r.sl[g]] += r.T; }
    }
    r.finish(n_rows, &need, "the launcher's counts differ from the plan");
    state.download();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_mel_frames(int32_t n) { return mel_frames(n); }

/* [EXT] reference audio intake: the host-only half (intake.h) */
int q3tts_intake_plan(int32_t rate, int32_t* L, int32_t* M, int32_t* n_taps, int32_t* taps_per_output) {
    Q3_API_BEGIN
    IntakePlan p;
    if (const char* why = intake_rate_why_not(rate)) throw Error(why);
    Q3_CHECK(intake_plan(rate, &p), "no tile fits this ratio");
    if (L) *L = p.L;
    if (M) *M = p.M;
    if (n_taps) *n_taps = p.n_taps;
    if (taps_per_output) *taps_per_output = p.taps;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int64_t q3tts_intake_filter(int32_t rate, float* h32, int64_t cap) {
    Q3_API_BEGIN
    if (const char* why = intake_rate_why_not(rate)) throw Error(why);
    const std::vector<float> h = intake_filter(rate);
    Q3_CHECK((h32 || h.empty()) && cap >= (int64_t)h.size(), "h32 is too small for the rate's taps");
    std::copy(h.begin(), h.end(), h32);
    return (int64_t)h.size();
    Q3_API_END(Q3TTS_ERR)
}
int64_t q3tts_intake_samples(int32_t rate, int64_t n_frames) {
    Q3_API_BEGIN
    if (const char* why = intake_rate_why_not(rate)) throw Error(why);
    Q3_CHECK(n_frames >= 0, "negative frame count");
    return intake_samples(rate, n_frames);
    Q3_API_END(Q3TTS_ERR)
}
int32_t q3tts_intake_tile(int32_t rate) {
    Q3_API_BEGIN
    IntakePlan p;
    if (const char* why = intake_rate_why_not(rate)) throw Error(why);
    Q3_CHECK(intake_plan(rate, &p), "no tile fits this ratio");
    return p.tile;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_intake_check(const q3tts_intake_clip* c) {
    Q3_API_BEGIN
    if (const char* why = intake_refusal(c)) throw Error(std::string("intake: ") + why);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_wav_probe(const void* bytes, int64_t n, q3tts_wav_info* out) {
    Q3_API_BEGIN
    q3tts_wav_info w{};
    if (const char* why = wav_probe(bytes, n, &w)) throw Error(std::string("WAV error: ") + why);
    *out = w;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

/* [EXT] the intake itself: host clips in, host samples out, one launch of k_intake (intake.hip) */
int q3tts_intake(int32_t device, const q3tts_intake_clip* clips, int32_t n_clips, float* const* out, const int64_t* out_cap, int64_t* n_out) {
    Q3_API_BEGIN
    require_gpu();
    int nd = 0;
    Q3_HIP(hipGetDeviceCount(&nd));
    Q3_CHECK(device >= 0 && device < nd, "device out of range");
    intake_run(intake_stage(device), clips, n_clips, out, out_cap, n_out);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_wav_intake(const char* path, int32_t downmix, int32_t device, float* out, int64_t cap, int64_t* n_out, q3tts_wav_info* info) {
    Q3_API_BEGIN
    Q3_CHECK(path && n_out, "null argument");
    FILE* f = fopen(path, "rb");
    if (!f) throw Error(std::string("WAV error: cannot open ") + path);
    std::vector<unsigned char> d;
    unsigned char buf[65536];
    size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) d.insert(d.end(), buf, buf + got);
    fclose(f);
    q3tts_wav_info w{};
    if (const char* why = wav_probe(d.data(), (int64_t)d.size(), &w)) throw Error(std::string("WAV error: ") + why);
    const q3tts_intake_clip c{d.data() + w.data_offset, w.n_frames, w.sample_rate, w.channels, w.sample_format, downmix};
    if (const char* why = intake_refusal(&c)) throw Error(std::string("intake: ") + why);
    const int64_t n = intake_samples(c.sample_rate, c.n_frames);
    if (!out && cap == 0) {   // the size query
        *n_out = n;
        if (info) *info = w;
        return Q3TTS_OK;
    }
    require_gpu();
    int nd = 0;
    Q3_HIP(hipGetDeviceCount(&nd));
    Q3_CHECK(device >= 0 && device < nd, "device out of range");
    int64_t cnt = 0;
    float* const outs[1] = {out};
    intake_run(intake_stage(device), &c, 1, outs, &cap, &cnt);
    *n_out = cnt;
    if (info) *info = w;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

} // extern "C"

// ---------------- ONNX graph ingestion (host only, no GPU needed) ----------------
#include "onnx_reader.h"
#include "onnx_exec.h"
struct q3tts_onnx { std::unique_ptr<OnnxModel> m; std::string text; };
extern "C" {
int q3tts_onnx_open(const char* path, q3tts_onnx** out) {
    Q3_API_BEGIN
    Q3_CHECK(path && out, "null argument");
    auto* h = new q3tts_onnx();
    try { h->m.reset(new OnnxModel(path)); } catch (...) { delete h; throw; }
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_onnx_close(q3tts_onnx* m) { delete m; }
int q3tts_onnx_counts(q3tts_onnx* m, int32_t* n_nodes, int32_t* n_init, int32_t* n_in, int32_t* n_out) {
    if (!m) return Q3TTS_ERR;
    if (n_nodes) *n_nodes = (int32_t)m->m->nodes.size();
    if (n_init) *n_init = (int32_t)m->m->initializers.size();
    if (n_in) *n_in = (int32_t)m->m->inputs.size();
    if (n_out) *n_out = (int32_t)m->m->outputs.size();
    return Q3TTS_OK;
}
int64_t q3tts_onnx_summary(q3tts_onnx* m, char* buf, int64_t cap) {
    if (!m) return -1;
    m->text = m->m->summary();
    if (buf && cap > 0) { const size_t n = std::min((size_t)cap - 1, m->text.size()); std::memcpy(buf, m->text.data(), n); buf[n] = 0; }
    return (int64_t)m->text.size() + 1;
}
int q3tts_onnx_node(q3tts_onnx* m, int32_t i, const char** op_type, const char** name, int32_t* n_in, int32_t* n_out, int32_t* n_attr) {
    Q3_API_BEGIN
    Q3_CHECK(m && i >= 0 && i < (int)m->m->nodes.size(), "node index out of range");
    const OnnxNode& n = m->m->nodes[i];
    if (op_type) *op_type = n.op_type.c_str();
    if (name) *name = n.name.c_str();
    if (n_in) *n_in = (int32_t)n.inputs.size();
    if (n_out) *n_out = (int32_t)n.outputs.size();
    if (n_attr) *n_attr = (int32_t)n.attrs.size();
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
const char* q3tts_onnx_node_input(q3tts_onnx* m, int32_t i, int32_t j) {
    return (m && i >= 0 && i < (int)m->m->nodes.size() && j >= 0 && j < (int)m->m->nodes[i].inputs.size()) ? m->m->nodes[i].inputs[j].c_str() : nullptr;
}
const char* q3tts_onnx_node_output(q3tts_onnx* m, int32_t i, int32_t j) {
    return (m && i >= 0 && i < (int)m->m->nodes.size() && j >= 0 && j < (int)m->m->nodes[i].outputs.size()) ? m->m->nodes[i].outputs[j].c_str() : nullptr;
}
/* INT / INTS attribute -> values (returns the count, -1 when the node has no such attribute) */
int32_t q3tts_onnx_node_attr_ints(q3tts_onnx* m, int32_t i, const char* attr, int64_t* out, int32_t cap) {
    if (!m || i < 0 || i >= (int)m->m->nodes.size() || !attr) return -1;
    const OnnxAttr* a = m->m->nodes[i].attr(attr);
    if (!a) return -1;
    if (a->type == 2 || (a->ints.empty() && a->type == 0)) { if (out && cap > 0) out[0] = a->i; return 1; }
    for (int k = 0; k < (int)a->ints.size() && k < cap; k++) out[k] = a->ints[k];
    return (int32_t)a->ints.size();
}
int32_t q3tts_onnx_node_attr_float(q3tts_onnx* m, int32_t i, const char* attr, float* out) {
    if (!m || i < 0 || i >= (int)m->m->nodes.size() || !attr || !out) return -1;
    const OnnxAttr* a = m->m->nodes[i].attr(attr);
    if (!a) return -1;
    *out = a->f;
    return 1;
}
int q3tts_onnx_initializer(q3tts_onnx* m, int32_t i, const char** name, int32_t* dtype, int64_t* dims8, int32_t* ndims, const void** data, int64_t* nbytes) {
    Q3_API_BEGIN
    Q3_CHECK(m && i >= 0 && i < (int)m->m->initializers.size(), "initializer index out of range");
    const OnnxTensor& t = m->m->initializers[i];
    Q3_CHECK(t.dims.size() <= 8, "more than 8 dimensions");
    if (name) *name = t.name.c_str();
    if (dtype) *dtype = t.data_type;
    if (ndims) *ndims = (int32_t)t.dims.size();
    if (dims8) for (size_t d = 0; d < t.dims.size(); d++) dims8[d] = t.dims[d];
    const void* p = t.raw; int64_t nb = (int64_t)t.raw_bytes;
    if (!p && !t.float_data.empty()) { p = t.float_data.data(); nb = (int64_t)t.float_data.size() * 4; }
    else if (!p && !t.int64_data.empty()) { p = t.int64_data.data(); nb = (int64_t)t.int64_data.size() * 8; }
    else if (!p && !t.int32_data.empty()) { p = t.int32_data.data(); nb = (int64_t)t.int32_data.size() * 4; }
    if (data) *data = p;
    if (nbytes) *nbytes = nb;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
const char* q3tts_onnx_op_kernel(const char* op_type) { return op_type ? onnx_op_kernel(op_type) : nullptr; }
/* 0: the graph carries the streaming-decoder inputs / outputs of onnx.rs:355-455; 1: something is missing (listed in buf) */
int q3tts_onnx_decoder_contract(q3tts_onnx* m, char* buf, int64_t cap) {
    if (!m) return Q3TTS_ERR;
    const std::string miss = m->m->check_decoder_contract();
    if (buf && cap > 0) { const size_t n = std::min((size_t)cap - 1, miss.size()); std::memcpy(buf, miss.data(), n); buf[n] = 0; }
    return miss.empty() ? 0 : 1;
}
} // extern "C"

// ---------------- tokenizer (host only) ----------------
#include "tokenizer.h"
struct q3tts_tokenizer { std::unique_ptr<Tokenizer> t; std::string text; };
extern "C" {
int q3tts_tokenizer_open(const char* tokenizer_json, q3tts_tokenizer** out) {
    Q3_API_BEGIN
    Q3_CHECK(tokenizer_json && out, "null argument");
    auto* h = new q3tts_tokenizer();
    try { h->t.reset(new Tokenizer(tokenizer_json)); } catch (...) { delete h; throw; }
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_tokenizer_close(q3tts_tokenizer* t) { delete t; }
/* returns the number of ids (which may exceed cap: call again with a larger buffer), < 0 on error */
int32_t q3tts_tokenizer_encode(q3tts_tokenizer* t, const char* text_utf8, int32_t* ids, int32_t cap) {
    Q3_API_BEGIN
    Q3_CHECK(t && text_utf8, "null argument");
    const std::vector<int32_t> v = t->t->encode(text_utf8);
    for (size_t i = 0; i < v.size() && (int32_t)i < cap; i++) ids[i] = v[i];
    return (int32_t)v.size();
    Q3_API_END(-1)
}
/* returns the byte length of the decoded UTF-8 text (without NUL; may exceed cap - 1), < 0 on error */
int64_t q3tts_tokenizer_decode(q3tts_tokenizer* t, const int32_t* ids, int32_t n, char* buf, int64_t cap) {
    Q3_API_BEGIN
    Q3_CHECK(t && (ids || n == 0) && n >= 0, "bad arguments");
    t->text = t->t->decode(std::vector<int32_t>(ids, ids + n));
    if (buf && cap > 0) { const size_t k = std::min((size_t)cap - 1, t->text.size()); std::memcpy(buf, t->text.data(), k); buf[k] = 0; }
    return (int64_t)t->text.size();
    Q3_API_END(-1)
}
int64_t q3tts_text_nfc(const char* utf8, char* out, int64_t cap) {
    try {
        if (!utf8) return 0;
        const std::string r = q3::nfc_utf8(utf8);
        if (out && cap > 0) { const size_t n = std::min<size_t>((size_t)cap - 1, r.size()); memcpy(out, r.data(), n); out[n] = 0; }
        return (int64_t)r.size() + 1;
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return -1; }
}
int32_t q3tts_tokenizer_vocab_size(q3tts_tokenizer* t) { return t ? t->t->vocab_size() : 0; }
} // extern "C"

// ---- ONNX graph execution (onnx_exec.h) ----
struct q3tts_onnx_session { std::unique_ptr<q3::OnnxSession> s; };
extern "C" {
int q3tts_onnx_session_open(const char* path, int32_t device, q3tts_onnx_session** out) {
    try {
        if (!path || !out) throw q3::Error("q3tts_onnx_session_open: null argument");
        auto* h = new q3tts_onnx_session();
        try { h->s.reset(new q3::OnnxSession(path, device)); } catch (...) { delete h; throw; }
        *out = h;
        return 0;
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
void q3tts_onnx_session_close(q3tts_onnx_session* s) { delete s; }
int32_t q3tts_onnx_session_unsupported(q3tts_onnx_session* s, char* buf, int64_t cap) {
    if (!s) return -1;
    const auto v = s->s->unsupported_ops();
    std::string t;
    for (size_t i = 0; i < v.size(); i++) t += (i ? "," : "") + v[i];
    if (buf && cap > 0) { const size_t n = std::min<size_t>((size_t)cap - 1, t.size()); memcpy(buf, t.data(), n); buf[n] = 0; }
    return (int32_t)v.size();
}
int q3tts_onnx_session_set_input(q3tts_onnx_session* s, const char* name, int32_t dtype, const void* data, const int64_t* shape, int32_t rank) {
    try {
        if (!s || !name || (rank > 0 && !shape)) throw q3::Error("q3tts_onnx_session_set_input: null argument");
        std::vector<int64_t> sh(shape, shape + rank);
        int64_t n = 1; for (auto d : sh) { if (d < 0) throw q3::Error("negative dimension"); n *= d; }
        if (n > 0 && !data) throw q3::Error("q3tts_onnx_session_set_input: null data");
        s->s->set_input(name, dtype, data, sh);
        return 0;
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
int q3tts_onnx_session_run(q3tts_onnx_session* s) {
    try { if (!s) throw q3::Error("null session"); s->s->run(); return 0; } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
int q3tts_onnx_session_output_info(q3tts_onnx_session* s, const char* name, int32_t* dtype, int32_t* rank, int64_t* shape8) {
    try {
        if (!s || !name) throw q3::Error("null argument");
        const q3::XTensor& t = s->s->value(name);
        if (t.shape.size() > 8) throw q3::Error("rank above 8");
        if (dtype) *dtype = t.dtype;
        if (rank) *rank = (int32_t)t.shape.size();
        if (shape8) for (size_t i = 0; i < t.shape.size(); i++) shape8[i] = t.shape[i];
        return 0;
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
int q3tts_onnx_session_output(q3tts_onnx_session* s, const char* name, void* dst, int64_t cap_bytes) {
    try {
        if (!s || !name || !dst || cap_bytes < 0) throw q3::Error("null argument");
        s->s->fetch(s->s->value(name), dst, (size_t)cap_bytes);
        return 0;
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
int64_t q3tts_onnx_session_launches(q3tts_onnx_session* s) { return s ? (int64_t)s->s->launches() : 0; }
int q3tts_onnx_op_executable(const char* op_type) { return op_type && q3::onnx_exec_supports(op_type) ? 1 : 0; }
}
struct q3tts_onnx_decoder { std::unique_ptr<q3::OnnxStreamDecoder> d; std::vector<float> last; }; // last = the most recent chunk's PCM (re-fetchable)
extern "C" {
int q3tts_onnx_decoder_open(const char* path, int32_t device, q3tts_onnx_decoder** out) {
    try {
        if (!path || !out) throw q3::Error("q3tts_onnx_decoder_open: null argument");
        auto* h = new q3tts_onnx_decoder();
        try { h->d.reset(new q3::OnnxStreamDecoder(path, device)); } catch (...) { delete h; throw; }
        *out = h;
        return 0;
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
void q3tts_onnx_decoder_close(q3tts_onnx_decoder* d) { delete d; }
int q3tts_onnx_decoder_reset(q3tts_onnx_decoder* d) {
    try { if (!d) throw q3::Error("null decoder"); d->d->reset(); d->last.clear(); return 0; } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
static int onnx_decoder_copy_out(q3tts_onnx_decoder* d, float* pcm, int64_t cap, int64_t* n_out) {
    *n_out = (int64_t)d->last.size();
    if ((int64_t)d->last.size() > cap || (!pcm && !d->last.empty())) {
        q3::set_last_error("pcm buffer too small for the chunk (" + std::to_string(d->last.size()) + " samples); the chunk is kept: call q3tts_onnx_decoder_fetch with a larger buffer");
        return 2;
    }
    if (!d->last.empty()) memcpy(pcm, d->last.data(), d->last.size() * 4);
    return 0;
}
int q3tts_onnx_decoder_decode(q3tts_onnx_decoder* d, const int64_t* codes, int32_t n_frames, int32_t is_final, float* pcm, int64_t cap, int64_t* n_out) {
    try {
        if (!d || !n_out) throw q3::Error("q3tts_onnx_decoder_decode: null argument");
        d->last = d->d->decode(codes, n_frames, is_final != 0); // the streaming state has advanced: the PCM stays in the handle until the next decode / reset
        return onnx_decoder_copy_out(d, pcm, cap, n_out);
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
int q3tts_onnx_decoder_fetch(q3tts_onnx_decoder* d, float* pcm, int64_t cap, int64_t* n_out) {
    try {
        if (!d || !n_out) throw q3::Error("q3tts_onnx_decoder_fetch: null argument");
        return onnx_decoder_copy_out(d, pcm, cap, n_out);
    } catch (const std::exception& e) { q3::set_last_error(e.what()); return 1; }
}
}
