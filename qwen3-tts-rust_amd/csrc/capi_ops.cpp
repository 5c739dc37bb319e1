// capi_ops.cpp -- kernel-level C-ABI entry points for the parity tests (host buffers in, host buffers out).
#include "../../include/q3tts.h"
#include "transformer.h"
#include "host_logic.h"
#include "kdev.h"
#include "codec.h"

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

static void attention_op_run(q3tts_attention_desc* dp) {
    Q3_CHECK(dp, "null attention descriptor");
    q3tts_attention_desc& d = *dp;
    Q3_CHECK(d.ntok >= 1 && d.n_head >= 1 && d.n_kv >= 1, "bad attention shape");
    const int form = d.form == Q3TTS_ATTN_AUTO ? attention_op_plan(d) : d.form;
    attention_op_check(d, form);
    const int nt = d.ntok, dq = d.n_head * 128, qs = d.qkv_stride;
    DevBuf<float> qkv((size_t)nt * qs); qkv.upload(d.qkv, qkv.n);
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
        launch_qk_rope_append(0, qkv.p, qs, nullptr, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv, d.layer, qrot.p, nt);
        launch_attention(0, qrot.p, d.n_head, d.n_kv, tm, kv, d.layer, att.p, aq.p, ad.p, nt);
        break;
    case ATTN_FUSED:
        launch_attention_fused(0, qkv.p, qs, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv, d.layer, aq.p, ad.p, nt);
        break;
    case ATTN_SHORT1: case ATTN_SHORT2:
        launch_attention_short(0, form == ATTN_SHORT1 ? 1 : 2, qkv.p, qs, d.n_head, d.n_kv, qn.p, kn.p, d.eps, rc.p, rs.p, d.n_ctx, sec.p, tm, kv,
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
    d.form_ran = form;
}

extern "C" {

int q3tts_op_attention(q3tts_attention_desc* d) {
    Q3_API_BEGIN
    require_gpu();
    attention_op_run(d);
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
    KqPart parts[3];
    int n = 0;
    for (int i = 0; i < nparts; i++) { parts[i] = KqPart{raws[i], types[i], rows[i]}; n += rows[i]; }
    DevBuf<uint8_t> storage;
    Q8Mat m = kqmat_from_host(parts, nparts, k, storage);
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
    KqPart parts[2] = {KqPart{gate_raw, type, ff}, KqPart{up_raw, type, ff}};
    DevBuf<uint8_t> storage;
    Q8Mat m = kqmat_from_host(parts, 2, k, storage);
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
    std::vector<float> wt((size_t)n_in * n_out);
    for (int o = 0; o < n_out; o++) for (int i = 0; i < n_in; i++) wt[(size_t)i * n_out + o] = w[(size_t)o * n_in + i];
    DevBuf<float> dx(n_in), dw(wt.size()), db(n_out), dy(n_out);
    dx.upload(x, n_in); dw.upload(wt.data(), wt.size()); db.upload(b, n_out);
    launch_project(0, dx.p, n_in, dw.p, db.p, n_in, n_out, dy.p, n_out, 1);
    Q3_HIP(hipDeviceSynchronize());
    dy.download(y, n_out);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_mel_frames(int32_t n) { const int plen = n + 768; return (plen > 1024 ? plen - 1024 : 0) / 256 + 1; }

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
