// kvq8.hip -- [EXT] KV cache type Q8_0 (q3tts_spec.h "KV cache type Q8_0"): the talker's attention step over int8 K/V pages.
//   k_qk_rope_append_q8   per-head RMSNorm + M-RoPE as k_qk_rope_append; q -> qrot f32; the K and V rows -> four int8 blocks of 32 + f16 scales
//   k_attention_q8kv<GRP> causal GQA attention of the GRP = n_head / n_kv query heads of one kv head from ONE read of its K and V rows
// Page unit of one (page, layer, kv head), KvCacheQ8:
//   K quants [4 blocks][64 pos][32] int8   a wave scoring 64 positions reads 2 KiB contiguous per block, each lane two 16-byte loads
//   K scales [4][64] f16
//   V quants [64 pos][128] int8            a 16-lane group reads one row, 8 bytes per lane
//   V scales [64][4] f16
#include "kernels.h"
#include "kdev.h"
#include <type_traits>

namespace q3 {

// amax of the 32-lane half-wave the lane sits in (a block of 32 consecutive elements); max is exact in any order
__device__ __forceinline__ float amax32(float a) {
    a = fmaxf(a, xor_lane<1>(a)); a = fmaxf(a, xor_lane<2>(a)); a = fmaxf(a, xor_lane<4>(a)); a = fmaxf(a, xor_lane<8>(a));
    return fmaxf(a, xor_lane<16>(a));
}
// spec S2 for one element of a block whose amax is known: d (f32) and the quant
__device__ __forceinline__ int quant1(float x, float amax, float* d) {
    const float dd = amax / 127.0f;
    const float id = (dd != 0.0f) ? (1.0f / dd) : 0.0f;
    *d = dd;
    return (int)q3_rintf(x * id);
}

// =====================================================================================================
// One wave per (token, head vector); lane l owns the rotation pair (x[l], x[l+64]): x[l] lies in block l/32, x[l+64] in block 2 + l/32, so a
// block's amax is a half-wave exchange.  Byte and f16 stores, all vector stores.
// =====================================================================================================
__global__ void __launch_bounds__(64) k_qk_rope_append_q8(QkvRows qkv, int n_head, int n_kv, const float* __restrict__ q_norm_w,
                                                          const float* __restrict__ k_norm_w, float eps, const float* __restrict__ rope_cos,
                                                          const float* __restrict__ rope_sin, int n_ctx, const int32_t* __restrict__ mrope_sec,
                                                          TokMeta tm, KvCacheQ8 kv, int layer, float* __restrict__ qrot) {
    const int hv = blockIdx.x, tok = blockIdx.y, lane = threadIdx.x;
    const float* vec = qkv.row(tok) + (size_t)hv * 128;
    const float x1 = vec[lane], x2 = vec[lane + 64];
    const int seq = tm.seq_of(tok), slot = tm.slot_of(tok);
    const int page = kv.page_of(seq, slot >> 6);
    const int ps = slot & 63;
    float o1 = x1, o2 = x2;   // the V row is the raw v
    if (hv < n_head + n_kv) {
        const float* w = hv < n_head ? q_norm_w : k_norm_w;
        float p = x1 * x1;
        p = q3_fmaf(x2, x2, p);
        const float ss = wave_sum_bfly(p);
        const float mean = ss / 128.0f;
        const float scale = 1.0f / q3_sqrtf(mean + eps);
        const float y1 = (x1 * scale) * w[lane], y2 = (x2 * scale) * w[lane + 64];
        int32_t sec[4] = { mrope_sec[0], mrope_sec[1], mrope_sec[2], mrope_sec[3] };
        int pp = tm.pos_of(tok, q3_mrope_stream(lane, sec));
        if (pp < 0) pp = 0;
        if (pp > n_ctx - 1) pp = n_ctx - 1;
        q3_rope_pair(y1, y2, rope_cos[(size_t)pp * 64 + lane], rope_sin[(size_t)pp * 64 + lane], &o1, &o2);
        if (hv < n_head) {
            float* dst = qrot + ((size_t)tok * n_head + hv) * 128;
            dst[lane] = o1; dst[lane + 64] = o2;
            return;
        }
    }
    float d1, d2;
    const int q1 = quant1(o1, amax32(q3_fabsf(o1)), &d1), q2 = quant1(o2, amax32(q3_fabsf(o2)), &d2);
    const int b1 = lane >> 5, b2 = 2 + (lane >> 5), e = lane & 31;
    if (hv < n_head + n_kv) {
        const int kh = hv - n_head;
        int8_t* Kq = kv.kq + kv.q_off(page, layer, kh);
        uint16_t* Ks = kv.ks + kv.s_off(page, layer, kh);
        Kq[(b1 * 64 + ps) * 32 + e] = (int8_t)q1;
        Kq[(b2 * 64 + ps) * 32 + e] = (int8_t)q2;
        if (e == 0) { Ks[b1 * 64 + ps] = f2h(d1); Ks[b2 * 64 + ps] = f2h(d2); }
    } else {
        const int vh = hv - n_head - n_kv;
        int8_t* Vq = kv.vq + kv.q_off(page, layer, vh);
        uint16_t* Vs = kv.vs + kv.s_off(page, layer, vh);
        Vq[ps * 128 + lane] = (int8_t)q1;
        Vq[ps * 128 + 64 + lane] = (int8_t)q2;
        if (e == 0) { Vs[ps * 4 + b1] = f2h(d1); Vs[ps * 4 + b2] = f2h(d2); }
    }
}

static void check_grp(int n_head, int n_kv) {
    Q3_CHECK(n_kv >= 1 && n_head % n_kv == 0, "n_head must be a multiple of n_kv");
    const int grp = n_head / n_kv;
    Q3_CHECK(grp == 1 || grp == 2 || grp == 4 || grp == 8, "the Q8_0 KV attention serves 1, 2, 4 or 8 query heads per kv head");
}

void launch_qk_rope_append_q8(hipStream_t st, const QkvRows& qkv, int n_head, int n_kv, const float* q_norm_w, const float* k_norm_w, float eps,
                              const float* rope_cos, const float* rope_sin, int n_ctx, const int32_t* mrope_sec, const TokMeta& tm,
                              const KvCacheQ8& kv, int layer, float* qrot, int ntok) {
    hipLaunchKernelGGL(k_qk_rope_append_q8, dim3(n_head + 2 * n_kv, ntok), dim3(64), 0, st, qkv, n_head, n_kv, q_norm_w, k_norm_w, eps, rope_cos,
                       rope_sin, n_ctx, mrope_sec, tm, kv, layer, qrot);
}

// (float) of byte i of a word of four int8
template <int I> __device__ __forceinline__ float sb2f(uint32_t w) { return (float)((int32_t)(w << (24 - 8 * I)) >> 24); }

// =====================================================================================================
// Workgroup = 4 waves per (kv head, token), all GRP query heads of the kv head.
//   query   the GRP rotated f32 rows are quantised (S2) by the workgroup into LDS: 128 B of quants and four f32-of-f16 scales per head
//   QK      wave w scores positions c0 + 64w + lane of each 256-chunk for every head: per block of 32 dims one exact int32 dot
//           (8 v_dot4_i32_i8 against the head's quants, read from LDS at a wave-uniform address) and one fma of the block term
//   PV      S7's 16 chains: the wave owns chains 4w + lane/16, lane%16 owns 8 dims -- inside one block of 32, so p_j * dv is formed once
//           per position and head and multiplies the 8 converted bytes
//   merge   wave w owns heads w and w + 4: chunk sums, M / L rescale, output row and its S2 quantisation; lane l holds dims l and l + 64
// Every global load of a chunk depends on the page table alone and is issued before the chunk's first barrier: the q rows, the wave's K
// rows and scales and all of its V batches (int8 rows are half the registers of f16 ones, so they can wait under the score chain).  No load sits behind an
// exec-mask branch: a position past the token's last one is clamped to that one -- the address, so nothing the token may not see is read -- and
// zeroed by a select.  One straight-line instance of the chunk per batch count, as k_attention.  Barriers wait for LDS only.
// =====================================================================================================
template <int GRP>
__global__ void __launch_bounds__(256) k_attention_q8kv(const float* __restrict__ qrot, int n_head, TokMeta tm, KvCacheQ8 kv, int layer,
                                                        float* __restrict__ att, int8_t* __restrict__ aq, uint16_t* __restrict__ ad) {
    constexpr int HPW = (GRP + 3) / 4;   // heads a wave merges
    __shared__ __attribute__((aligned(16))) uint32_t qq_s[GRP][32];
    __shared__ float qe_s[GRP][4];
    __shared__ float p_s[GRP][256];
    __shared__ float red_s[GRP][4][128];
    __shared__ float wmax_s[GRP][4];
    const int kvh = blockIdx.x, tok = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int seq = tm.seq_of(tok), n = tm.slot_of(tok) + 1;
    const int jj = lane >> 4, dc = lane & 15;
    typedef const int32_t __attribute__((address_space(4))) * const_i32_ptr;
    const const_i32_ptr ptab = (const_i32_ptr)(uintptr_t)kv.page_table;
    auto page_of = [&](int logical) { return kv.page_table ? ptab[(size_t)seq * kv.max_pages + logical] : seq; };
    const size_t hq = kv.q_off(0, layer, kvh), hs = kv.s_off(0, layer, kvh);
    // the query rows: thread t holds element t % 128 of heads t / 128, t / 128 + 2, ... (a head past the group is clamped, and not stored)
    float qx[(GRP + 1) / 2];
#pragma unroll
    for (int i = 0; i < (GRP + 1) / 2; i++) {
        const int g = 2 * i + (tid >> 7);
        qx[i] = qrot[((size_t)tok * n_head + (size_t)kvh * GRP + (g < GRP ? g : GRP - 1)) * 128 + (tid & 127)];
    }
    const float scale = 0.08838834764831845f;
    float M[HPW], L[HPW], O[HPW][2];
#pragma unroll
    for (int k = 0; k < HPW; k++) { M[k] = 0.0f; L[k] = 0.0f; O[k][0] = 0.0f; O[k][1] = 0.0f; }
    for (int c0 = 0; c0 < n; c0 += 256) {
        const int cn = (n - c0) < 256 ? (n - c0) : 256;
        const int jbase = c0 + wave * 64;
        float S[GRP][8];
        auto chunk = [&](auto nb_const) {
            constexpr int NB = decltype(nb_const)::value;
            uint2 vq[4 * NB];
            uint32_t vsc[4 * NB];
            int pg[NB];
#pragma unroll
            for (int b = 0; b < NB; b++) pg[b] = page_of((c0 >> 6) + b);
            auto load_v = [&](int b) {   // batch b = the 64 positions of one page: every lane loads, a row past n - 1 is clamped (same page)
                const int8_t* Vq = kv.vq + (size_t)pg[b] * kv.page_q + hq;
                const uint16_t* Vs = kv.vs + (size_t)pg[b] * kv.page_s + hs;
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) {
                    const int jg = c0 + 64 * b + 16 * g4 + 4 * wave + jj;
                    const int jc = (jg < n ? jg : n - 1) & 63;
                    vq[4 * b + g4] = *reinterpret_cast<const uint2*>(Vq + jc * 128 + dc * 8);
                    vsc[4 * b + g4] = Vs[jc * 4 + (dc >> 2)];
                }
            };
            auto load_all_v = [&]() {
#pragma unroll
                for (int b = 0; b < NB; b++) load_v(b);
            };
            auto q_handoff = [&]() {   // first chunk: the q rows arrive while the chunk's K and V rows are on their way
                if (c0 == 0) {
#pragma unroll
                    for (int i = 0; i < (GRP + 1) / 2; i++) {
                        const int g = 2 * i + (tid >> 7);
                        float d;
                        const int q = quant1(qx[i], amax32(q3_fabsf(qx[i])), &d);
                        if (g < GRP) {
                            reinterpret_cast<int8_t*>(&qq_s[g][0])[tid & 127] = (int8_t)q;
                            if ((lane & 31) == 0) qe_s[g][(tid & 127) >> 5] = h2f(f2h(d));
                        }
                    }
                    wg_barrier_lds();
                }
            };
            const bool valid = (jbase + lane) < n;
            float s[GRP];
            if (jbase < n) {   // the wave's 64 positions are one page
                int pgk = pg[0];
#pragma unroll
                for (int b = 1; b < NB; b++) pgk = wave == b ? pg[b] : pgk;
                const int jl = (valid ? jbase + lane : n - 1) & 63;
                const int8_t* Kq = kv.kq + (size_t)pgk * kv.page_q + hq;
                const uint16_t* Ks = kv.ks + (size_t)pgk * kv.page_s + hs;
                uint4 kreg[8];
                uint32_t ksc[4];
#pragma unroll
                for (int b = 0; b < 4; b++) {
                    kreg[2 * b] = *reinterpret_cast<const uint4*>(Kq + (b * 64 + jl) * 32);
                    kreg[2 * b + 1] = *reinterpret_cast<const uint4*>(Kq + (b * 64 + jl) * 32 + 16);
                    ksc[b] = Ks[b * 64 + jl];
                }
                load_all_v();
                q_handoff();
#pragma unroll
                for (int g = 0; g < GRP; g++) {
                    float acc = 0.0f;
#pragma unroll
                    for (int b = 0; b < 4; b++) {
                        const uint4 qa = *reinterpret_cast<const uint4*>(&qq_s[g][8 * b]), qb = *reinterpret_cast<const uint4*>(&qq_s[g][8 * b + 4]);
                        const int I = dot16(qa, kreg[2 * b]) + dot16(qb, kreg[2 * b + 1]);
                        const float ed = qe_s[g][b] * h2f(ksc[b]);
                        acc = q3_fmaf((float)I, ed, acc);
                    }
                    s[g] = valid ? acc * scale : -INFINITY;
                }
            } else {
                load_all_v();
                q_handoff();
#pragma unroll
                for (int g = 0; g < GRP; g++) s[g] = -INFINITY;
            }
#pragma unroll
            for (int g = 0; g < GRP; g++) {
                const float wm = wave_max_bfly(s[g]);
                if (lane == 0) wmax_s[g][wave] = wm;
            }
            wg_barrier_lds();
#pragma unroll
            for (int g = 0; g < GRP; g++) {
                const float mc = fmaxf(fmaxf(wmax_s[g][0], wmax_s[g][1]), fmaxf(wmax_s[g][2], wmax_s[g][3]));
                p_s[g][wave * 64 + lane] = valid ? q3_expf(s[g] - mc) : 0.0f;
            }
            wg_barrier_lds();
#pragma unroll
            for (int g = 0; g < GRP; g++)
#pragma unroll
                for (int i = 0; i < 8; i++) S[g][i] = 0.0f;
#pragma unroll
            for (int u = 0; u < 4 * NB; u++) {
                if (16 * u < cn) {
                    const int jl = 16 * u + 4 * wave + jj;
                    const bool ok = (c0 + jl) < n;
                    const uint32_t lo = ok ? vq[u].x : 0u, hi = ok ? vq[u].y : 0u;   // (selects: the loads above were of a clamped row)
                    const float dv = ok ? h2f(vsc[u]) : 0.0f;
                    const float f[8] = { sb2f<0>(lo), sb2f<1>(lo), sb2f<2>(lo), sb2f<3>(lo), sb2f<0>(hi), sb2f<1>(hi), sb2f<2>(hi), sb2f<3>(hi) };
#pragma unroll
                    for (int g = 0; g < GRP; g++) {
                        const float w = p_s[g][jl] * dv;
#pragma unroll
                        for (int i = 0; i < 8; i++) S[g][i] = q3_fmaf(w, f[i], S[g][i]);
                    }
                }
            }
        };
        if (cn <= 64) chunk(std::integral_constant<int, 1>());
        else if (cn <= 128) chunk(std::integral_constant<int, 2>());
        else if (cn <= 192) chunk(std::integral_constant<int, 3>());
        else chunk(std::integral_constant<int, 4>());
#pragma unroll
        for (int g = 0; g < GRP; g++)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const float a = S[g][i] + xor_lane<16>(S[g][i]);   // (S0+S1) | (S2+S3)
                const float T = a + xor_lane<32>(a);                // (S0+S1)+(S2+S3)
                if (jj == 0) red_s[g][wave][dc * 8 + i] = T;
            }
        wg_barrier_lds();
#pragma unroll
        for (int k = 0; k < HPW; k++) {
            const int g = wave + 4 * k;
            if (g < GRP) {
                const float mc = fmaxf(fmaxf(wmax_s[g][0], wmax_s[g][1]), fmaxf(wmax_s[g][2], wmax_s[g][3]));
                float a = p_s[g][lane];
                a = a + p_s[g][lane + 64]; a = a + p_s[g][lane + 128]; a = a + p_s[g][lane + 192];
                const float lc = wave_sum_bfly(a);
                float oc[2];
#pragma unroll
                for (int e = 0; e < 2; e++) {
                    const int d = lane + 64 * e;
                    oc[e] = (red_s[g][0][d] + red_s[g][1][d]) + (red_s[g][2][d] + red_s[g][3][d]);
                }
                if (c0 == 0) {
                    M[k] = mc; L[k] = lc; O[k][0] = oc[0]; O[k][1] = oc[1];
                } else {
                    const float mn = fmaxf(M[k], mc);
                    const float ea = q3_expf(M[k] - mn), eb = q3_expf(mc - mn);
                    const float t = lc * eb;
                    L[k] = q3_fmaf(L[k], ea, t);
#pragma unroll
                    for (int e = 0; e < 2; e++) { const float u2 = oc[e] * eb; O[k][e] = q3_fmaf(O[k][e], ea, u2); }
                    M[k] = mn;
                }
            }
        }
        wg_barrier_lds();
    }
#pragma unroll
    for (int k = 0; k < HPW; k++) {
        const int g = wave + 4 * k;
        if (g < GRP) {
            const size_t o = ((size_t)tok * n_head + (size_t)kvh * GRP + g) * 128;
#pragma unroll
            for (int e = 0; e < 2; e++) {
                const float y = O[k][e] / L[k];
                float d;
                const int q = quant1(y, amax32(q3_fabsf(y)), &d);
                if (att) att[o + 64 * e + lane] = y;
                aq[o + 64 * e + lane] = (int8_t)q;
                if ((lane & 31) == 0) ad[(o >> 5) + 2 * e + (lane >> 5)] = f2h(d);
            }
        }
    }
}

void launch_attention_q8kv(hipStream_t st, const float* qrot, int n_head, int n_kv, const TokMeta& tm, const KvCacheQ8& kv, int layer, float* att,
                           int8_t* aq, uint16_t* ad, int ntok) {
    check_grp(n_head, n_kv);
    const dim3 grid(n_kv, ntok), block(256);
    switch (n_head / n_kv) {
    case 1: hipLaunchKernelGGL(k_attention_q8kv<1>, grid, block, 0, st, qrot, n_head, tm, kv, layer, att, aq, ad); break;
    case 2: hipLaunchKernelGGL(k_attention_q8kv<2>, grid, block, 0, st, qrot, n_head, tm, kv, layer, att, aq, ad); break;
    case 4: hipLaunchKernelGGL(k_attention_q8kv<4>, grid, block, 0, st, qrot, n_head, tm, kv, layer, att, aq, ad); break;
    default: hipLaunchKernelGGL(k_attention_q8kv<8>, grid, block, 0, st, qrot, n_head, tm, kv, layer, att, aq, ad); break;
    }
}

// host only: bytes of one plane page (K or V of 64 positions, every layer and kv head, padded to 16 KiB) and of one token in both planes
void kv_layout(int n_layer, int n_kv, int kv_type, size_t* bytes_per_token, size_t* plane_page_bytes) {
    Q3_CHECK(n_layer >= 1 && n_kv >= 1, "bad n_layer / n_kv");
    Q3_CHECK(kv_type == KV_F16 || kv_type == KV_Q8_0, "unknown KV cache type (1 = F16, 8 = Q8_0)");
    const size_t unit = kv_type == KV_F16 ? 16384 : KVQ8_UNIT;
    const size_t page = ((size_t)n_layer * n_kv * unit + 16383) / 16384 * 16384;
    if (plane_page_bytes) *plane_page_bytes = page;
    if (bytes_per_token) *bytes_per_token = 2 * page / 64;
}

} // namespace q3
