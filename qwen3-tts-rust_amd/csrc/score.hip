// score.hip -- [EXT] scoring given frames (q3tts_spec.h "scoring"): the two kernels of a teacher-forced predictor pass over F frames.
//
// k_score_inputs builds the pass's predictor input, position-major: token p * F + f is position p of frame f.  Position 0 is the projected
// hidden row of the frame's talker row (k_project_mt made it, as in the frame graph); position p >= 1 is row codes[f][p - 1] of the
// pre-projected table P_{p-1}, under k_gather_rows_keys' rule for a code outside the table (negative: row 0; past the end: a zero row).
// Rows move as 16-byte vectors (the projection width is a multiple of 16 floats).
//
// k_score_rows writes the 17 columns of F frames in one launch, one 256-lane workgroup per (frame, head): heads 0..14 read the predictor's
// 2048-wide logits slices and give columns 1..15, head 15 reads the talker's row and gives columns 0 and 16.  The arithmetic is
// k_logprob_rows': a row is read once, as 16-byte loads with a scalar tail when its base is 16-byte aligned or as strided scalar loads when
// it is not, max and sum go through xor butterflies inside a wave and through LDS across the four waves in the same order, q3_expf.
// No atomics, no scratch, no global workspace.
#include "kernels.h"
#include "kdev.h"
#include "q3_common.h"

namespace q3 {

#define SC_THREADS 256
#define SC_MAX_N 4096
#define SC_VEC (SC_MAX_N / 4 / SC_THREADS)
#define SC_SCAL (SC_MAX_N / SC_THREADS)

__device__ __forceinline__ float sc_max4(float m, const float4& v) { return fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float sc_sum4(float s, const float4& v, float m) {
    s = s + q3_expf(v.x - m); s = s + q3_expf(v.y - m); s = s + q3_expf(v.z - m); s = s + q3_expf(v.w - m);
    return s;
}
__device__ __forceinline__ float sc_value(float xc, float m, float logs) {
    if (xc == -INFINITY) return -INFINITY;
    const float lp = (xc - m) - logs;
    return lp > 0.0f ? 0.0f : lp;
}

__global__ void __launch_bounds__(SC_THREADS) k_score_rows(ScoreRowsArgs a) {
    __shared__ float red_m[SC_THREADS / 64], red_s[SC_THREADS / 64];
    const int f = blockIdx.x, head = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool talker = head == 15; // uniform
    const float* lg = talker ? a.tlogits + (size_t)f * a.t_stride : a.plogits + (size_t)head * a.p_head_stride + (size_t)f * Q3_CODEBOOK_SIZE;
    const int n = talker ? Q3_SAMPLE_END : Q3_CODEBOOK_SIZE;
    const int c = a.codes[(size_t)f * 16 + (talker ? 0 : head + 1)];
    float m = -INFINITY, s = 0.0f;
    if ((reinterpret_cast<uintptr_t>(lg) & 15u) == 0) {
        const float4* lg4 = reinterpret_cast<const float4*>(lg);
        const int nv = n >> 2;
        float4 v[SC_VEC];
#pragma unroll
        for (int j = 0; j < SC_VEC; j++) {
            const int i = tid + j * SC_THREADS;
            v[j] = i < nv ? lg4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
        const int it = (nv << 2) + tid; // the n % 4 tail: lanes 0..2
        const float tail = (tid < 3 && it < n) ? lg[it] : -INFINITY;
#pragma unroll
        for (int j = 0; j < SC_VEC; j++) m = sc_max4(m, v[j]);
        m = fmaxf(m, tail);
        m = wave_max_bfly(m);
        if (lane == 0) red_m[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        if (m != -INFINITY) { // uniform; an all -inf row has no finite entry to report
#pragma unroll
            for (int j = 0; j < SC_VEC; j++) s = sc_sum4(s, v[j], m);
            s = s + q3_expf(tail - m);
        }
    } else {
        float x[SC_SCAL];
#pragma unroll
        for (int j = 0; j < SC_SCAL; j++) {
            const int i = tid + j * SC_THREADS;
            x[j] = i < n ? lg[i] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < SC_SCAL; j++) m = fmaxf(m, x[j]);
        m = wave_max_bfly(m);
        if (lane == 0) red_m[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        if (m != -INFINITY) {
#pragma unroll
            for (int j = 0; j < SC_SCAL; j++) s = s + q3_expf(x[j] - m);
        }
    }
    s = wave_sum_bfly(s);
    if (lane == 0) red_s[wave] = s;
    __syncthreads();
    if (tid != 0) return;
    s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const float logs = logf(s);
    float* out = a.out + (size_t)f * Q3_LOGPROB_COLS;
    // a code outside the row has no probability: the "not computed" mark (a score request's codes were range-checked at submit)
    out[talker ? 0 : head + 1] = (c >= 0 && c < n) ? sc_value(lg[c], m, logs) : Q3_LOGPROB_NONE;
    if (talker) out[Q3_LOGPROB_COLS - 1] = sc_value(lg[Q3_CODEC_EOS], m, logs);
}

void launch_score_rows(hipStream_t st, const ScoreRowsArgs& a, int F) {
    Q3_CHECK(F >= 1 && a.tlogits && a.plogits && a.codes && a.out, "bad arguments");
    Q3_CHECK(a.t_stride >= Q3_SAMPLE_END && a.p_head_stride >= (size_t)F * Q3_CODEBOOK_SIZE, "logits rows overlap");
    hipLaunchKernelGGL(k_score_rows, dim3(F, 16), dim3(SC_THREADS), 0, st, a);
}

// one float4 per lane; grid = (row vectors / 256, 16 F tokens)
__global__ void __launch_bounds__(256) k_score_inputs(const float* __restrict__ hidden_proj, const float* const* __restrict__ tabs,
                                                      const int64_t* __restrict__ tab_rows, int dP, const int32_t* __restrict__ codes, int F,
                                                      float* __restrict__ out) {
    const int tok = blockIdx.y, i4 = blockIdx.x * 256 + threadIdx.x;
    if (i4 >= (dP >> 2)) return;
    const int p = tok / F, f = tok - p * F;
    float4 v;
    if (p == 0) v = reinterpret_cast<const float4*>(hidden_proj + (size_t)f * dP)[i4];
    else {
        int c = codes[(size_t)f * 16 + (p - 1)];
        if (c < 0) c = 0;
        v = ((int64_t)c < tab_rows[p - 1]) ? reinterpret_cast<const float4*>(tabs[p - 1] + (size_t)c * dP)[i4] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    reinterpret_cast<float4*>(out + (size_t)tok * dP)[i4] = v;
}

void launch_score_inputs(hipStream_t st, const float* hidden_proj, const float* const* tabs, const int64_t* tab_rows, int dP, const int32_t* codes,
                         int F, float* out) {
    Q3_CHECK(F >= 1 && dP >= 4 && dP % 4 == 0, "bad arguments");
    Q3_CHECK(((reinterpret_cast<uintptr_t>(hidden_proj) | reinterpret_cast<uintptr_t>(out)) & 15u) == 0, "rows must be 16-byte aligned");
    hipLaunchKernelGGL(k_score_inputs, dim3((dP / 4 + 255) / 256, 16 * F), dim3(256), 0, st, hidden_proj, tabs, tab_rows, dP, codes, F, out);
}

} // namespace q3
