// logprob.hip -- [EXT] token log-probabilities (q3tts_spec.h "token log-probabilities"): k_logprob_rows reads raw f32 logits rows and
// writes log softmax(row)[chosen] (and optionally log softmax(row)[extra_idx]) per row.  One 256-lane workgroup per (row, head): a row of at
// most 4096 logits is read ONCE, as up to four 16-byte loads per lane when its base is 16-byte aligned (the talker's rows at tl_stride_, the
// predictor's 2048-wide slices) with a scalar tail for n % 4, or as strided scalar loads when it is not; max and sum are reduced across the
// lanes of a wave by xor butterflies and across the four waves through LDS.  No atomics, no scratch, no global workspace.
//
// In the frame graph one launch covers the 15 predictor heads (logits slices [15][B][2048], codes keys[b][1..15], columns 1..15 of row
// n_frames[b]) and the talker head (d_tlogits_, code next_key0[b], columns 0 and 16 of row n_frames[b] + 1); it runs between the talker's
// sampler and k_advance_keys and reads the slot table as k_stall_save does: idle, finished, stalled and non-recording slots write nothing.
#include "kernels.h"
#include "kdev.h"
#include "q3_common.h"

namespace q3 {

#define LP_THREADS 256
#define LP_MAX_N 4096
#define LP_VEC (LP_MAX_N / 4 / LP_THREADS) // float4 loads per lane on the aligned path
#define LP_SCAL (LP_MAX_N / LP_THREADS)    // scalar loads per lane on the unaligned path

__device__ __forceinline__ float lp_max4(float m, const float4& v) { return fmaxf(fmaxf(m, fmaxf(v.x, v.y)), fmaxf(v.z, v.w)); }
// e^(x - m) terms of one lane's elements; a padding element is -inf: q3_expf(-inf) = 0
__device__ __forceinline__ float lp_sum4(float s, const float4& v, float m) {
    s = s + q3_expf(v.x - m); s = s + q3_expf(v.y - m); s = s + q3_expf(v.z - m); s = s + q3_expf(v.w - m);
    return s;
}
// lp = (x_c - m) - logf(s): never positive (a rounding residue is clamped); an -inf logit gives -inf
__device__ __forceinline__ float lp_value(float xc, float m, float logs) {
    if (xc == -INFINITY) return -INFINITY;
    const float lp = (xc - m) - logs;
    return lp > 0.0f ? 0.0f : lp;
}

__global__ void __launch_bounds__(LP_THREADS) k_logprob_rows(LogprobArgs a) {
    __shared__ float red_m[LP_THREADS / 64], red_s[LP_THREADS / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const bool second = (int)blockIdx.y >= a.n_first; // uniform: the launch's last head may be of another shape (the talker's)
    const int head = second ? 0 : (int)blockIdx.y;
    // plain selects of argument fields (selecting a struct would make the compiler index a scratch copy of the arguments)
    const float* logits = second ? a.t.logits : a.p.logits;
    const int stride = second ? a.t.stride : a.p.stride;
    const size_t head_stride = second ? 0 : a.p.head_stride;
    const int n = second ? a.t.n : a.p.n;
    const u64* key = second ? a.t.key : a.p.key;
    const int key_stride = second ? a.t.key_stride : a.p.key_stride;
    const int32_t* chosen = second ? a.t.chosen : a.p.chosen;
    const int extra_idx = second ? a.t.extra_idx : a.p.extra_idx;
    const int col = second ? a.t.col : a.p.col + head;
    const int col_extra = second ? a.t.col_extra : a.p.col_extra;
    const int row_ahead = second ? a.t.row_ahead : a.p.row_ahead;

    float* out;
    if (a.n_frames) { // engine form: the slot table decides whether and where slot b writes
        const int f = a.n_frames[b];
        const bool live = !a.finished[b] && f < a.max_frames[b];
        const bool waits = live && a.open[b] && f >= a.n_trail[b]; // a stalled frame is discarded: it leaves no trace
        const int row = f + row_ahead;
        if (!live || waits || !a.record[b] || row >= a.out_rows) return;
        out = a.out + ((size_t)b * a.out_rows + row) * a.out_stride;
    } else out = a.out + (size_t)b * a.out_stride;

    const float* lg = logits + (size_t)head * head_stride + (size_t)b * stride;
    const int c = chosen ? chosen[b] : key_code(key[(size_t)b * key_stride + head]);
    float m = -INFINITY, s = 0.0f;
    if ((reinterpret_cast<uintptr_t>(lg) & 15u) == 0) {
        const float4* lg4 = reinterpret_cast<const float4*>(lg);
        const int nv = n >> 2;
        float4 v[LP_VEC];
#pragma unroll
        for (int j = 0; j < LP_VEC; j++) {
            const int i = tid + j * LP_THREADS;
            v[j] = i < nv ? lg4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
        const int it = (nv << 2) + tid; // the n % 4 tail: lanes 0..2
        const float tail = (tid < 3 && it < n) ? lg[it] : -INFINITY;
#pragma unroll
        for (int j = 0; j < LP_VEC; j++) m = lp_max4(m, v[j]);
        m = fmaxf(m, tail);
        m = wave_max_bfly(m);
        if (lane == 0) red_m[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        if (m != -INFINITY) { // uniform; an all -inf row has no finite entry to report
#pragma unroll
            for (int j = 0; j < LP_VEC; j++) s = lp_sum4(s, v[j], m);
            s = s + q3_expf(tail - m);
        }
    } else {
        float x[LP_SCAL];
#pragma unroll
        for (int j = 0; j < LP_SCAL; j++) {
            const int i = tid + j * LP_THREADS;
            x[j] = i < n ? lg[i] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < LP_SCAL; j++) m = fmaxf(m, x[j]);
        m = wave_max_bfly(m);
        if (lane == 0) red_m[wave] = m;
        __syncthreads();
        m = fmaxf(fmaxf(red_m[0], red_m[1]), fmaxf(red_m[2], red_m[3]));
        if (m != -INFINITY) {
#pragma unroll
            for (int j = 0; j < LP_SCAL; j++) s = s + q3_expf(x[j] - m);
        }
    }
    s = wave_sum_bfly(s);
    if (lane == 0) red_s[wave] = s;
    __syncthreads();
    if (tid != 0) return;
    s = (red_s[0] + red_s[1]) + (red_s[2] + red_s[3]);
    const float logs = logf(s);
    // a code outside the row (a key that was never drawn) has no probability: the "not computed" mark
    out[col] = (c >= 0 && c < n) ? lp_value(lg[c], m, logs) : Q3_LOGPROB_NONE;
    if (extra_idx >= 0 && col_extra >= 0) out[col_extra] = extra_idx < n ? lp_value(lg[extra_idx], m, logs) : Q3_LOGPROB_NONE;
}

void launch_logprob_rows(hipStream_t st, const LogprobArgs& a, int B) {
    Q3_CHECK(B >= 1 && a.n_first >= 0 && a.n_first + (a.t.logits ? 1 : 0) >= 1, "nothing to launch");
    Q3_CHECK(a.n_first == 0 || (a.p.logits && a.p.n >= 1 && a.p.n <= LP_MAX_N && a.p.n <= a.p.stride && (a.p.chosen || a.p.key)), "bad first head group");
    Q3_CHECK(!a.t.logits || (a.t.n >= 1 && a.t.n <= LP_MAX_N && a.t.n <= a.t.stride && (a.t.chosen || a.t.key)), "bad last head");
    Q3_CHECK(a.out && (!a.n_frames || (a.finished && a.max_frames && a.open && a.n_trail && a.record && a.out_rows >= 1)), "bad output arguments");
    hipLaunchKernelGGL(k_logprob_rows, dim3(B, a.n_first + (a.t.logits ? 1 : 0)), dim3(LP_THREADS), 0, st, a);
}

} // namespace q3
