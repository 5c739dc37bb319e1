// wsola.h -- device code the three output stages share (pcmout.hip, tsm.hip, pitch.hip): the clamp, the int16 rounding and the packing of 8
// samples into one 16-byte store, and the WSOLA frame step of the speaking rate (q3tts_spec.h "speaking rate"), which the pitch shifter's
// stage 1 is at another tempo.
//
// wsola_frame, per frame and by all WS_THREADS lanes of the stream's only workgroup: x[a_k - 720 .. a_k + 1200) goes into LDS -- 1920 floats
// whatever the chunk length, from the chunk, from the stream's history below the chunk's first sample, zeros outside [0, N) -- which holds
// every candidate, the template and both output terms.  Lane `tid` < 481 is candidate d = tid - 240 and runs the 480-term chain: consecutive
// lanes read consecutive LDS words (no bank conflict), the template word is the same for all lanes (a broadcast).  The (SSD bits << 32 | o)
// keys are reduced by xor shuffles inside a wave and through 8 LDS words across waves.  Lanes < 480 then form the output hop in LDS, where
// the caller wants it.  The callers work out a_k and t_k: the stretcher divides by the constant 100, the shifter by its P.
#pragma once
#include "kdev.h"
#include "tsm.h"

namespace q3 {

#define WS_THREADS 512
#define WS_WAVES (WS_THREADS / 64)
#define WS_CAND (2 * Q3_TSM_SEARCH + 1)
#define WS_BACK (Q3_TSM_HIST - Q3_TSM_LOOK)            // 720: how far below a_k a frame reaches

__device__ __forceinline__ float pcm_clamp(float y) { return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y); }
__device__ __forceinline__ uint32_t pcm_s16(float y) { return (uint32_t)(uint16_t)(int16_t)rintf(y * 32767.0f); }
__device__ __forceinline__ uint4 pcm_pack8(const float4 lo, const float4 hi) {
    uint4 w;
    w.x = pcm_s16(lo.x) | (pcm_s16(lo.y) << 16); w.y = pcm_s16(lo.z) | (pcm_s16(lo.w) << 16);
    w.z = pcm_s16(hi.x) | (pcm_s16(hi.y) << 16); w.w = pcm_s16(hi.z) | (pcm_s16(hi.w) << 16);
    return w;
}

// One frame: x = the chunk, samples [n_prev, n_new) of the stream; h = its history, the Q3_TSM_HIST samples below n_prev.  win [Q3_TSM_HIST],
// wt [2 * Q3_TSM_HOP] (the two window tables) and best [WS_WAVES] are the caller's LDS; the hop goes to hop [Q3_TSM_HOP], also LDS, and is
// visible to the workgroup behind the caller's next barrier.  Returns d_k, uniform, in [-240, 240].  The window and the keys of the next frame
// are written behind barriers that follow every read of this frame's
__device__ __forceinline__ int wsola_frame(long long ak, long long tk, const float* __restrict__ x, const float* h, long long n_prev, long long n_new,
                                           float* win, const float* wt, unsigned long long* best, float* hop) {
    const int tid = threadIdx.x;
    const long long base = ak - WS_BACK;
    for (int i = tid; i < Q3_TSM_HIST; i += WS_THREADS) {
        const long long n = base + i, rel = n - n_prev;
        float v = 0.0f;
        if (n >= 0 && n < n_new) {
            if (rel >= 0) v = x[rel];
            else if (rel >= -Q3_TSM_HIST) v = h[Q3_TSM_HIST + rel];
        }
        win[i] = v;
    }
    int tb = (int)(tk - base);   // in [0, 1440] by the spec's reach; clamped so that no read can leave the window
    tb = tb < 0 ? 0 : (tb > Q3_TSM_HIST - Q3_TSM_HOP ? Q3_TSM_HIST - Q3_TSM_HOP : tb);
    wg_barrier_lds();
    unsigned long long key = ~0ull;
    if (tid < WS_CAND && ak + tid - Q3_TSM_SEARCH >= 0) {
        const float* __restrict__ c = win + (WS_BACK - Q3_TSM_SEARCH) + tid;
        const float* __restrict__ t = win + tb;
        float acc = 0.0f;
#pragma unroll 16
        for (int i = 0; i < Q3_TSM_HOP; i++) {
            const float d = c[i] - t[i];
            acc = fmaf(d, d, acc);
        }
        key = ((unsigned long long)__float_as_uint(acc) << 32) | (unsigned)tsm_visit_order(tid - Q3_TSM_SEARCH);
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const unsigned long long o = __shfl_xor(key, s, 64);
        key = o < key ? o : key;
    }
    if ((tid & 63) == 0) best[tid >> 6] = key;
    wg_barrier_lds();
    unsigned long long kmin = best[0];
#pragma unroll
    for (int w = 1; w < WS_WAVES; w++) kmin = best[w] < kmin ? best[w] : kmin;
    const int d = tsm_offset_of_order((int)(unsigned)(kmin & 0xffffffffull));
    if (tid < Q3_TSM_HOP) hop[tid] = pcm_clamp(fmaf(wt[tid], win[WS_BACK + d + tid], __fmul_rn(wt[Q3_TSM_HOP + tid], win[tb + tid])));
    return d;
}

// The end of a launch's frame walk: every read of the history is done, and the stream's only workgroup replaces it with the chunk's last
// Q3_TSM_HIST samples (a flush has no chunk and leaves it) and stores the offset of its last frame
__device__ __forceinline__ void wsola_finish(const float* __restrict__ x, int T, float* h, int32_t* d_prev_of_slot, int d_prev) {
    const int tid = threadIdx.x;
    __syncthreads();
    if (T >= Q3_TSM_HIST) for (int i = tid; i < Q3_TSM_HIST; i += WS_THREADS) h[i] = x[T - Q3_TSM_HIST + i];
    if (tid == 0) *d_prev_of_slot = d_prev;
}

} // namespace q3
