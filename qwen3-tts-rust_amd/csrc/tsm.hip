// tsm.hip -- [EXT] speaking rate (q3tts_spec.h "speaking rate"): WSOLA time-scale change behind the codec, one launch per decode pass that has
// a stretching stream.
//
// k_tsm_stretch: grid = G, 512 lanes, one workgroup per stream; a stream that is not stretched exits at once.  The frames of a stream are
// sequential (t_k depends on d_{k-1}), so the workgroup walks them.  Per frame it loads x[a_k - 720 .. a_k + 1200) into LDS -- 1920 floats
// whatever the chunk length, from the chunk, from the stream's history below the chunk's first sample, zeros outside [0, N) -- which holds
// every candidate, the template and both output terms.  Lane `tid` < 481 is candidate d = tid - 240 and runs the 480-term chain: consecutive
// lanes read consecutive LDS words (no bank conflict), the template word is the same for all lanes (a broadcast).  The (SSD bits << 32 | o)
// keys are reduced by xor shuffles inside a wave and through 8 LDS words across waves.  Lanes < 480 then form the output hop into LDS, from
// where it leaves as 16-byte vectors (4 floats or 8 int16); the launcher refuses a destination that is not 16-byte aligned, which the
// engine's staging and the codec's buffers never are (a hop is 1920 or 960 bytes).
//
// State: hist [n_streams][1920] and d_prev [n_streams], updated in place by the stream's only workgroup behind a barrier, after its last
// read.  The counters (samples seen, frames made) are data-independent and live on the host; the launch's meta entry carries them.
// No atomics, no scratch, no global workspace; the barriers inside the frame loop wait for LDS only.
#include "kernels.h"
#include "kdev.h"
#include "tsm.h"

namespace q3 {

#define TS_THREADS 512
#define TS_WAVES (TS_THREADS / 64)
#define TS_CAND (2 * Q3_TSM_SEARCH + 1)
#define TS_BACK (Q3_TSM_HIST - Q3_TSM_LOOK)            // 720: how far below a_k a frame reaches
#define TS_RING 64

__device__ __forceinline__ float ts_clamp(float y) { return y < -1.0f ? -1.0f : (y > 1.0f ? 1.0f : y); }
__device__ __forceinline__ uint32_t ts_s16(float y) { return (uint32_t)(uint16_t)(int16_t)rintf(y * 32767.0f); }

struct TsmArgs { const float* in; int T; const TsmStreamMeta* meta; const float* tabs; float* hist; int32_t* d_prev; unsigned char* out; int32_t* trace; };

__global__ void __launch_bounds__(TS_THREADS) k_tsm_stretch(TsmArgs a) {
    __shared__ __attribute__((aligned(16))) float win[Q3_TSM_HIST];
    __shared__ __attribute__((aligned(16))) float wt[2 * Q3_TSM_HOP];
    __shared__ __attribute__((aligned(16))) float stage[Q3_TSM_HOP];
    __shared__ unsigned long long best[TS_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x;
    const TsmStreamMeta mt = a.meta[g];
    if (mt.enc < 0) return;   // uniform: the stream is not stretched
    const float* __restrict__ x = a.in + (size_t)g * a.T;
    float* const h = a.hist + (size_t)mt.slot * Q3_TSM_HIST;
    const long long n_prev = mt.n_prev, n_new = mt.n_prev + a.T, step = (long long)Q3_TSM_HOP * mt.pct;
    for (int i = tid; i < 2 * Q3_TSM_HOP; i += TS_THREADS) wt[i] = a.tabs[i];
    int d_prev = a.d_prev[mt.slot];
    unsigned char* const ob = a.out + mt.out_off;   // 16-byte aligned (the launcher saw to it), and so is every hop: 1920 or 960 bytes
    for (int f = 0; f < mt.n_frames; f++) {
        const long long k = mt.k0 + f, ak = k * step / 100;
        const long long tk = k == 0 ? 0 : (k - 1) * step / 100 + d_prev + Q3_TSM_HOP;
        const long long base = ak - TS_BACK;
        for (int i = tid; i < Q3_TSM_HIST; i += TS_THREADS) {
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
        if (tid < TS_CAND && ak + tid - Q3_TSM_SEARCH >= 0) {
            const float* __restrict__ c = win + (TS_BACK - Q3_TSM_SEARCH) + tid;
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
        for (int w = 1; w < TS_WAVES; w++) kmin = best[w] < kmin ? best[w] : kmin;
        const int d = tsm_offset_of_order((int)(unsigned)(kmin & 0xffffffffull));   // uniform, in [-240, 240]
        if (tid < Q3_TSM_HOP) stage[tid] = ts_clamp(fmaf(wt[tid], win[TS_BACK + d + tid], __fmul_rn(wt[Q3_TSM_HOP + tid], win[tb + tid])));
        wg_barrier_lds();
        if (mt.enc == Q3_PCM_S16) {
            uint16_t* o = reinterpret_cast<uint16_t*>(ob) + (size_t)f * Q3_TSM_HOP;
            if (tid < Q3_TSM_HOP / 8) {
                const float4 lo = reinterpret_cast<const float4*>(stage)[2 * tid], hi = reinterpret_cast<const float4*>(stage)[2 * tid + 1];
                uint4 w;
                w.x = ts_s16(lo.x) | (ts_s16(lo.y) << 16); w.y = ts_s16(lo.z) | (ts_s16(lo.w) << 16);
                w.z = ts_s16(hi.x) | (ts_s16(hi.y) << 16); w.w = ts_s16(hi.z) | (ts_s16(hi.w) << 16);
                reinterpret_cast<uint4*>(o)[tid] = w;
            }
        } else {
            float* o = reinterpret_cast<float*>(ob) + (size_t)f * Q3_TSM_HOP;
            if (tid < Q3_TSM_HOP / 4) reinterpret_cast<float4*>(o)[tid] = reinterpret_cast<const float4*>(stage)[tid];
        }
        if (tid == 0 && a.trace) a.trace[mt.trace_off + f] = d;
        d_prev = d;
        // the next frame's window and keys are written behind barriers that follow every read of this frame's
    }
    __syncthreads();   // every read of the history is done: the stream's only workgroup replaces it
    if (a.T >= Q3_TSM_HIST) for (int i = tid; i < Q3_TSM_HIST; i += TS_THREADS) h[i] = x[a.T - Q3_TSM_HIST + i];
    if (tid == 0) a.d_prev[mt.slot] = d_prev;
}

TsmStretcher::TsmStretcher(int n_streams_, int max_group_) : n_streams(n_streams_), max_group(max_group_) {
    Q3_CHECK(n_streams >= 1 && max_group >= 1, "bad stretcher shape");
    std::vector<float> t(2 * Q3_TSM_HOP);
    tsm_windows(t.data(), t.data() + Q3_TSM_HOP);
    tabs.alloc(t.size()); tabs.upload(t.data(), t.size());
    hist_own.alloc((size_t)n_streams * Q3_TSM_HIST); hist_own.zero();
    hist = hist_own.p;
    d_prev.alloc((size_t)n_streams); d_prev.zero();
    Q3_HIP(hipStreamSynchronize(nullptr)); // the memsets ran on the null stream, which the caller's non-blocking streams do not wait for
    d_ring.alloc((size_t)TS_RING * max_group);
    Q3_HIP(hipHostMalloc((void**)&h_ring, sizeof(TsmStreamMeta) * TS_RING * max_group));
    n_seen.assign((size_t)n_streams, 0); k_done.assign((size_t)n_streams, 0);
    ring_ev.resize(TS_RING); ring_used.assign(TS_RING, 0);
    for (auto& e : ring_ev) Q3_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
}
TsmStretcher::~TsmStretcher() {
    for (auto e : ring_ev) if (e) (void)hipEventDestroy(e);
    if (h_ring) (void)hipHostFree(h_ring);
}

void TsmStretcher::reset_async(hipStream_t st, int slot) {
    Q3_CHECK(slot >= 0 && slot < n_streams, "stream out of range");
    Q3_HIP(hipMemsetAsync(hist + (size_t)slot * Q3_TSM_HIST, 0, sizeof(float) * Q3_TSM_HIST, st));
    Q3_HIP(hipMemsetAsync(d_prev.p + slot, 0, sizeof(int32_t), st));
    n_seen[(size_t)slot] = 0; k_done[(size_t)slot] = 0;
}

void launch_tsm_stretch(hipStream_t st, TsmStretcher& s, const float* in, int G, int T, bool flush, const int32_t* streams, const int32_t* pct,
                        const int32_t* enc, void* out, const int64_t* out_off, int64_t* n_out, int32_t* trace, const int64_t* trace_off) {
    if (const char* why = tsm_launch_refusal(G, s.max_group, T, flush, streams, s.n_streams, pct, enc)) throw Error(std::string("tsm stretch: ") + why);
    Q3_CHECK((in || T == 0) && out && out_off && n_out && (!trace || trace_off), "bad buffers");
    bool any = false;
    for (int g = 0; g < G; g++) {   // the last of the checks: nothing of the stretcher has changed yet
        if (pct[g] == 100) continue;
        any = true;
        const uintptr_t dst = reinterpret_cast<uintptr_t>(out) + (uintptr_t)out_off[g];
        Q3_CHECK(out_off[g] >= 0 && (dst & 15u) == 0, "misaligned output");   // the hops leave as 16-byte vectors
    }
    for (int g = 0; g < G; g++) if (pct[g] == 100) n_out[g] = T;
    if (!any) return;   // no stream is stretched: nothing to run
    const int rs = s.ring_idx;   // the slot's previous launch, on whichever stream it ran, has consumed its upload
    s.ring_idx = (s.ring_idx + 1) % TS_RING;
    if (s.ring_used[(size_t)rs]) Q3_HIP(hipEventSynchronize(s.ring_ev[(size_t)rs]));
    const size_t slot0 = (size_t)rs * s.max_group;
    TsmStreamMeta* hm = s.h_ring + slot0;
    for (int g = 0; g < G; g++) {
        TsmStreamMeta& m = hm[g];
        m.enc = pct[g] == 100 ? -1 : enc[g];
        m.slot = streams[g]; m.pct = pct[g]; m.n_frames = 0; m.n_prev = 0; m.k0 = 0;
        m.out_off = out_off[g]; m.trace_off = trace ? trace_off[g] : 0;
        if (m.enc < 0) continue;
        int64_t& seen = s.n_seen[(size_t)streams[g]]; int64_t& done = s.k_done[(size_t)streams[g]];
        const int64_t total = tsm_frames(pct[g], seen + T, flush);
        m.n_prev = seen; m.k0 = done; m.n_frames = (int32_t)std::max<int64_t>(total - done, 0);
        seen += T; done += m.n_frames;
        n_out[g] = (int64_t)m.n_frames * Q3_TSM_HOP;
        s.chunks += T > 0; s.frames_out += m.n_frames; s.flushes += flush;
    }
    Q3_HIP(hipMemcpyAsync(s.d_ring.p + slot0, hm, sizeof(TsmStreamMeta) * G, hipMemcpyHostToDevice, st));
    TsmArgs a{in, T, s.d_ring.p + slot0, s.tabs.p, s.hist, s.d_prev.p, (unsigned char*)out, trace};
    hipLaunchKernelGGL(k_tsm_stretch, dim3((unsigned)G), dim3(TS_THREADS), 0, st, a);
    Q3_HIP(hipEventRecord(s.ring_ev[(size_t)rs], st));
    s.ring_used[(size_t)rs] = 1;
}

} // namespace q3
