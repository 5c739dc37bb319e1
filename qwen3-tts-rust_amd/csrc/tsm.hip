// tsm.hip -- [EXT] speaking rate (q3tts_spec.h "speaking rate"): WSOLA time-scale change behind the codec, one launch per decode pass that has
// a stretching stream.
//
// k_tsm_stretch: grid = G, 512 lanes, one workgroup per stream; a stream that is not stretched exits at once.  The frames of a stream are
// sequential (t_k depends on d_{k-1}), so the workgroup walks them: wsola_frame (wsola.h) per frame, with a_k = floor(k * 480 * pct / 100),
// leaves the hop in LDS, from where it goes out as 16-byte vectors (4 floats or 8 int16); the launcher refuses a destination that is not
// 16-byte aligned, which the engine's staging and the codec's buffers never are (a hop is 1920 or 960 bytes).
//
// State: hist [n_streams][1920] and d_prev [n_streams], updated in place by the stream's only workgroup behind a barrier, after its last
// read.  The counters (samples seen, frames made) are data-independent and live on the host; the launch's meta entry carries them.
// No atomics, no scratch, no global workspace; the barriers inside the frame loop wait for LDS only.
#include "out_stages.h"
#include "kdev.h"
#include "tsm.h"
#include "wsola.h"

namespace q3 {

struct TsmArgs { const float* in; int T; const TsmStreamMeta* meta; const float* tabs; float* hist; int32_t* d_prev; unsigned char* out; int32_t* trace; };

__global__ void __launch_bounds__(WS_THREADS) k_tsm_stretch(TsmArgs a) {
    __shared__ __attribute__((aligned(16))) float win[Q3_TSM_HIST];
    __shared__ __attribute__((aligned(16))) float wt[2 * Q3_TSM_HOP];
    __shared__ __attribute__((aligned(16))) float stage[Q3_TSM_HOP];
    __shared__ unsigned long long best[WS_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x;
    const TsmStreamMeta mt = a.meta[g];
    if (mt.enc < 0) return;   // uniform: the stream is not stretched
    const float* __restrict__ x = a.in + (size_t)g * a.T;
    float* const h = a.hist + (size_t)mt.slot * Q3_TSM_HIST;
    const long long n_prev = mt.n_prev, n_new = mt.n_prev + a.T, step = (long long)Q3_TSM_HOP * mt.pct;
    for (int i = tid; i < 2 * Q3_TSM_HOP; i += WS_THREADS) wt[i] = a.tabs[i];
    int d_prev = a.d_prev[mt.slot];
    unsigned char* const ob = a.out + mt.out_off;   // 16-byte aligned (the launcher saw to it), and so is every hop: 1920 or 960 bytes
    for (int f = 0; f < mt.n_frames; f++) {
        const long long k = mt.k0 + f, ak = k * step / 100;
        const long long tk = k == 0 ? 0 : (k - 1) * step / 100 + d_prev + Q3_TSM_HOP;
        const int d = wsola_frame(ak, tk, x, h, n_prev, n_new, win, wt, best, stage);
        wg_barrier_lds();
        if (mt.enc == Q3_PCM_S16) {
            uint16_t* o = reinterpret_cast<uint16_t*>(ob) + (size_t)f * Q3_TSM_HOP;
            if (tid < Q3_TSM_HOP / 8) reinterpret_cast<uint4*>(o)[tid] = pcm_pack8(reinterpret_cast<const float4*>(stage)[2 * tid], reinterpret_cast<const float4*>(stage)[2 * tid + 1]);
        } else {
            float* o = reinterpret_cast<float*>(ob) + (size_t)f * Q3_TSM_HOP;
            if (tid < Q3_TSM_HOP / 4) reinterpret_cast<float4*>(o)[tid] = reinterpret_cast<const float4*>(stage)[tid];
        }
        if (tid == 0 && a.trace) a.trace[mt.trace_off + f] = d;
        d_prev = d;
    }
    wsola_finish(x, a.T, h, a.d_prev + mt.slot, d_prev);
}

TsmStretcher::TsmStretcher(int n_streams_, int max_group_, StageCounters* count_) : StageBase(n_streams_, max_group_, count_, "stretcher") {
    std::vector<float> t(2 * Q3_TSM_HOP);
    tsm_windows(t.data(), t.data() + Q3_TSM_HOP);
    tabs.alloc(t.size()); tabs.upload(t.data(), t.size());
    hist_own.alloc((size_t)n_streams * Q3_TSM_HIST); hist_own.zero();
    hist = hist_own.p;
    d_prev.alloc((size_t)n_streams); d_prev.zero();
    Q3_HIP(hipStreamSynchronize(nullptr)); // the memsets ran on the null stream, which the caller's non-blocking streams do not wait for
    ring.alloc(max_group);
    n_seen.assign((size_t)n_streams, 0); k_done.assign((size_t)n_streams, 0);
}

void TsmStretcher::reset_async(hipStream_t st, int slot) {
    check_slot(slot);
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
    const TsmStreamMeta* dm;
    TsmStreamMeta* hm = s.ring.take(&dm);
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
        s.count->tsm_chunks += T > 0; s.count->tsm_frames += m.n_frames; s.count->tsm_flushes += flush;
    }
    s.ring.commit(st, G);
    TsmArgs a{in, T, dm, s.tabs.p, s.hist, s.d_prev.p, (unsigned char*)out, trace};
    hipLaunchKernelGGL(k_tsm_stretch, dim3((unsigned)G), dim3(WS_THREADS), 0, st, a);
    s.ring.launched(st);
}

} // namespace q3
