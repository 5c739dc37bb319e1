// pitch.hip -- [EXT] pitch (q3tts_spec.h "pitch"): the stretcher at the rational tempo R / P and the L / M = 100 / P resampler behind it, one
// launch per decode pass that has a stream with a pitch.
//
// k_tsm_pitch: grid = G, 512 lanes, one workgroup per stream; a stream without a pitch exits at once.  Stage 1 is the stretcher's frame
// step, wsola_frame (wsola.h), with a_k = floor(k * 480 * R / P).  The hop z[480 k .. 480 k + 480) is not delivered: it goes into LDS behind
// the stream's last 64 samples of z (zb[0 .. 64) = z[480 k - 64 .. 480 k), zb[64 + i] = z[480 k + i]).  Stage 2 then forms the delivered
// samples this hop completes, n in [ceil(480 k L / M), ceil(480 (k + 1) L / M)), at most 961: lane i takes n_lo + i, n_lo + i + 512; with
// t = n M, j = t div L and p = t mod L it sums h32[p + kk L] * z[j - kk], kk ascending, one fmaf per term.  j lies in this hop and kk <= 64, so
// every read stays inside zb.  The samples are parked in LDS and leave as 16-byte vectors where the destination allows, with plain stores up
// to the first 16-byte boundary and behind the last whole vector: the outputs of a hop start wherever the hops before it ended.
//
// The pitch's tap table is loaded into LDS once per launch, as it lies in memory (6369 floats at most, pitch 199).  For a given kk the lanes
// of a wave read h32[p_n + kk L]: the phases of consecutive n advance by M mod L, L and M are coprime, so 32 consecutive lanes hold 32
// distinct phases when L >= 32 and the same few (a broadcast) when L is small.  ds_read_b32 banks by dword mod 32 within a 32-lane half, so
// distinct phases in [0, 100) put at most 4 addresses on one bank; a phase-major image with an odd row stride would spread them no better,
// since the bank is then p * stride mod 32, again a function of p mod 32.  The z reads have stride M / L in [1/2, 2] dwords: 2-way at most.
// At 50 hops per second and stream that is at most 961 * 65 term pairs a hop beside the 481 * 480 of the search: left as it is.
//
// State: hist [n_streams][1920] and d_prev [n_streams] as the stretcher's, zhist [n_streams][64]; all updated in place by the stream's only
// workgroup after its last read.  The counters are data-independent and live on the host.  No atomics, no scratch, no global workspace; the
// barriers inside the frame loop wait for LDS only.
#include "out_stages.h"
#include "kdev.h"
#include "pitch.h"
#include "wsola.h"
#include <mutex>

namespace q3 {

#define PT_TAB_MAX 6400                                // floats of the longest table: 2 * 16 * 199 + 1 = 6369
#define PT_OUT_MAX 964                                 // delivered samples one hop completes: at most ceil(480 * 2) + 1

struct PitchArgs { const float* in; int T; const PitchStreamMeta* meta; const float* wins; const float* tabs; float* hist; float* zhist; int32_t* d_prev; unsigned char* out; int32_t* trace; };

__global__ void __launch_bounds__(WS_THREADS) k_tsm_pitch(PitchArgs a) {
    __shared__ __attribute__((aligned(16))) float win[Q3_TSM_HIST];
    __shared__ __attribute__((aligned(16))) float wt[2 * Q3_TSM_HOP];
    __shared__ __attribute__((aligned(16))) float zb[Q3_PITCH_HIST + Q3_TSM_HOP];
    __shared__ __attribute__((aligned(16))) float stage[PT_OUT_MAX];
    __shared__ __attribute__((aligned(16))) float tab[PT_TAB_MAX];
    __shared__ unsigned long long best[WS_WAVES];
    const int g = blockIdx.x, tid = threadIdx.x;
    const PitchStreamMeta mt = a.meta[g];
    if (mt.enc < 0) return;   // uniform: the stream has no pitch
    const float* __restrict__ x = a.in + (size_t)g * a.T;
    float* const h = a.hist + (size_t)mt.slot * Q3_TSM_HIST;
    float* const zh = a.zhist + (size_t)mt.slot * Q3_PITCH_HIST;
    const long long n_prev = mt.n_prev, n_new = mt.n_prev + a.T, step = (long long)Q3_TSM_HOP * mt.R;
    const int L = mt.L, M = mt.M, n_taps = mt.n_taps < PT_TAB_MAX ? mt.n_taps : PT_TAB_MAX, esz = mt.enc == Q3_PCM_S16 ? 2 : 4;
    for (int i = tid; i < 2 * Q3_TSM_HOP; i += WS_THREADS) wt[i] = a.wins[i];
    for (int i = tid; i < n_taps; i += WS_THREADS) tab[i] = a.tabs[mt.tab_off + i];
    if (tid < Q3_PITCH_HIST) zb[tid] = zh[tid];   // lane tid alone reads and writes zb[tid] outside stage 2
    int d_prev = a.d_prev[mt.slot];
    const long long n_first = (mt.k0 * Q3_TSM_HOP * L + M - 1) / M;   // delivered samples before this launch
    unsigned char* const ob = a.out + mt.out_off;
    for (int f = 0; f < mt.n_frames; f++) {
        const long long k = mt.k0 + f, ak = k * step / mt.P;
        const long long tk = k == 0 ? 0 : (k - 1) * step / mt.P + d_prev + Q3_TSM_HOP;
        const int d = wsola_frame(ak, tk, x, h, n_prev, n_new, win, wt, best, zb + Q3_PITCH_HIST);
        wg_barrier_lds();
        // stage 2: the delivered samples this hop completes
        const long long n_lo = (k * Q3_TSM_HOP * L + M - 1) / M, n_hi = ((k + 1) * Q3_TSM_HOP * L + M - 1) / M;
        const int cnt = (int)(n_hi - n_lo) < PT_OUT_MAX ? (int)(n_hi - n_lo) : PT_OUT_MAX;   // at most 961 by L <= 2 M
        const long long t0 = n_lo * M, j0 = t0 / L;
        const int r0 = (int)(t0 - j0 * L), jb = (int)(j0 - k * Q3_TSM_HOP) + Q3_PITCH_HIST;   // j0 >= 480 k: jb >= 64
        for (int i = tid; i < cnt; i += WS_THREADS) {
            const int ti = r0 + i * M, q = ti / L, p = ti - q * L;
            int jl = jb + q;   // zb index of z[j]; j < 480 (k + 1) by the choice of n_hi
            jl = jl > Q3_PITCH_HIST + Q3_TSM_HOP - 1 ? Q3_PITCH_HIST + Q3_TSM_HOP - 1 : jl;
            int K = (n_taps - 1 - p) / L + 1;   // terms with p + kk L < N_taps: at most 65, so jl - kk >= 0
            K = K > jl + 1 ? jl + 1 : K;
            float acc = 0.0f;
            for (int kk = 0; kk < K; kk++) acc = fmaf(tab[p + kk * L], zb[jl - kk], acc);
            stage[i] = pcm_clamp(acc);
        }
        wg_barrier_lds();
        // the hop's samples leave: plain stores up to the first 16-byte boundary of the destination, whole vectors, plain stores behind them
        unsigned char* const o = ob + (size_t)(n_lo - n_first) * esz;
        const int per = 16 / esz;
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(o) & 15u)) & 15u) / (unsigned)esz);
        head = head < cnt ? head : cnt;
        const int nv = (cnt - head) / per, tail0 = head + nv * per;
        if (mt.enc == Q3_PCM_S16) {
            uint16_t* o16 = reinterpret_cast<uint16_t*>(o);
            for (int v = tid; v < nv; v += WS_THREADS) {
                const float* s = stage + head + 8 * v;
                *reinterpret_cast<uint4*>(o16 + head + 8 * v) = pcm_pack8(make_float4(s[0], s[1], s[2], s[3]), make_float4(s[4], s[5], s[6], s[7]));
            }
            for (int i = tid; i < head + (cnt - tail0); i += WS_THREADS) { const int e = i < head ? i : tail0 + (i - head); o16[e] = (uint16_t)pcm_s16(stage[e]); }
        } else {
            float* o32 = reinterpret_cast<float*>(o);
            for (int v = tid; v < nv; v += WS_THREADS) {
                const float* s = stage + head + 4 * v;
                *reinterpret_cast<float4*>(o32 + head + 4 * v) = make_float4(s[0], s[1], s[2], s[3]);
            }
            for (int i = tid; i < head + (cnt - tail0); i += WS_THREADS) { const int e = i < head ? i : tail0 + (i - head); o32[e] = stage[e]; }
        }
        if (tid < Q3_PITCH_HIST) zb[tid] = zb[Q3_TSM_HOP + tid];   // the last 64 of z move to the front: nobody else touches either range here
        if (tid == 0 && a.trace) a.trace[mt.trace_off + f] = d;
        d_prev = d;
        // the next frame's window, keys, hop and samples are written behind barriers that follow every read of this frame's
    }
    wsola_finish(x, a.T, h, a.d_prev + mt.slot, d_prev);   // behind its barrier every read of the histories is done
    if (tid < Q3_PITCH_HIST) zh[tid] = zb[tid];
}

// all 151 tables are built once per process (1.47 MB of floats, a few milliseconds) and uploaded once per shifter
static const PitchTables& pt_host_tables() {
    static std::once_flag once; static PitchTables t;
    std::call_once(once, [] { t = pitch_tables(); });
    return t;
}

PitchShifter::PitchShifter(int n_streams_, int max_group_, StageCounters* count_) : StageBase(n_streams_, max_group_, count_, "shifter") {
    std::vector<float> w(2 * Q3_TSM_HOP);
    tsm_windows(w.data(), w.data() + Q3_TSM_HOP);
    wins.alloc(w.size()); wins.upload(w.data(), w.size());
    const PitchTables& t = pt_host_tables();
    for (int P = Q3_PITCH_MIN; P <= Q3_PITCH_MAX; P++) {
        PitchPlan p;
        pitch_plan(P, &p);
        Q3_CHECK(p.n_taps <= PT_TAB_MAX && p.taps_per_output <= Q3_PITCH_HIST + 1 && 2 * p.M >= p.L, "tap table does not fit");
        tab_off[P - Q3_PITCH_MIN] = t.off[P - Q3_PITCH_MIN];
    }
    tabs.alloc(t.all.size()); tabs.upload(t.all.data(), t.all.size());
    count->pitch_table_bytes = t.taps * (int64_t)sizeof(float);
    hist_own.alloc((size_t)n_streams * Q3_TSM_HIST); hist_own.zero();
    zhist_own.alloc((size_t)n_streams * Q3_PITCH_HIST); zhist_own.zero();
    hist = hist_own.p; zhist = zhist_own.p;
    d_prev.alloc((size_t)n_streams); d_prev.zero();
    Q3_HIP(hipStreamSynchronize(nullptr)); // the memsets ran on the null stream, which the caller's non-blocking streams do not wait for
    ring.alloc(max_group);
    n_seen.assign((size_t)n_streams, 0); k_done.assign((size_t)n_streams, 0);
}

void PitchShifter::reset_async(hipStream_t st, int slot) {
    check_slot(slot);
    Q3_HIP(hipMemsetAsync(hist + (size_t)slot * Q3_TSM_HIST, 0, sizeof(float) * Q3_TSM_HIST, st));
    Q3_HIP(hipMemsetAsync(zhist + (size_t)slot * Q3_PITCH_HIST, 0, sizeof(float) * Q3_PITCH_HIST, st));
    Q3_HIP(hipMemsetAsync(d_prev.p + slot, 0, sizeof(int32_t), st));
    n_seen[(size_t)slot] = 0; k_done[(size_t)slot] = 0;
}

void launch_tsm_pitch(hipStream_t st, PitchShifter& s, const float* in, int G, int T, bool flush, const int32_t* streams, const int32_t* rate,
                      const int32_t* pitch, const int32_t* enc, void* out, const int64_t* out_off, int64_t* n_out, int32_t* trace,
                      const int64_t* trace_off) {
    if (const char* why = pitch_launch_refusal(G, s.max_group, T, flush, streams, s.n_streams, rate, pitch, enc)) throw Error(std::string("tsm pitch: ") + why);
    Q3_CHECK((in || T == 0) && out && out_off && n_out && (!trace || trace_off), "bad buffers");
    bool any = false;
    for (int g = 0; g < G; g++) {   // the last of the checks: nothing of the shifter has changed yet
        if (pitch[g] == 100) continue;
        any = true;
        const uintptr_t dst = reinterpret_cast<uintptr_t>(out) + (uintptr_t)out_off[g];
        Q3_CHECK(out_off[g] >= 0 && (dst & (enc[g] == Q3_PCM_S16 ? 1u : 3u)) == 0, "misaligned output");
    }
    if (!any) return;   // no stream has a pitch: nothing to run
    const PitchStreamMeta* dm;
    PitchStreamMeta* hm = s.ring.take(&dm);
    for (int g = 0; g < G; g++) {
        PitchStreamMeta& m = hm[g];
        m = PitchStreamMeta{};
        m.enc = pitch[g] == 100 ? -1 : enc[g];
        m.slot = streams[g]; m.R = rate[g]; m.P = pitch[g];
        m.out_off = out_off[g]; m.trace_off = trace ? trace_off[g] : 0;
        if (m.enc < 0) continue;
        PitchPlan p;
        pitch_plan(pitch[g], &p);
        m.L = p.L; m.M = p.M; m.n_taps = p.n_taps; m.tab_off = s.tab_off[pitch[g] - Q3_PITCH_MIN];
        int64_t& seen = s.n_seen[(size_t)streams[g]]; int64_t& done = s.k_done[(size_t)streams[g]];
        const int64_t total = std::max<int64_t>(pitch_frames(rate[g], pitch[g], seen + T, flush), done);
        m.n_prev = seen; m.k0 = done; m.n_frames = (int32_t)(total - done);
        n_out[g] = pitch_samples_of_z(p, total * Q3_TSM_HOP) - pitch_samples_of_z(p, done * Q3_TSM_HOP);
        seen += T; done = total;
        s.count->pitch_chunks += T > 0; s.count->pitch_samples += n_out[g]; s.count->pitch_flushes += flush;
    }
    s.ring.commit(st, G);
    PitchArgs a{in, T, dm, s.wins.p, s.tabs.p, s.hist, s.zhist, s.d_prev.p, (unsigned char*)out, trace};
    hipLaunchKernelGGL(k_tsm_pitch, dim3((unsigned)G), dim3(WS_THREADS), 0, st, a);
    s.ring.launched(st);
}

} // namespace q3
