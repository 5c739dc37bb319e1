// pcmout.hip -- [EXT] output formats (q3tts_spec.h "output formats"): sample-rate conversion and int16 PCM behind the codec, one launch per
// decode pass over G streams.
//
// k_pcm_convert: grid = (output tiles of PO_TILE samples, G), 256 lanes.  A block reads its stream's entry of the launch's meta array; the
// native format exits at once.  The rate's filter table goes into LDS phase-major, [L][stride] with stride = the taps of one output sample
// rounded up to whole 16-byte vectors (zeros behind the last tap), so that one output's taps are contiguous and read as float4.  The tile's
// input window goes into LDS beside it: the chunk's samples, the stream's history for indices in [-96, 0), zeros below that (only the zero
// taps of a padded row reach there).  Lane `tid` computes outputs tid, tid + 256, ... of the tile -- one f32 accumulator, k ascending, one fmaf
// per tap; a zero tap adds +0 * x to a sum that started at +0 and changes nothing for finite x -- clamps, and parks the value in LDS; the
// tile then leaves as 16-byte vectors: 4 floats, or 8 int16 when the destination is 16-byte aligned.  (A frame is a whole number of f32
// vectors at every rate, but 1764 int16 = 3528 bytes at 22050 Hz: an s16 destination off 16 bytes, and the tail of a tile, take scalar stores.)
//
// History: [n_streams][2][96].  A launch reads the half meta.parity names and tile 0 of the stream leaves the chunk's last 96 samples in
// the other half, so no block of the launch can read what another one wrote; the host flips the parity per launch.  Every chunk is at
// least one frame long, so the tail always comes from one chunk.  No atomics, no scratch, no global workspace; the barriers wait for LDS only.
#include "out_stages.h"
#include "kdev.h"
#include "pcm_out.h"
#include "wsola.h"

namespace q3 {

#define PO_THREADS 256
#define PO_TILE 1024                                   // output samples per block
#define PO_TAB_MAX (147 * 36)                          // floats of the largest table (22050 and 44100 Hz)
#define PO_WIN_MAX 3200                                // floats of the largest window: 1023 * 3 + 1 + 100 at 8000 Hz

struct PcmConvertArgs { const float* in; int T; const PcmStreamMeta* meta; const float* tabs; float* hist; unsigned char* out; };

__global__ void __launch_bounds__(PO_THREADS) k_pcm_convert(PcmConvertArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[PO_TAB_MAX + PO_WIN_MAX + PO_TILE];
    float* const tab = lds; float* const win = lds + PO_TAB_MAX; float* const stage = lds + PO_TAB_MAX + PO_WIN_MAX;
    const int g = blockIdx.y, tid = threadIdx.x;
    const PcmStreamMeta mt = a.meta[g];
    const int m0 = blockIdx.x * PO_TILE;
    if (mt.enc < 0 || m0 >= mt.n_out) return;   // uniform: the native format, or a tile past this stream's output
    const int cnt = min(PO_TILE, mt.n_out - m0), L = mt.L, M = mt.M, stride = mt.stride;
    const float* __restrict__ x = a.in + (size_t)g * a.T;
    if (stride == 0) {   // 24000 Hz: no filter
        for (int i = tid; i < cnt; i += PO_THREADS) stage[i] = pcm_clamp(x[m0 + i]);
    } else {
        const float* __restrict__ hr = a.hist + ((size_t)mt.slot * 2 + mt.parity) * Q3_PCM_HIST;
        if (blockIdx.x == 0 && tid < Q3_PCM_HIST) a.hist[((size_t)mt.slot * 2 + (mt.parity ^ 1)) * Q3_PCM_HIST + tid] = x[a.T - Q3_PCM_HIST + tid];
        const float4* __restrict__ t4 = reinterpret_cast<const float4*>(a.tabs + mt.tab_off);
        for (int i = tid; i < (L * stride) >> 2; i += PO_THREADS) reinterpret_cast<float4*>(tab)[i] = t4[i];
        // outputs m0 .. m0 + cnt - 1 read x[j - k], j = m * M div L in [j_lo, j_hi], k in [0, stride): the window starts at j_lo - (stride - 1)
        const int j_lo = (m0 * M) / L, j_hi = ((m0 + cnt - 1) * M) / L, base = j_lo - (stride - 1), wn = j_hi - base + 1;
        for (int i = tid; i < wn; i += PO_THREADS) {
            const int j = base + i;
            win[i] = j >= 0 ? x[j] : (j >= -Q3_PCM_HIST ? hr[Q3_PCM_HIST + j] : 0.0f);
        }
        wg_barrier_lds();
        for (int ml = tid; ml < cnt; ml += PO_THREADS) {
            const int t = (m0 + ml) * M, j = t / L, p = t - j * L;
            const float4* h4 = reinterpret_cast<const float4*>(tab + p * stride);
            const float* xw = win + (j - base);   // x[j - k] = xw[-k]
            float acc = 0.0f;
            for (int k4 = 0; k4 < (stride >> 2); k4++) {
                const float4 h = h4[k4];
                acc = fmaf(h.x, xw[-4 * k4], acc);
                acc = fmaf(h.y, xw[-4 * k4 - 1], acc);
                acc = fmaf(h.z, xw[-4 * k4 - 2], acc);
                acc = fmaf(h.w, xw[-4 * k4 - 3], acc);
            }
            stage[ml] = pcm_clamp(acc);
        }
    }
    wg_barrier_lds();
    unsigned char* ob = a.out + mt.out_off + (size_t)m0 * (mt.enc == Q3_PCM_S16 ? 2 : 4);
    const bool vec = (reinterpret_cast<uintptr_t>(ob) & 15u) == 0;   // uniform
    if (mt.enc == Q3_PCM_S16) {
        uint16_t* o = reinterpret_cast<uint16_t*>(ob);
        const int nv = vec ? cnt >> 3 : 0;
        for (int v = tid; v < nv; v += PO_THREADS) {
            reinterpret_cast<uint4*>(o)[v] = pcm_pack8(reinterpret_cast<const float4*>(stage)[2 * v], reinterpret_cast<const float4*>(stage)[2 * v + 1]);
        }
        for (int i = (nv << 3) + tid; i < cnt; i += PO_THREADS) o[i] = (uint16_t)pcm_s16(stage[i]);
    } else {
        // f32: the launcher saw to it that the destination is 16-byte aligned and the count a multiple of 4 (both hold for whole frames)
        for (int v = tid; v < (cnt >> 2); v += PO_THREADS) reinterpret_cast<float4*>(ob)[v] = reinterpret_cast<const float4*>(stage)[v];
    }
}

PcmConverter::PcmConverter(int n_streams_, int max_group_, StageCounters* count_) : StageBase(n_streams_, max_group_, count_, "converter") {
    std::vector<float> all;
    for (int r = 0; r < PCM_N_RATES; r++) {
        PcmPlan p;
        pcm_plan(pcm_rates()[r], &p);
        const std::vector<float> t = pcm_filter_phase_major(p, pcm_filter(pcm_rates()[r]));
        tab_off[r] = (int)all.size(); tab_stride[r] = pcm_phase_stride(p); tab_L[r] = p.L; tab_M[r] = p.M;
        // what the kernel's LDS holds: the table, and the window of a full tile
        Q3_CHECK(t.size() <= PO_TAB_MAX && t.size() % 4 == 0 && all.size() % 4 == 0, "filter table does not fit");
        Q3_CHECK((int64_t)(PO_TILE - 1) * p.M / p.L + 1 + tab_stride[r] <= PO_WIN_MAX && p.taps_per_phase - 1 <= Q3_PCM_HIST, "input window does not fit");
        all.insert(all.end(), t.begin(), t.end());
    }
    tabs.alloc(all.size()); tabs.upload(all.data(), all.size());
    hist_own.alloc((size_t)n_streams * 2 * Q3_PCM_HIST); hist_own.zero();
    hist = hist_own.p;
    ring.alloc(max_group);
    parity.assign((size_t)n_streams, 0);
}

void PcmConverter::reset_async(hipStream_t st, int slot) {
    check_slot(slot);
    Q3_HIP(hipMemsetAsync(hist + (size_t)slot * 2 * Q3_PCM_HIST, 0, sizeof(float) * 2 * Q3_PCM_HIST, st));
}

void launch_pcm_convert(hipStream_t st, PcmConverter& c, const float* in, int G, int T, const int32_t* streams, const q3tts_pcm_format* fmt,
                        void* out, const int64_t* out_off, int64_t* n_out) {
    if (const char* why = pcm_convert_refusal(G, c.max_group, T, streams, c.n_streams, fmt)) throw Error(std::string("pcm convert: ") + why);
    Q3_CHECK(in && out && n_out && (reinterpret_cast<uintptr_t>(in) & 15u) == 0, "bad buffers");
    int64_t most = 0;
    for (int g = 0; g < G; g++) {   // the last of the checks: nothing of the converter has changed yet
        const int64_t n = pcm_samples_of_native(fmt[g].sample_rate, T), off = out_off ? out_off[g] : (int64_t)g * T * 4;
        const uintptr_t dst = reinterpret_cast<uintptr_t>(out) + (uintptr_t)off;
        const bool f32 = fmt[g].encoding == Q3_PCM_F32;
        if (!pcm_format_native(fmt[g])) Q3_CHECK(off >= 0 && (f32 ? (dst & 15u) == 0 && n % 4 == 0 : (dst & 1u) == 0), "misaligned output");
        if (!pcm_format_native(fmt[g]) && n > most) most = n;
    }
    for (int g = 0; g < G; g++) n_out[g] = pcm_samples_of_native(fmt[g].sample_rate, T);
    if (most == 0) return;   // every stream is native: nothing to run
    const PcmStreamMeta* dm;
    PcmStreamMeta* hm = c.ring.take(&dm);
    for (int g = 0; g < G; g++) {
        const int r = pcm_rate_index(fmt[g].sample_rate);
        PcmStreamMeta& m = hm[g];
        m.enc = pcm_format_native(fmt[g]) ? -1 : fmt[g].encoding;
        m.slot = streams[g]; m.parity = c.parity[(size_t)streams[g]];
        m.L = c.tab_L[r]; m.M = c.tab_M[r]; m.stride = c.tab_stride[r]; m.tab_off = c.tab_off[r]; m.n_out = (int32_t)n_out[g];
        m.out_off = out_off ? out_off[g] : (int64_t)g * T * 4; m.pad = 0;
        if (m.enc >= 0) { c.parity[(size_t)streams[g]] ^= 1; c.count->conv_chunks++; c.count->conv_samples += n_out[g]; }
    }
    c.ring.commit(st, G);
    PcmConvertArgs a{in, T, dm, c.tabs.p, c.hist, (unsigned char*)out};
    hipLaunchKernelGGL(k_pcm_convert, dim3((unsigned)((most + PO_TILE - 1) / PO_TILE), G), dim3(PO_THREADS), 0, st, a);
    c.ring.launched(st);
}

} // namespace q3
