// intake.hip -- [EXT] reference audio intake (q3tts_spec.h "reference audio intake"): clips in the caller's rate, sample format and channel
// count become mono f32 at 24000 Hz, one launch per ragged batch.
//
// k_intake: grid = (output tiles, clips), 256 lanes.  A block reads its clip's meta entry and leaves at once if its tile lies past the
// clip's n_out.  The ratio's filter table goes into LDS phase-major, [L][stride] as the output converter keeps it (pcmout.hip), the tile's
// input window beside it: frame j of the clip decoded and downmixed from the raw bytes, zero for j outside [0, n).  Lane `tid` computes
// outputs tid, tid + 256, ... of the tile -- one f32 accumulator from +0, k ascending, one fmaf per tap; a zero tap of a padded row adds
// +0 * x to the sum and changes nothing for finite x -- and parks the value in LDS; the tile leaves as 16-byte vectors, its tail as scalars.
// The tile's size is the host's choice per ratio (intake.h) so that table, window and outputs fit the block's 64 KB.  A 24000 Hz clip has
// no table and no window: the decoded, downmixed frames go straight to the output.
//
// Non-finite input: every lane notes whether a frame it decoded was not finite, a wave ballots, and the block stores one int.  The windows
// of a clip's tiles cover every frame of the clip, so the host's sum over the clip's blocks is nonzero exactly if the clip holds such a
// frame.  No atomics, no scratch, no global workspace; the barriers wait for LDS only.
#include "kernels.h"
#include "kdev.h"
#include "intake.h"
#include <map>
#include <memory>

namespace q3 {

#define IN_THREADS 256
constexpr size_t INTAKE_KEEP_BYTES = (size_t)256 << 20;   // the largest input or output buffer a stage keeps between calls

__device__ __forceinline__ float intake_decode(const unsigned char* __restrict__ s, size_t idx, int fmt) {
    switch (fmt) {
    case Q3_INTAKE_U8: return (float)((int)s[idx] - 128) / 128.0f;
    case Q3_INTAKE_S16: return (float)reinterpret_cast<const int16_t*>(s)[idx] / 32768.0f;
    case Q3_INTAKE_S24: {   // three single-byte loads: a 3-byte sample is aligned to nothing
        const unsigned char* b = s + idx * 3;
        const int v = (int)b[0] | ((int)b[1] << 8) | ((int)(signed char)b[2] * 65536);
        return (float)v / 8388608.0f;
    }
    case Q3_INTAKE_S32: return (float)reinterpret_cast<const int32_t*>(s)[idx] / 2147483648.0f;
    default: return reinterpret_cast<const float*>(s)[idx];
    }
}
// frame j of the clip as one f32 sample
__device__ __forceinline__ float intake_mono(const IntakeClipMeta& mt, int j) {
    const size_t at = (size_t)j * mt.C;
    float v = intake_decode(mt.src, at, mt.fmt);
    if (mt.mix == Q3_INTAKE_MEAN) {
        for (int ch = 1; ch < mt.C; ch++) v = v + intake_decode(mt.src, at + ch, mt.fmt);
        v = v / (float)mt.C;
    }
    return v;
}
__device__ __forceinline__ int intake_not_finite(float v) { return (__builtin_bit_cast(uint32_t, v) & 0x7f800000u) == 0x7f800000u; }

__global__ void __launch_bounds__(IN_THREADS) k_intake(const IntakeClipMeta* __restrict__ meta, int32_t* __restrict__ flags) {
    __shared__ __attribute__((aligned(16))) float lds[INTAKE_LDS_FLOATS];
    __shared__ int wave_bad[IN_THREADS / 64];
    const IntakeClipMeta mt = meta[blockIdx.y];
    const int tid = threadIdx.x, tile = mt.tile, m0 = blockIdx.x * tile;
    if (m0 >= mt.n_out) return;   // uniform: a tile past this clip's output
    const int cnt = min(tile, mt.n_out - m0), L = mt.L, M = mt.M, stride = mt.stride;
    float* const tab = lds; float* const win = lds + L * stride; float* const stage = win + mt.win;
    int bad = 0;
    if (stride == 0) {   // 24000 Hz: no filter (win == lds, mt.win == 0)
        for (int i = tid; i < cnt; i += IN_THREADS) {
            const float v = intake_mono(mt, m0 + i);
            bad |= intake_not_finite(v);
            stage[i] = v;
        }
    } else {
        const float4* __restrict__ t4 = reinterpret_cast<const float4*>(mt.tab);
        for (int i = tid; i < (L * stride) >> 2; i += IN_THREADS) reinterpret_cast<float4*>(tab)[i] = t4[i];
        // outputs m0 .. m0 + cnt - 1 read x[j - k], j = (m M + c) div L in [j_lo, j_hi], k in [0, stride): the window starts at j_lo - (stride - 1)
        const int j_lo = (m0 * M + mt.c) / L, j_hi = ((m0 + cnt - 1) * M + mt.c) / L, base = j_lo - (stride - 1), wn = j_hi - base + 1;
        for (int i = tid; i < wn; i += IN_THREADS) {
            const int j = base + i;
            const float v = (j >= 0 && j < mt.n) ? intake_mono(mt, j) : 0.0f;
            bad |= intake_not_finite(v);
            win[i] = v;
        }
    }
    const bool any = __ballot(bad) != 0;
    if ((tid & 63) == 0) wave_bad[tid >> 6] = any ? 1 : 0;
    wg_barrier_lds();
    if (tid == 0) flags[mt.flag_off + blockIdx.x] = wave_bad[0] + wave_bad[1] + wave_bad[2] + wave_bad[3];
    if (stride != 0) {
        const int base = (m0 * M + mt.c) / L - (stride - 1);
        for (int ml = tid; ml < cnt; ml += IN_THREADS) {
            const int t = (m0 + ml) * M + mt.c, j = t / L, p = t - j * L;
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
            stage[ml] = acc;
        }
        wg_barrier_lds();
    }
    // the clip's output starts on 16 bytes and a tile is a whole number of vectors, so every tile starts on 16 bytes
    float* const o = mt.dst + m0;
    for (int v = tid; v < (cnt >> 2); v += IN_THREADS) reinterpret_cast<float4*>(o)[v] = reinterpret_cast<const float4*>(stage)[v];
    for (int i = (cnt & ~3) + tid; i < cnt; i += IN_THREADS) o[i] = stage[i];
}

static_assert(IN_THREADS == 256 && INTAKE_TILE_MIN % 4 == 0 && (INTAKE_LDS_FLOATS + IN_THREADS / 64) * 4 <= 65536, "k_intake's LDS");

IntakeStage::IntakeStage(int device_) : device(device_) {}

// the ratio's plan and its table on this device: built and uploaded by the first clip at that rate, kept from then on
const float* IntakeStage::table(int rate, IntakePlan* plan) {
    Q3_CHECK(intake_plan(rate, plan), "sample rate is not one the intake takes");
    if (plan->n_taps == 0) return nullptr;
    auto it = tabs.find(rate);
    if (it != tabs.end()) return it->second.p;
    const std::vector<float> t = intake_table(*plan, intake_filter(rate));
    // what the kernel's LDS holds: the table, the window of a full tile, the tile
    Q3_CHECK((int)t.size() == intake_table_floats(*plan) && t.size() % 4 == 0, "filter table has the wrong shape");
    Q3_CHECK(plan->tile >= INTAKE_TILE_MIN && plan->tile % 4 == 0 && intake_lds_floats(*plan, plan->tile) <= INTAKE_LDS_FLOATS, "table, window and tile do not fit");
    DevBuf<float>& d = tabs[rate];
    d.alloc(t.size()); d.upload(t.data(), t.size());
    return d.p;
}

IntakeStage& intake_stage(int device) {
    static std::mutex mu;
    static std::map<int, std::unique_ptr<IntakeStage>> stages;
    std::lock_guard<std::mutex> lk(mu);
    std::unique_ptr<IntakeStage>& s = stages[device];
    if (!s) s.reset(new IntakeStage(device));
    return *s;
}

void launch_intake(hipStream_t st, const IntakeClipMeta* d_meta, int n_clips, int tiles, int32_t* d_flags) {
    Q3_CHECK(d_meta && d_flags && n_clips >= 1 && n_clips <= Q3_INTAKE_MAX_CLIPS && tiles >= 1 && tiles <= Q3_INTAKE_MAX_OUT / INTAKE_TILE_MIN, "bad intake launch");
    hipLaunchKernelGGL(k_intake, dim3((unsigned)tiles, (unsigned)n_clips), dim3(IN_THREADS), 0, st, d_meta, d_flags);
    Q3_LAUNCH_CHECK();
}

void intake_run(IntakeStage& s, const q3tts_intake_clip* clips, int n_clips, float* const* out, const int64_t* out_cap, int64_t* n_out) {
    // everything is checked before anything is allocated or launched
    Q3_CHECK(clips && out && out_cap && n_out, "null argument");
    if (n_clips < 1 || n_clips > Q3_INTAKE_MAX_CLIPS) throw Error("intake: clip count outside [1, 64]");
    std::vector<int64_t> cnt((size_t)n_clips);
    for (int i = 0; i < n_clips; i++) {
        if (const char* why = intake_refusal(&clips[i])) throw Error("intake: clip " + std::to_string(i) + ": " + why);
        cnt[i] = intake_samples(clips[i].sample_rate, clips[i].n_frames);
        if (!out[i] || out_cap[i] < cnt[i]) throw Error("intake: clip " + std::to_string(i) + ": output holds fewer than " + std::to_string(cnt[i]) + " samples");
    }
    std::lock_guard<std::mutex> own(s.mu);
    std::lock_guard<std::mutex> cap(capture_mutex());   // synchronous allocations and copies beside an engine that may be capturing
    int prev = 0;
    Q3_HIP(hipGetDevice(&prev));
    Q3_HIP(hipSetDevice(s.device));
    struct Back { int d; ~Back() { (void)hipSetDevice(d); } } back{prev};
    std::vector<IntakeClipMeta> hm((size_t)n_clips);
    std::vector<size_t> in_off((size_t)n_clips), out_off((size_t)n_clips);
    size_t in_bytes = 0, out_floats = 0;
    int flag_n = 0, tiles = 0;
    for (int i = 0; i < n_clips; i++) {
        const q3tts_intake_clip& c = clips[i];
        IntakePlan p;
        IntakeClipMeta& m = hm[i];
        m.tab = s.table(c.sample_rate, &p);
        in_off[i] = in_bytes; out_off[i] = out_floats;
        in_bytes += ((size_t)c.n_frames * c.channels * intake_sample_bytes(c.sample_format) + 15) / 16 * 16;
        out_floats += ((size_t)cnt[i] + 3) / 4 * 4;
        m.n = (int32_t)c.n_frames; m.n_out = (int32_t)cnt[i];
        m.L = p.L; m.M = p.M; m.stride = p.stride; m.c = p.c; m.tile = p.tile;
        m.win = p.stride ? (int32_t)((intake_window_floats(p, p.tile) + 3) / 4 * 4) : 0;
        m.C = c.channels; m.fmt = c.sample_format; m.mix = c.downmix; m.flag_off = flag_n;
        const int t = (int)((cnt[i] + p.tile - 1) / p.tile);
        flag_n += t;
        if (t > tiles) tiles = t;
    }
    // the stage's buffers grow to the largest call seen; one too large to keep is given back when the call ends
    DevBuf<unsigned char>& d_in = s.in; DevBuf<float>& d_out = s.out; DevBuf<int32_t>& d_flags = s.flags; DevBuf<IntakeClipMeta>& d_meta = s.meta;
    struct Trim { IntakeStage& s; ~Trim() { if (s.in.n > INTAKE_KEEP_BYTES) s.in.release(); if (s.out.n * sizeof(float) > INTAKE_KEEP_BYTES) s.out.release(); } } trim{s};
    if (d_in.n < in_bytes) d_in.alloc(in_bytes);
    if (d_out.n < out_floats) d_out.alloc(out_floats);
    if (d_flags.n < (size_t)flag_n) d_flags.alloc((size_t)flag_n);
    if (d_meta.n < (size_t)n_clips) d_meta.alloc(Q3_INTAKE_MAX_CLIPS);
    for (int i = 0; i < n_clips; i++) {
        const size_t nb = (size_t)clips[i].n_frames * clips[i].channels * intake_sample_bytes(clips[i].sample_format);
        Q3_HIP(hipMemcpy(d_in.p + in_off[i], clips[i].data, nb, hipMemcpyHostToDevice));
        hm[i].src = d_in.p + in_off[i]; hm[i].dst = d_out.p + out_off[i];
    }
    d_meta.upload(hm.data(), hm.size());
    launch_intake(nullptr, d_meta.p, n_clips, tiles, d_flags.p);
    Q3_HIP(hipDeviceSynchronize());
    std::vector<int32_t> flags((size_t)flag_n);
    d_flags.download(flags.data(), flags.size());
    for (int i = 0; i < n_clips; i++) {   // every active block of a clip wrote its flag
        const int end = i + 1 < n_clips ? hm[i + 1].flag_off : flag_n;
        for (int f = hm[i].flag_off; f < end; f++)
            if (flags[f]) throw Error("intake: clip " + std::to_string(i) + " holds a non-finite sample");
    }
    for (int i = 0; i < n_clips; i++) Q3_HIP(hipMemcpy(out[i], d_out.p + out_off[i], (size_t)cnt[i] * sizeof(float), hipMemcpyDeviceToHost));
    for (int i = 0; i < n_clips; i++) n_out[i] = cnt[i];
}

} // namespace q3
