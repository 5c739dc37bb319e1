// out_stages.h -- [EXT] the five stages behind the codec's output conv (q3tts_spec.h "output formats", "speaking rate", "pitch", "volume",
// "loudness"): each one's per-stream launch entry, its device state and its launcher, with what they share -- the shape and slot checks, the
// upload ring and the counters.  OutChain (out_chain.h) runs them behind a pass; the test entry points (capi_ops.cpp) run each alone.
#pragma once
#include "q3_common.h"
#include "../../include/q3tts.h"
#include "sched_logic.h"
#include <atomic>

namespace q3 {

// The stages' counters (OutputStageStats, sched_logic.h, field for field): added to by the launchers on the owner thread, read by any thread.
// A stage counts into the block it is given -- the chain's, which outlives its stages and is never re-pointed -- or into its own.
struct StageCounters {
    std::atomic<int64_t> conv_chunks{0}, conv_samples{0}, tsm_chunks{0}, tsm_frames{0}, tsm_flushes{0};
    std::atomic<int64_t> pitch_chunks{0}, pitch_samples{0}, pitch_flushes{0}, pitch_table_bytes{0}, vol_chunks{0}, vol_samples{0};
    std::atomic<int64_t> loud_chunks{0}, loud_blocks{0};
    OutputStageStats snapshot() const {
        OutputStageStats s;
        s.conv_chunks = conv_chunks; s.conv_samples = conv_samples; s.tsm_chunks = tsm_chunks; s.tsm_frames = tsm_frames; s.tsm_flushes = tsm_flushes;
        s.pitch_chunks = pitch_chunks; s.pitch_samples = pitch_samples; s.pitch_flushes = pitch_flushes; s.pitch_table_bytes = pitch_table_bytes;
        s.vol_chunks = vol_chunks; s.vol_samples = vol_samples; s.loud_chunks = loud_chunks; s.loud_blocks = loud_blocks;
        return s;
    }
};

// What every stage is: a state store of n_streams slots, launches of up to max_group streams, counters.  One owner thread; its launches may
// go to different HIP streams, and the caller orders a stream slot's chunks across them as it does for the codec.
struct StageBase {
    StageBase(int n_streams_, int max_group_, StageCounters* count_, const char* what) : n_streams(n_streams_), max_group(max_group_), count(count_ ? count_ : &own_) {
        Q3_CHECK(n_streams >= 1 && max_group >= 1, std::string("bad ") + what + " shape");
    }
    StageBase(const StageBase&) = delete; StageBase& operator=(const StageBase&) = delete;
    void check_slot(int slot) const { Q3_CHECK(slot >= 0 && slot < n_streams, "stream out of range"); }
    int n_streams, max_group;
    StageCounters* count;
private:
    StageCounters own_;
};

// The stages' upload ring: 64 slots of max_group launch entries each, pinned host + device, every slot with the event of the launch
// that last read it.  take() waits for that launch, on whichever HIP stream it ran, and hands out the slot's host entries and their device
// address; commit() uploads the first G of them on the launch's stream; launched() records the launch.  One owner thread.
template <class Meta> struct UploadRing {
    static constexpr int SLOTS = 64;
    UploadRing() = default;
    UploadRing(const UploadRing&) = delete; UploadRing& operator=(const UploadRing&) = delete;
    ~UploadRing() {
        for (auto e : ev) if (e) (void)hipEventDestroy(e);
        if (host) (void)hipHostFree(host);
    }
    void alloc(int max_group_) {
        max_group = max_group_;
        dev.alloc((size_t)SLOTS * max_group);
        Q3_HIP(hipHostMalloc((void**)&host, sizeof(Meta) * SLOTS * max_group));
        for (auto& e : ev) Q3_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    Meta* take(const Meta** d) {
        cur = next; next = (next + 1) % SLOTS;
        if (used[cur]) Q3_HIP(hipEventSynchronize(ev[cur]));   // the slot's previous launch has consumed its upload
        *d = dev.p + (size_t)cur * max_group;
        return host + (size_t)cur * max_group;
    }
    void commit(hipStream_t st, int G) {
        Q3_HIP(hipMemcpyAsync(dev.p + (size_t)cur * max_group, host + (size_t)cur * max_group, sizeof(Meta) * G, hipMemcpyHostToDevice, st));
    }
    void launched(hipStream_t st) { Q3_HIP(hipEventRecord(ev[cur], st)); used[cur] = 1; }
    int max_group = 0, cur = 0, next = 0;
    DevBuf<Meta> dev; Meta* host = nullptr; hipEvent_t ev[SLOTS] = {}; char used[SLOTS] = {};
};

// [EXT] output formats (pcmout.hip): sample-rate conversion and int16 PCM behind the codec.
// One entry per stream of a launch, written by launch_pcm_convert into the converter's upload ring.
struct PcmStreamMeta {
    int32_t enc;              // Q3_PCM_F32 / Q3_PCM_S16; -1: the native format, the stream's blocks exit at once
    int32_t slot, parity;     // history store entry; which of its two halves this launch reads (it leaves the new tail in the other)
    int32_t L, M, stride;     // the rate's ratio; floats per phase row of its table (0: 24000 Hz, no filter)
    int32_t tab_off, n_out;   // first float of the rate's table in PcmConverter::tabs; output samples of this chunk
    int64_t out_off, pad;     // first output byte, from the launch's `out`
};
// The converter's device state: the eight filter tables (phase-major, pcm_out.h), the history store [n_streams][2][Q3_PCM_HIST], and its
// upload ring.  Counts conv_chunks (stream chunks converted) and conv_samples.
struct PcmConverter : StageBase {
    PcmConverter(int n_streams, int max_group, StageCounters* count = nullptr);
    void reset_async(hipStream_t st, int slot);   // zeroes the slot's history: its next sample is sample 0 of a stream
    float* hist;                                   // = hist_own.p, or a caller's store of the same shape (the test entry point's guarded one)
    DevBuf<float> tabs, hist_own; UploadRing<PcmStreamMeta> ring;
    int tab_off[8], tab_stride[8], tab_L[8], tab_M[8];
    std::vector<uint8_t> parity;                   // per slot: the half the next launch reads
};
// in [G][T] native samples (T = frames * 1920), stream g of history slot streams[g] in format fmt[g].  Stream g's T*L/M output samples go to
// out + out_off[g] bytes (out_off NULL: g * T * 4, which every format fits into); n_out[g] receives their count.  A native stream is not
// touched: n_out[g] = T and its bytes stay where they are, in `in`.  16-byte stores where the destination is 16-byte aligned.
// Refused (pcm_convert_refusal, pcm_out.h) before anything is uploaded or launched: T % 1920 != 0, G outside [1, max_group], an unknown
// format, a stream out of range or listed twice.
void launch_pcm_convert(hipStream_t st, PcmConverter& c, const float* in, int G, int T, const int32_t* streams, const q3tts_pcm_format* fmt,
                        void* out, const int64_t* out_off, int64_t* n_out);

// [EXT] speaking rate (tsm.hip): WSOLA time-scale change behind the codec.
// One entry per stream of a launch, written by launch_tsm_stretch into the stretcher's upload ring.  The counts are data-independent, so the
// host keeps the two counters of every stream and hands the kernel what it derived from them.
struct TsmStreamMeta {
    int32_t enc;              // Q3_PCM_F32 / Q3_PCM_S16; -1: the stream is not stretched, its workgroup exits at once
    int32_t slot, pct;        // state store entry; the rate
    int32_t n_frames;         // synthesis frames this launch makes: k0 .. k0 + n_frames - 1
    int64_t n_prev, k0;       // native samples seen before this chunk; first frame to make
    int64_t out_off;          // first output byte, from the launch's `out`
    int64_t trace_off;        // first entry of the launch's `trace` (unused when that is NULL)
};
// The stretcher's device state: the two window tables, the history store [n_streams][Q3_TSM_HIST] (a stream's last 1920 native samples), the
// offset of every stream's last frame, and an upload ring as the converter's.  n_seen / k_done are the host's counters per stream.  Counts
// tsm_chunks (stream chunks taken), tsm_frames (synthesis frames made) and tsm_flushes.
struct TsmStretcher : StageBase {
    TsmStretcher(int n_streams, int max_group, StageCounters* count = nullptr);
    void reset_async(hipStream_t st, int slot);    // zeroes the slot's history, offset and counters: its next sample is sample 0 of a stream
    float* hist;                                   // = hist_own.p, or a caller's store of the same shape (the test entry point's guarded one)
    DevBuf<float> tabs, hist_own; DevBuf<int32_t> d_prev; UploadRing<TsmStreamMeta> ring;
    std::vector<int64_t> n_seen, k_done;
};
// in [G][T] native samples (T a multiple of 1920; 0 with flush alone), stream g of state slot streams[g] at pct[g] percent in encoding
// enc[g].  The frames that became available (with flush: every frame with a_k < N, the input ending in zeros) go to out + out_off[g] bytes,
// 480 samples each; n_out[g] receives their sample count.  A stream at 100 is not touched: n_out[g] = T and its bytes stay where they are, in
// `in`.  trace (optional, device) receives d_k of every frame made, stream g's from entry trace_off[g] on.  The hops leave as 16-byte
// stores: out + out_off[g] must be 16-byte aligned.  A flushed stream must be reset before it is used again.
// Refused (tsm_launch_refusal, tsm.h) before anything is uploaded or launched.
void launch_tsm_stretch(hipStream_t st, TsmStretcher& s, const float* in, int G, int T, bool flush, const int32_t* streams, const int32_t* pct,
                        const int32_t* enc, void* out, const int64_t* out_off, int64_t* n_out, int32_t* trace = nullptr,
                        const int64_t* trace_off = nullptr);

// [EXT] pitch (pitch.hip): the stretcher at the rational tempo R / P and the L / M resampler behind it, in one launch.
// One entry per stream of a launch, written by launch_tsm_pitch into the shifter's upload ring.  As with the stretcher every count is
// data-independent: the host keeps the counters and hands the kernel what it derived from them.
struct PitchStreamMeta {
    int32_t enc;              // Q3_PCM_F32 / Q3_PCM_S16; -1: the stream has no pitch, its workgroup exits at once
    int32_t slot, R, P;       // state store entry; the rate and the pitch
    int32_t L, M, n_taps;     // 100 / P in lowest terms and the taps of its prototype
    int32_t tab_off;          // first float of the pitch's h32 in the shifter's tables
    int32_t n_frames, pad;    // stage-1 frames this launch makes: k0 .. k0 + n_frames - 1
    int64_t n_prev, k0;       // native samples seen before this chunk; first frame to make
    int64_t out_off;          // first output byte, from the launch's `out`
    int64_t trace_off;        // first entry of the launch's `trace` (unused when that is NULL)
};
// The shifter's device state: the stretcher's (window tables, history [n_streams][Q3_TSM_HIST], d of every stream's last frame), the
// intermediate history [n_streams][Q3_PITCH_HIST] (a stream's last 64 samples of z), all 151 tap tables (pitch.h), and an upload ring as
// the stretcher's.  n_seen / k_done are the host's counters per stream; Nz = 480 k_done and the outputs made follow from them.  Counts
// pitch_chunks (stream chunks shifted), pitch_samples (delivered), pitch_flushes, and sets pitch_table_bytes when it is made.
struct PitchShifter : StageBase {
    PitchShifter(int n_streams, int max_group, StageCounters* count = nullptr);
    void reset_async(hipStream_t st, int slot);    // zeroes the slot's two histories, offset and counters: its next sample is sample 0 of a stream
    float* hist; float* zhist;                     // = the own stores, or a caller's of the same shapes (the test entry point's guarded ones)
    DevBuf<float> wins, tabs, hist_own, zhist_own; DevBuf<int32_t> d_prev; UploadRing<PitchStreamMeta> ring;
    int tab_off[151];
    std::vector<int64_t> n_seen, k_done;
};
// in [G][T] native samples (T a multiple of 1920; 0 with flush alone), stream g of state slot streams[g] at rate[g] percent and pitch[g]
// percent in encoding enc[g].  The delivered samples that became available (with flush: those of every frame with a_k < N) go to
// out + out_off[g] bytes, which need the alignment of one sample only; n_out[g] receives their count.  A stream at pitch 100 is not touched:
// n_out[g] is left alone and its bytes stay where they are.  trace (optional, device) receives d_k of every stage-1 frame made, stream g's
// from entry trace_off[g] on.  A flushed stream must be reset before it is used again.
// Refused (pitch_launch_refusal, pitch.h) before anything is uploaded or launched.
void launch_tsm_pitch(hipStream_t st, PitchShifter& s, const float* in, int G, int T, bool flush, const int32_t* streams, const int32_t* rate,
                      const int32_t* pitch, const int32_t* enc, void* out, const int64_t* out_off, int64_t* n_out, int32_t* trace = nullptr,
                      const int64_t* trace_off = nullptr);

// [EXT] volume (volume.hip): a gain with a look-ahead peak limiter, in place on the native chunk, in front of the other output stages.
// One entry per stream of a launch, written by launch_volume into the stage's upload ring.
struct VolStreamMeta {
    float gain;               // G of the stream's volume
    int32_t slot;             // state store entry; -1: the stream has no volume, its workgroup exits at once
    int64_t trace_off;        // first entry of the launch's `trace` (unused when that is NULL)
};
// The stage's device state: the store [n_streams][Q3_VOL_HIST] (a stream's last 638 values of v) and an upload ring as the other stages'.
// The stage maps sample n to sample n.  Counts vol_chunks (stream chunks taken) and vol_samples (rewritten).
struct VolumeStage : StageBase {
    VolumeStage(int n_streams, int max_group, StageCounters* count = nullptr);
    void reset_async(hipStream_t st, int slot);    // zeroes the slot's store: its next sample is sample 0 of a stream
    float* hist;                                   // = hist_own.p, or a caller's store of the same shape (the test entry point's guarded one)
    DevBuf<float> hist_own; UploadRing<VolStreamMeta> ring;
};
// pcm [G][T] native samples (T a multiple of 1920, pcm 16-byte aligned), rewritten in place: stream g of state slot streams[g] at db10[g]
// tenths of a dB becomes y of "volume".  A stream at 0 is not touched.  trace (optional, device) receives g[n] of every sample made, stream
// g's from entry trace_off[g] on.  Nothing runs when no stream has a volume.
// Refused (volume_launch_refusal, volume.h) before anything is uploaded or launched.
void launch_volume(hipStream_t st, VolumeStage& s, float* pcm, int G, int T, const int32_t* streams, const int32_t* db10, float* trace = nullptr,
                   const int64_t* trace_off = nullptr);

// [EXT] loudness (loudness.hip): the K-weighted 100 ms block energies and peaks of the native chunk, in front of the volume stage; it reads
// the chunk and never writes it.  One entry per stream of a launch, written by launch_loudness into the upload ring.
struct LoudStreamMeta {
    int32_t slot;             // state store entry; -1: the stream is not metered, its workgroup exits at once
    int32_t pad;
    int64_t pos;              // native samples the stream was given before this chunk, since its reset
    int64_t out_off;          // first output byte, from the launch's `out`
};
// The stage's device state: the store [n_streams][Q3_LOUD_STATE] doubles (filter state, running energy and peak), the tables (loudness.h,
// built once on the host) and an upload ring as the other stages'.  The host passes every stream's position.  Counts loud_chunks (stream
// chunks metered) and loud_blocks (completed).
struct LoudnessStage : StageBase {
    LoudnessStage(int n_streams, int max_group, StageCounters* count = nullptr);
    void reset_async(hipStream_t st, int slot);    // zeroes the slot's state: its next sample is sample 0 of a stream
    double* state;                                 // = state_own.p, or a caller's store of the same shape (the test entry point's guarded one)
    DevBuf<double> state_own; UploadRing<LoudStreamMeta> ring;
    double coef[10], m[16];
};
// pcm [G][T] native samples (T a multiple of 1920), read only.  Stream g of state slot streams[g], metered where metered[g] != 0 and then at
// stream position pos[g] (a multiple of 1920): the rows {energy, peak} of the blocks the chunk completes go to out + out_off[g] bytes
// (8-byte aligned), 16 bytes each, and n_out[g] receives their count, floor((pos + T) / 2400) - floor(pos / 2400); an unmetered stream has
// n_out[g] = 0 and nothing of it is read or written.  Nothing runs when no stream is metered.
// Refused (loudness_launch_refusal, loudness.h) before anything is uploaded or launched.
void launch_loudness(hipStream_t st, LoudnessStage& s, const float* pcm, int G, int T, const int32_t* streams, const int32_t* metered,
                     const int64_t* pos, void* out, const int64_t* out_off, int64_t* n_out);

} // namespace q3
