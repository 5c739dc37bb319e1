// codec.h -- streaming codec decoder on device (codes -> 24 kHz PCM), the replacement for the ONNX AudioDecoder
// (/root/reference/src/models/onnx.rs:324-496).  Architecture "Q3TTS-codec-synth" (see DESIGN.md).
#pragma once
#include "q3_common.h"
#include "sched_logic.h"
#include <memory>
#include <string>
#include <vector>

struct q3tts_codec_gemm_desc;
struct q3tts_codec_kernel_desc;

namespace q3 {

struct CodecStateEntry { std::string name; int64_t offset; int rows, cols; }; // one named tensor of a stream's state blob ([rows][cols] f32 at `offset` floats)

class CodecDecoder {
public:
    // DecoderState (onnx.rs:461-496) out of / into the device: flat f32 blob per stream, layout = named history tensors + counters
    std::vector<CodecStateEntry> state_layout() const;
    size_t state_floats() const;
    void state_export(int stream, float* out, size_t n_floats) const; // n_floats must equal state_floats()
    void state_import(int stream, const float* in, size_t n_floats);  // validates the blob size and its trailer before committing
    // n_lanes: independent scratch sets so that decodes of different streams can run concurrently on different HIP streams
    // max_group: how many streams one pass may decode together (decode_group_async)
    CodecDecoder(const std::string& gguf_path, int n_streams, int max_frames_per_call, int n_lanes = 1, int max_group = 1);
    int max_group() const;
    int n_lanes() const;
    ~CodecDecoder();
    int samples_per_frame() const;
    void reset(int stream); // AudioDecoder::create_state (onnx.rs:338-340, 474-495)
    void reset_async(hipStream_t st, int stream); // same, ordered on `st` (call from the thread that issues the decodes)
    // [EXT] codec preambles (q3tts_spec.h): a device-side copy of one stream's whole state.  snapshot_async copies the stream's history slots
    // of every state tensor into a free slot of the snapshot store (one k_hist_copy launch per 48 tensors) and notes its two counters;
    // restore_async copies a snapshot into a stream the same way and sets the stream's counters from it, where reset_async zeroes both.
    // Both are ordered on `st` and synchronise nothing; a slot's buffer is allocated by the first snapshot that takes it.  pcm_tail (optional,
    // Q3_PCM_HIST floats of pinned host memory that stay valid until `st` has passed): the stream will be delivered converted and its converter
    // history starts as these samples.  The caller sees to it that a freed slot's restores have completed before the slot is taken again
    // on another HIP stream.  All three refuse a stream or snapshot out of range and a freed snapshot before anything is launched
    int snapshot_async(hipStream_t st, int stream);
    void restore_async(hipStream_t st, int snapshot, int stream, const float* pcm_tail = nullptr);
    void snapshot_free(int snapshot);
    size_t snapshot_bytes() const; // device bytes of one snapshot
    int snapshots_live() const;
    // codes: host [n_frames][16] (already clamped to [0,2047], engine.rs:515-519); pcm: host, n_frames*spf floats
    int decode(hipStream_t st, int stream, const int64_t* codes, int n_frames, bool is_last, float* pcm);
    // same, but returns right after enqueueing: pcm_pinned must be hipHostMalloc'd and stay valid until `st` is synchronised
    int decode_async(hipStream_t st, int stream, const int64_t* codes, int n_frames, bool is_last, float* pcm_pinned, int lane = 0);
    // G distinct streams, each with n_frames new frames: codes [G][n_frames][16], pcm[g] pinned destinations
    // [EXT] out[g] = what stream g is delivered as (OutSpec, sched_logic.h); NULL, or every entry the default, is the plain call: the same
    // launches, the same copies.  Otherwise, behind the output conv on `st`: one volume launch (volume.hip) rewrites the chunks of the streams
    // with a volume in place; then one launch of each stage that a stream of the pass belongs to (out_kind: convert, pcmout.hip; stretch,
    // tsm.hip; pitch, pitch.hip), and every stream's copy takes the n_out[g] (optional) samples its stage made -- of a stretched or shifted
    // stream those that became available, possibly none -- in 4 or 2 bytes each.  A stage's tables, state store and per-lane buffers are
    // made by the first call that needs it; a reset and a snapshot restore zero a stream's state in all of them.
    // [EXT] loudness: a stream with out[g].loud is metered -- in front of the volume launch one loudness launch (loudness.hip) reads the chunks
    // of the metered streams, and the rows stream g completes are copied to loud[g].rows (LoudDst, sched_logic.h), which it then needs (an
    // unmetered stream's entry is not looked at).  All of it is OutChain::run (out_chain.h) over the routing out_route works out (sched_logic.h)
    int decode_group_async(hipStream_t st, int G, const int* streams, const int64_t* codes, int n_frames, float* const* pcm_pinned, int lane = 0,
                           const OutSpec* out = nullptr, int64_t* n_out = nullptr, const LoudDst* loud = nullptr);
    // ends a stretched or shifted utterance: the hops its last samples still owe go to dst (pinned) and *n_out is their sample count (0 for a
    // stream that was neither since its reset)
    void tsm_flush_async(hipStream_t st, int stream, void* dst, int64_t* n_out, int lane = 0);
    OutputStageStats output_stats() const; // the counters of the output stages and the meter (read by other threads)
    double flops_per_frame() const;
private:
    struct Impl;
    std::unique_ptr<Impl> impl_;
};

// test entry points (include/q3tts.h: q3tts_op_codec_gemm, q3tts_codec_gemm_plan): one codec GEMM, dispatched as the decoder does or forced
void codec_gemm_run(q3tts_codec_gemm_desc* d);
void codec_gemm_plan_only(q3tts_codec_gemm_desc* d); // host only
int codec_gemm_tap_reuse(const q3tts_codec_gemm_desc* d); // host only: 1 = the GEMM d describes runs k_conv_gemm_h3's tap-reusing loop
void codec_kernel_run(q3tts_codec_kernel_desc* d); // q3tts_op_codec_kernel: one non-GEMM kernel as the decoder launches it

} // namespace q3
