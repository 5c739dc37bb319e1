// codec_worker.h -- the decoder thread (the reference decodes on a second thread too, engine.rs:495-543): it owns every codec launch, so the ~200
// kernel launches of a chunk never delay the AR stream's.  The scheduler gives it typed tasks and takes completions back (CodecQueue, sched_logic.h).
#pragma once
#include "codec.h"
#include "loudness.h"
#include "sched_logic.h"
#include <atomic>
#include <condition_variable>
#include <mutex>
#include <thread>

namespace q3 {

// A request as the decoder thread sees it.  The scheduler fills the first block before the request's first task is pushed and changes it only
// behind the fence's completion; the second block is the thread's own from the first task to the fence, and the scheduler reads it behind a
// completion (pcm_enq and loud_enq travel in the completion itself).  `cancel` alone changes while tasks are in flight.
struct CodecJob {
    int64_t id = 0;          // TaskHead::req
    bool decode = false;     // [EXT] decoding given frames: its tasks wait in the low queue
    int cs = -1;             // its codec stream
    OutSpec out;             // [EXT] what its PCM is delivered as
    // [EXT] codec preambles: the snapshot and the pinned tail its reset restores; snapshot: it builds a preamble, its fence enqueues a snapshot
    int pre_snap = -1; const float* pre_tail = nullptr; bool snapshot = false;
    std::atomic<bool> cancel{false}; // [EXT] set once by Engine::cancel, never cleared; looked at when the fence runs
    int64_t tsm_native = 0;  // native samples its stream has been given
    size_t pcm_enq = 0;      // delivered samples enqueued: out_delivered(out, tsm_native, .)
    size_t loud_enq = 0;     // [EXT] loudness: rows enqueued, loud_blocks(0, tsm_native) of a metered job
    int snap = -1;           // the snapshot its fence enqueued
    size_t sample_bytes() const { return out_sample_bytes(out); }
    bool stretched() const { return out_kind(out) >= OUT_RATED; }
    // bytes of the samples that become available with n_more native samples more, or (final) with the flush
    size_t bytes_due(int64_t n_more, bool final) const {
        return (size_t)(out_delivered(out, tsm_native + n_more, final) - out_delivered(out, tsm_native, false)) * sample_bytes();
    }
};

class CodecWorker {
public:
    struct Completion { CodecJob* job; hipEvent_t ev; size_t pcm_after; bool fence; size_t loud_after; }; // loud_after: [EXT] loudness rows reached
    // n_lanes HIP streams (consecutive passes overlap with the next AR frames and with each other) and pinned staging of slot_cap native
    // floats for each of n_cs codec streams
    CodecWorker(CodecDecoder* codec, int dev, int n_lanes, int n_cs, size_t slot_cap);
    ~CodecWorker(); // runs what is still queued, joins
    void start() { if (!started_) { started_ = true; thread_ = std::thread([this] { main(); }); } }

    // a request's tasks are reset, chunks, fence, in that order
    void push_reset(CodecJob* j) { push(j, TASK_RESET); }
    void push_chunk(CodecJob* j, const int64_t* codes, int n_codes, bool is_final) { push(j, TASK_CHUNK, codes, n_codes, is_final); }
    void push_fence(CodecJob* j) { push(j, TASK_FENCE); }
    void purge(CodecJob* j);
    // One hand-over: the thread forms no pass until every task of it is queued, and its generating chunks carry one epoch.  Handed over one by
    // one, the thread would start a pass with the chunks that happened to have arrived: which streams share a pass, and with it the GEMM forms
    // a request's samples go through, would depend on the two threads' timing
    struct Handover {
        CodecWorker* w;
        Handover(CodecWorker* w_, bool on) : w(on ? w_ : nullptr) { if (w) { std::lock_guard<std::mutex> lk(w->mu_); w->q_.open(); } }
        ~Handover() { if (w) { { std::lock_guard<std::mutex> lk(w->mu_); w->q_.close(); } w->cv_.notify_all(); } }
        Handover(const Handover&) = delete; Handover& operator=(const Handover&) = delete;
    };
    int pending(); // CodecQueue::pending
    // The oldest completion, its event complete; false when there is none.  Completions of a lane finish in order; keep it simple: FIFO.
    // block: waits 2 ms for one to appear, then for its event; else an event still running is none.  Throws "decoder thread: ..." once the
    // thread has failed
    bool poll_completion(bool block, Completion* out);

    // a stream's staging region, in bytes: slot_cap native floats, and no format needs more bytes per frame than the native one
    size_t slot_bytes() const { return slot_cap_ * sizeof(float); }
    const float* staging(int cs) const { return pcm_pinned_ + (size_t)cs * slot_cap_; }
    unsigned char* stage(const CodecJob& j, size_t add) const; // where the next `add` bytes of j land; throws "pcm staging overflow"
    // [EXT] loudness: a stream's rows {energy, peak}, loud_cap() of them, beside the PCM staging; pinned by the first pass that holds a
    // metered job, nullptr until then.  Read by the scheduler behind a completion with loud_after > 0
    size_t loud_cap() const { return slot_cap_ / Q3_LOUD_BLOCK + 1; }
    const double* loud_staging(int cs) const { return loud_pinned_.load() + (size_t)cs * loud_cap() * 2; }

    // decode-only chunks decoded, and of those the ones that shared a pass with a generating request's chunk; preamble restores
    std::atomic<int64_t> dec_chunks{0}, dec_shared{0}, pre_restores{0};
    long take_codec_calls() { return (long)codec_calls_.exchange(0); } // chunks enqueued since the last take (EngineStats::codec_calls)

private:
    typedef CodecQueue<CodecJob>::Task Task;
    typedef std::vector<Task> Step; // one reset or fence, or the chunks of one pass
    void push(CodecJob* j, TaskKind kind, const int64_t* codes = nullptr, int n_codes = 0, bool is_final = false);
    void main();
    // what a step does on its lane, in this order
    int pick_lane(const Step& s);              // and waits for the lanes the jobs' previous tasks ran on
    void start_stream(int lane, const Step& s); // a reset: zeroes, or [EXT] restores the preamble's snapshot
    void decode_pass(int lane, const Step& s);
    void flush_rate(int lane, const Step& s);   // [EXT] speaking rate, at a fence
    void snapshot_build(int lane, const Step& s); // [EXT] codec preambles, at a build's fence
    void record(int lane, const Step& s);       // the ordering events and the completions

    CodecDecoder* codec_; int dev_;
    std::vector<hipStream_t> st_;
    float* pcm_pinned_ = nullptr; size_t slot_cap_ = 0;
    std::atomic<double*> loud_pinned_{nullptr}; int n_cs_ = 0;
    double* loud_stage(const CodecJob& j, size_t add); // where the next `add` rows of j land; throws "loudness staging overflow"
    std::thread thread_; bool started_ = false, stop_ = false;
    std::mutex mu_; std::condition_variable cv_; // mu_: q_, comp_, err_, stop_
    CodecQueue<CodecJob> q_; std::deque<Completion> comp_; std::string err_;
    std::map<CodecJob*, std::pair<int, hipEvent_t>> last_; int next_lane_ = 0; // thread only: job -> (lane, event after its latest task)
    std::atomic<int64_t> codec_calls_{0};
};

} // namespace q3
