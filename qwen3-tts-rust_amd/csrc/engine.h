// engine.h -- the autoregressive generation loop on device: what TtsEngine::run_inference_stream does
// (/root/reference/src/tts/engine.rs:445-656), for many utterances at once.
//
// Execution model: the engine owns `max_batch` sequence slots.  One frame step for all slots is a static
// hipGraph (everything a frame needs -- codes, positions, sampler state, finished flags -- lives on the device).
// A scheduler admits queued requests into free slots (batched multi-sequence prefill), replays the frame graph in
// groups of 4 frames (one streaming step, engine.rs:505-512), retires sequences on EOS / max_steps and hands
// finished 4-frame chunks to a decoder thread (engine.rs:495-543; CodecWorker, codec_worker.h) that runs the codec on its own HIP streams.
// Sampling (greedy and temperature/top-k/top-p, llama/mod.rs:666-776) is on device.
#pragma once
#include "transformer.h"
#include "host_logic.h"
#include "sched_logic.h"
#include "codec.h"
#include "codec_worker.h"
#include <atomic>
#include <condition_variable>
#include <deque>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

namespace q3 {

struct EngineParams {
    std::string model_dir;      // contains <quant dir>/ and onnx/
    std::string quant = "q8_0"; // engine.rs:91-95
    int max_batch = 1;
    int max_prompt = 1024;      // llama/mod.rs:567-581: effective prompt cap of the reference
    int max_steps = Q3_DEFAULT_MAX_STEPS;
    bool load_codec = true;
    bool use_graph = true;
};

struct GenResult {
    std::vector<int32_t> codes; int n_frames = 0;
    std::vector<float> pcm;
    double prefill_ms = 0, first_chunk_ms = 0, total_ms = 0;
};

struct EngineStats { // accumulated since reset
    double frame_loop_ms = 0; long frames = 0;   // device time of the AR frame loop (HIP events), all sequences
    double gemv_ms = 0; long gemv_launches = 0; double gemv_bytes = 0; // instrumented (eager) leg only: GEMV family except ...
    double gu_ms = 0; long gu_launches = 0; double gu_bytes = 0;       // ... the talker's gate/up kernel, timed on its own
    double codec_ms = 0; long codec_calls = 0;
    double prefill_ms = 0;
    long steps = 0; double slot_frames = 0;      // scheduler: frame-group launches, sum of graph widths x frames (occupancy)
    long graph_frames = 0;                       // frame-graph replays
};

struct ReqStatus {
    int state = REQ_QUEUED; int n_frames = 0; int64_t n_pcm = 0; // frames emitted / PCM samples decoded so far
    double queue_ms = 0, prefill_ms = 0, first_chunk_ms = 0, total_ms = 0;
    std::string error; // REQ_FAILED: what the scheduler / decoder thread reported
};

struct Voice { // a registered voice: preset embedding or clone material (engine.rs:390-435, voice_file.rs:5-22)
    std::vector<float> spk_emb; std::vector<int32_t> ref_codes, ref_text_ids;
    int preamble = -1; // [EXT] codec preambles: what requests of the text forms with this voice are primed with (mu_)
    int stem = -1;     // [EXT] prompt stems: what applies to requests of the text forms with this voice (mu_)
};


class Engine {
public:
    explicit Engine(const EngineParams& p);
    ~Engine();
    // blocking convenience: submit all, run the scheduler until they are done (requests beyond max_batch queue up)
    void generate_batch(const std::vector<GenRequest>& reqs, std::vector<GenResult>& out, bool want_pcm);

    // ---- continuous-batching scheduler ----
    // may_record = false: the request never records log-probabilities, whatever the engine's flag says (generate_batch)
    int64_t submit(const GenRequest& r, bool want_pcm, bool copy_prompt = true, bool may_record = true); // thread-safe
    // [EXT] token log-probabilities (q3tts_spec.h): requests submitted from now on record 17 floats per frame.  Thread-safe; the first
    // enable allocates the device buffers ([B][max_steps + 1][17] rows, [15][B][2048] predictor logits); refused under Q3_SPEC=ggml
    void set_logprobs(bool on);
    // rows [frame_off, frame_off + max_frames) available now, [got][17]; the row count is fetch()'s; throws for a request that does not record
    void fetch_logprobs(int64_t id, float* out, int frame_off, int max_frames, int* got_frames);
    // [EXT] live text append, thread-safe and free of HIP calls (the scheduler uploads): 0 appended, 1 the request no longer takes text
    // (finished, done or failed); throws for an unknown id, a request not submitted open, a closed trail or a total beyond max_prompt
    int append_trail(int64_t id, const int32_t* ids, int n, bool close);
    void trail_progress(int64_t id, int* n_appended, int* n_consumed, bool* closed);
    // [EXT] stops a request wherever it is; thread-safe and free of HIP calls (the scheduler retires the slot between two frame groups):
    // 0 cancellation requested, 1 the request had already ended; throws for an unknown id
    int cancel(int64_t id);
    // [EXT] scoring given frames (q3tts_spec.h "scoring"): teacher-forced log-probabilities of codes [n][16] behind prompt [n_prompt][2048] and
    // optional closed trailing ids.  Queued like any request; ends REQ_DONE with n frames (the given codes) and their [n][17] rows, no PCM.
    // Thread-safe; the first call allocates the scoring state; throws score_refusal's reason before anything is queued
    int64_t submit_score(const float* prompt, int n_prompt, const int32_t* trail, int n_trail, const int32_t* codes, int n);
    int score_width() const { return score_w_; } // frames per predictor scoring pass
    // [EXT] candidate sets (q3tts_spec.h "candidate sets"): n requests of one prompt, candidate i exactly submit() of g with seed seeds[i] (g's own
    // seed is ignored; no prefix, no open trail).  The prompt and trail are copied once; the members are queued consecutively, admitted in one
    // wave, prefilled once and forked (k_kv_fork).  n = 1 is submit().  Thread-safe; throws candidates_refusal's reason or validate()'s before
    // anything is queued
    void submit_candidates(const GenRequest& g, bool want_pcm, const uint64_t* seeds, int n, int64_t* req_ids);
    // sets of two or more candidates accepted, prompt rows whose prefill the forks replaced, KV pages k_kv_fork copied (per destination)
    void candidate_stats(int64_t* sets, int64_t* rows_saved, int64_t* pages_copied) const {
        *sets = cand_sets_.load(); *rows_saved = cand_rows_saved_.load(); *pages_copied = cand_pages_.load();
    }
    // [EXT] decoding given frames (q3tts_spec.h "decoding given frames"): the PCM of codes [n][16], through the engine's codec.  The request
    // waits in a queue of its own, takes a codec stream (at most decode_width() such requests hold one) and nothing of the talker: no slot, no
    // KV pages, no prefill, no frame.  QUEUED until it holds a stream, then DRAINING, DONE behind its fence; its frames are the given codes
    // from submission on.  Thread-safe and free of HIP calls; throws decode_refusal's reason before anything is queued
    int64_t submit_decode(const int32_t* codes, int n);
    int decode_width() const { return decode_w_; }
    // decode-only requests accepted, their chunks decoded, and of those the chunks that shared a pass with a generating request's chunk
    void decode_stats(int64_t* requests, int64_t* chunks, int64_t* chunks_shared) const {
        *requests = dec_reqs_.load(); *chunks = worker_ ? worker_->dec_chunks.load() : 0; *chunks_shared = worker_ ? worker_->dec_shared.load() : 0;
    }
    // [EXT] output formats (q3tts_spec.h "output formats"): requests submitted from now on with want_pcm deliver this format (NULL: native);
    // read once per request at submit and once per candidate set; generate_batch always delivers native.  Thread-safe, no HIP calls; throws
    // pcm_format_refusal's reason.  fetch() serves f32 requests at their rate and refuses a PCM pointer on an s16 request; fetch_pcm16 is
    // its PCM half for s16 requests and refuses an f32 one.  poll()'s n_pcm counts samples of the request's format
    void set_output_format(const q3tts_pcm_format* f);
    q3tts_pcm_format request_format(int64_t id);
    void fetch_pcm16(int64_t id, int16_t* out, int64_t off, int64_t cap, int64_t* got);
    OutputStageStats output_stats() const; // the counters of the four output stages; all zeros without a codec
    // [EXT] speaking rate (q3tts_spec.h "speaking rate"): requests submitted from now on with want_pcm are spoken at pct percent of the native
    // tempo (100: off); read once per request at submit and once per candidate set; generate_batch, scoring and preamble builds are never
    // stretched.  Thread-safe, no HIP calls; throws for a rate outside [50, 200] or an engine without a codec.  A submit with a rate throws
    // tsm_submit_refusal's reason.  poll()'s n_pcm and the fetch offsets count delivered samples
    void set_speech_rate(int pct);
    int request_speech_rate(int64_t id);
    // [EXT] pitch (q3tts_spec.h "pitch"): requests submitted from now on with want_pcm have their pitch shifted to pct percent (100: off), with
    // or without a rate; read with the rate, once per request at submit and once per candidate set, wherever the rate is read.  Thread-safe, no
    // HIP calls; throws for a pitch outside [50, 200] or an engine without a codec.  The pair is judged at submit: a submit throws
    // pitch_submit_refusal's reason before anything is queued
    void set_pitch(int pct);
    int request_pitch(int64_t id);
    // [EXT] volume (q3tts_spec.h "volume"): requests submitted from now on with want_pcm have a gain of db10 tenths of a dB behind a look-ahead
    // limiter (0: off), in front of whatever format, rate or pitch they have; read with the rate and the pitch, wherever those are read.
    // Thread-safe, no HIP calls; throws volume_submit_refusal's reason for a volume outside [-400, 200] or an engine without a codec
    void set_volume(int db10);
    int request_volume(int64_t id);
    // [EXT] loudness (q3tts_spec.h "loudness"): requests submitted from now on with want_pcm are metered -- the K-weighted energy and the
    // sample peak of every 100 ms block of their native stream, whatever they are delivered as; read with the other output settings, wherever
    // those are read.  Thread-safe, no HIP calls; throws on an engine without a codec.  fetch_loudness: rows [block_off, block_off + max_blocks)
    // that are available now ({energy, peak}, two doubles each; they grow with poll()'s n_pcm); throws for a request that is not metered
    void set_loudness(bool on);
    bool request_metered(int64_t id);
    void fetch_loudness(int64_t id, double* out, int64_t block_off, int64_t max_blocks, int64_t* got);
    // [EXT] codec preambles (q3tts_spec.h "codec preambles"): a codec stream state to start requests from, built once from codes [n][16] like a
    // decode-only request (decode_q_, a codec stream, reset / chunks / fence through the decoder thread, which enqueues the snapshot at the
    // fence) and kept on the device.  create: thread-safe, no HIP calls; throws preamble_refusal's reason before anything is queued.  The
    // setters take a READY preamble only (HeldTable::set_refusal).  submit() / submit_candidates() / submit_decode() read the engine-level
    // setting once per request / set; a request with PCM holds a reference from submit to its end, and the `reset` task of a primed request
    // restores the snapshot (and, when it converts, uploads the preamble's last Q3_PCM_HIST samples) where it zeroed the stream
    int preamble_create(const int32_t* codes, int n);
    void preamble_poll(int id, int* state, int* n_frames);
    bool preamble_wait(int id, double timeout_ms); // true once READY or FAILED; drives step() itself when no driver thread is running
    void preamble_release(int id);                 // the creator's reference
    void set_voice_preamble(int voice_id, int preamble_id); // -1: none
    int voice_preamble(int voice_id);
    void set_preamble(int preamble_id);                     // -1: none
    int request_preamble(int64_t id);
    void preamble_stats(int64_t* built, int64_t* restores, int64_t* bytes_per_snapshot) const;
    // [EXT] prompt stems (q3tts_spec.h "prompt stems"): n prompt rows and their talker K/V at positions 0 .. n-1, built once by an internal wave
    // member (a slot for one wave, no head) whose pages the save launch copies into the stem's own device store, and restored by one launch
    // per wave in front of the first chunk.  create: thread-safe, no HIP calls (the scheduler allocates the store); throws stem_refusal's
    // reason before anything is queued.  The setters take a READY stem only.  submit() / submit_candidates() read the engine-level setting
    // once per request / set and apply the take rule; a request that took a stem holds a reference from submit to its end
    int stem_create(const float* rows, int n);
    void stem_poll(int id, int* state, int* n_rows);
    bool stem_wait(int id, double timeout_ms); // true once READY or FAILED; drives step() itself when no driver thread is running
    void stem_release(int id);                 // the creator's reference
    void set_voice_stem(int voice_id, int stem_id); // -1: none
    int voice_stem(int voice_id);
    void set_stem(int stem_id);                     // -1: none
    void request_stem(int64_t id, int* stem_id, int* rows_reused); // -1 / 0: the request took none
    struct StemStats { int64_t built = 0, restores = 0, rows_skipped = 0, pages_copied = 0, mismatches = 0, bytes_held = 0; };
    StemStats stem_stats() const;
    bool step();                                  // one scheduling iteration on the calling thread; false when idle
    ReqStatus poll(int64_t id);                   // thread-safe snapshot
    // copies frames [frame_off, ...) and PCM samples [pcm_off, ...) that are available now; returns counts
    void fetch(int64_t id, int32_t* codes, int frame_off, int max_frames, float* pcm, int64_t pcm_off, int64_t pcm_cap,
               int* got_frames, int64_t* got_pcm);
    bool wait(int64_t id, double timeout_ms);     // drives step() itself when no driver thread is running
    void release(int64_t id);
    void start_driver();                          // background thread looping step()
    void stop_driver();
    int register_voice(const Voice& v);
    const Voice& voice(int id) const;

    const HostAssets& assets() const { return *assets_; }
    Transformer& talker() { return *talker_; }
    Transformer& predictor() { return *predictor_; }
    CodecDecoder* codec() { return codec_.get(); }
    EngineStats stats; void reset_stats() { read_stats(); stats = EngineStats(); }
    const EngineStats& read_stats() { if (worker_) stats.codec_calls += worker_->take_codec_calls(); return stats; } // the decoder thread counts its own
    void set_instrument(bool on) { instrument_ = on; }
    size_t bytes_per_frame_step(int batch, double mean_ctx) const; // algorithmic HBM bytes of one batched frame step
    size_t pred_table_bytes() const { return pred_table_bytes_; }  // the predictor's layer-0 q/k/v table (0 = off: Q3_PRED_L0_TABLE=0 or Q3_SPEC=ggml)
    hipStream_t stream() const { return st_; }
    int max_batch() const { return B_; }
    int device() const { return dev_; }

private:
    struct Req;
    struct FrameGraph { // one captured frame step for `width` slots (+ the pass-A routing tables of that width)
        int width = 0; hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr;
        DevBuf<int32_t> seqA, slotA, posA;
    };
    void record_frame(FrameGraph& fg, FrameVariant v); // enqueue one frame step for fg.width slots on st_
    FrameGraph& frame_graph(int width, FrameVariant v, bool capture);
    void validate(const GenRequest& g) const; // prompt and max_steps ranges, then the options
    void ensure_text_stream(); // first request with trailing ids: text table + per-slot id rows go to the device
    Req& req(int64_t id);                                             // throws for an unknown id (mu_ held)
    int64_t enqueue(std::unique_ptr<Req> r, std::deque<Req*>& queue); // a submission's tail: id, reqs_, the queue, the wake-up (mu_ held)
    // Admission.  A wave is prefilled by one walk, prefill_wave, on one of two lanes.  A PrefillLane holds what the two forms differ in: the
    // talker context, the stream, the chunk width, the device buffers of one chunk and the pinned staging its rows and tables go up through.
    //   ar_  in line, on the AR stream (an idle engine, a one-slot engine, Q3_ASYNC_PREFILL=0): the talker itself, chunks of its launch width,
    //        the scheduler's staging arena, which waits for the stream and starts over when it is full.  The heads of the last prompt tokens
    //        draw code_0 straight into the live arrays (head_live), so go_live() runs before the walk
    //   pf_  asynchronously, beside running slots (async_pf_ only): a second talker context over the same weights on a stream of its own,
    //        chunks of pf_chunk_ rows, an arena that holds a whole wave and never waits.  The heads leave logits and hidden rows in d_pf_logits_ /
    //        d_pf_hidden_ (head_staged); activate() brings the wave in between two frame groups once pf_done_ has completed
    struct PrefillLane {
        Transformer* talker = nullptr; hipStream_t st = nullptr; int chunk = 0; bool async = false;
        DevBuf<float> d_rows; DevBuf<int32_t> d_seq, d_slot, d_pos; // one chunk: its input rows, seq / slot / pos [4] per token
        DevBuf<int32_t> d_codes, d_ids, d_fork_dst;                 // [EXT] resume: codes / trailing ids of its feedback rows; candidate sets: a wave's fork destinations
        DevBuf<StemJob> d_stem_jobs; DevBuf<int32_t> d_stem_slots;  // [EXT] prompt stems: a wave's restore jobs [B] then its save jobs [B], and their slot lists
        unsigned char* arena = nullptr; StageCursor cur;            // pinned staging
    };
    void lane_alloc(PrefillLane& L, Transformer* talker, hipStream_t st, int chunk, bool async, size_t arena_bytes);
    void* stage_take(PrefillLane& L, size_t bytes);
    void prefill_wave(PrefillLane& L, const std::vector<Req*>& wave, bool sampled); // sampled: of head_live, some slot draws with a temperature
    void head_live(Req* lead, const std::vector<Req*>& rest, int tok, bool sampled);
    void head_staged(Req* lead, const std::vector<Req*>& rest, int tok);
    SampleArgs first_head_args(const float* logits_row, int b) const; // slot b's first draw from a prefill head's logits row
    // [EXT] resume (q3tts_spec.h): the prefix frames' feedback rows of a prefill chunk, made on the device; the first head's history
    void feedback_rows(hipStream_t st, const std::vector<Req*>& batch, const std::vector<FbRun>& fb, int32_t* hc, int32_t* d_codes, int32_t* d_ids, float* d_rows);
    void head_history(SampleArgs& sa, int b) const;
    static bool resumed_penalised(const GenRequest& g) { return g.n_prefix > 0 && g.opts.penalised(); }
    // [EXT] log-probabilities: columns 0 and 16 of slot b's row `row` from the talker logits row a prefill head wrote and the key its sampler drew
    void first_head_logprobs(hipStream_t st, const float* logits_row, int b, int row);
    // [EXT] scoring: the state's one-time allocation; the talker heads and predictor passes of a prefill chunk's score rows, on the chunk's
    // stream (h_codes: pinned, 64 B per row of the chunk); the rows' way to the host and the end of the requests (st_ idle)
    void ensure_score();
    void score_chunk(hipStream_t st, Transformer& talker, const std::vector<Req*>& batch, const std::vector<ScoreRun>& runs, int32_t* h_codes);
    void finish_scores(const std::vector<Req*>& scores);
    // [EXT] candidate sets: the members of a wave that are prefilled (`lead`: everything but the later members of a set, in wave order) and per
    // lead its set's other members; the forks of a wave, enqueued on `st` behind its last chunk (h_dst: pinned, d_dst: device, B ints each)
    static void split_sets(const std::vector<Req*>& batch, std::vector<Req*>& lead, std::vector<std::vector<Req*>>& rest);
    void fork_sets(hipStream_t st, const std::vector<Req*>& lead, const std::vector<std::vector<Req*>>& rest, int32_t* h_dst, int32_t* d_dst);
    static int kv_positions(const GenRequest& g, bool score) { return score ? g.n_prompt + g.n_prefix + 1 : g.n_prompt + g.max_steps + 1; }
    // [EXT] prompt stems: the restores of a wave, one launch on the lane's stream behind the page-table rows and in front of the first chunk;
    // the saves of its builds, one launch behind the last chunk; the stores of the wave's builds (scheduler thread, capture_mutex()); the end
    // of the builds (the wave's prefill complete); the stores nobody holds any more (scheduler thread)
    void restore_stems(PrefillLane& L, const std::vector<Req*>& lead);
    void save_stems(PrefillLane& L, const std::vector<Req*>& lead);
    void alloc_stem_stores(const std::vector<Req*>& wave);
    void finish_builds(const std::vector<Req*>& builds);
    void free_stem_stores();
    void prefill_async(const std::vector<Req*>& wave); // the asynchronous wave's start: KV pages, events, the walk on pf_, pf_batch_
    void go_live(const std::vector<Req*>& batch);      // slot state of a wave's requests (no score request among them) goes live, on st_
    void activate();                                   // the asynchronous wave's completion
    void admit_decodes();     // [EXT] decode-only requests take free codec streams, after admit()
    // their reset, chunks and fence go to the low queue: at once when the step runs no frame group, else together with the chunks the group
    // produced (run_group), so that both kinds meet in the decoder thread's queues and share passes
    void enqueue_decodes();
    void admit(bool stalled); // stalled: every live slot waits for text (the admission quantum is not waited for)
    void run_group();
    void collect_appends();   // scheduler: new ids / close flags of live open slots into the slot table (upload in run_group)
    void collect_cancels();   // scheduler: retires the slots of cancelled requests, drops the unstarted chunks of draining ones
    void harvest(bool block);
    void retire(Req* r, bool flush_tail); // the slot leaves the batch: EOS / max_steps (tail flushed) or a cancel (tail and unstarted chunks dropped)
    int64_t copy_pcm(const Req& r, void* out, int64_t off, int64_t cap) const;
    // [EXT] output formats, speaking rate, pitch, volume: the engine-level settings as one record (OutSpec, sched_logic.h).  A setter writes its
    // field and take_out reads the whole record, both under out_mu_, so a request's settings are a record that stood at some instant.  A
    // request with PCM takes the engine's record, or `given` -- what the first member of its candidate set took -- if its length allows it
    // (out_submit_refusal: throws before anything is queued)
    OutSpec out_; mutable std::mutex out_mu_;
    void take_out(Req* r, int max_steps, const OutSpec* given = nullptr) const;
    void upload_slot_state(); // the whole slot table, routing rows derived first, in one copy
    // All scheduler transfers go through a pinned arena on the AR stream: the engine's streams are non-blocking, so nothing the
    // scheduler does waits for the codec lanes (a synchronous hipMemcpy on the null stream would).
    void* stage_alloc(size_t bytes) { return stage_take(ar_, bytes); }
    void h2d(void* dst, const void* src, size_t bytes);            // async on st_, source copied into the arena first
    void* d2h_begin(const void* src, size_t bytes);                // async on st_ into the arena; valid after the next sync of st_

    EngineParams p_;
    hipStream_t st_ = nullptr; int dev_ = 0;
    std::unique_ptr<HostAssets> assets_;
    std::unique_ptr<Transformer> talker_, predictor_, talker_pf_;
    hipStream_t st_pf_ = nullptr; PrefillLane ar_, pf_;
    DevBuf<float> d_pf_logits_, d_pf_hidden_; // [B] rows: what head_staged leaves for activate()
    std::vector<Req*> pf_batch_; hipEvent_t pf_done_ = nullptr, pf_e0_ = nullptr; bool async_pf_ = false; int n_prefilling_ = 0;
    int pf_chunk_ = 256; // rows of one prompt chunk of the asynchronous lane, and the least the in-line lane takes (512: Q8_0 talker, wide GEMM forms)
    std::unique_ptr<KvPool> kv_t_, kv_p_;
    std::unique_ptr<CodecDecoder> codec_;
    std::unique_ptr<CodecWorker> worker_; // the decoder thread with its lanes, queues and PCM staging; with a codec only
    // device assets
    DevBuf<float> d_codec_tab_[16]; DevBuf<float> d_proj_tab_[16];
    DevBuf<float> d_qkv0_tab_[16]; bool pred_l0_table_ = false; size_t pred_table_bytes_ = 0; // Q_q[c]: the predictor's layer-0 q/k/v of P_q[c], q = 1..14
    DevBuf<float> d_proj_wt_, d_proj_wblk_, d_proj_b_, d_tts_pad_;
    DevBuf<const float*> d_tab_ptrs_; DevBuf<int64_t> d_tab_rows_;
    int dP_ = 0;
    // per-slot state: the mirrored scalars (slot_req_[b] set = reserved; slots_.live[b] = stepping inside the frame graph) ...
    int B_ = 0; SlotTable slots_; DevBuf<uint32_t> d_slots_; bool slot_dirty_ = false; // dirty: the host block changed since upload_slot_state
    int32_t* di(SlotField f) const { return slots_.di(f); } float* df(SlotField f) const { return slots_.df(f); }
    // ... and what only the device keeps: code history, argmax keys ([B][16] codes of this frame, [B] code_0 of the next), the ChaCha12
    // keys and draw counters of the talker sampler and of the [EXT] predictor sampler, the predictor logits rows
    DevBuf<int32_t> d_hist_; DevBuf<q3_u64> d_keys_, d_next_key0_;
    DevBuf<uint32_t> d_rngkey_, d_draws_, d_prngkey_, d_pdraws_; DevBuf<float> d_plogits_;
    DevBuf<int32_t> d_pseq_, d_pslot_, d_ppos_;
    DevBuf<float> d_tlogits_, d_thidden_, d_pin_, d_fb_;
    int64_t kv_rows_ = 0; // positions a slot's KV pages hold
    int hist_stride_ = 0, tl_stride_ = 0;
    // [EXT] streaming-text state, allocated by the first request with n_trail > 0: the text table, [B][max_prompt] trailing ids
    DevBuf<float> d_text_; DevBuf<int32_t> d_trail_; int64_t text_rows_ = 0;
    std::mutex text_mu_; bool text_ready_ = false; // text_ready_ is written under text_mu_ and capture_mutex()
    // [EXT] live text append: the stall save area ([B][2048] hidden rows, [B][2] draw counters), allocated with the above
    DevBuf<float> d_stall_hidden_; DevBuf<uint32_t> d_stall_draws_;
    // [EXT] token log-probabilities, allocated when recording is first enabled: d_lp_ [B][lp_rows_][17] (row f = frame f; one row past
    // max_steps takes the last frame's talker columns), d_plp_ [15][B][2048] the predictor heads' logits of one frame, d_lp_rec_ [B] the
    // slot records.  lp_on_: what submit() reads; lp_ready_ is written under lp_mu_ and capture_mutex()
    DevBuf<float> d_lp_, d_plp_; DevBuf<int32_t> d_lp_rec_; int lp_rows_ = 0;
    std::mutex lp_mu_; std::atomic<bool> lp_on_{false}, lp_ready_{false};
    // [EXT] scoring given frames, allocated by the first submit_score: a second predictor context over the shared weights (16 W tokens a pass)
    // with W one-page sequences of its own, routing tables for every pass width F <= W (token p*F + f: sequence f, position p; the tables of
    // width F start at 16 * F(F-1)/2), the 15 pre-projected table pointers, and per prefill chunk the talker logits / hidden rows / codes of
    // its score rows.  d_sc_out_ [B][max_steps][17]: slot b's rows until finish_scores takes them.  Written under sc_mu_ and capture_mutex()
    std::unique_ptr<Transformer> pred_sc_; std::unique_ptr<KvPool> kv_sc_; int score_w_ = 32;
    DevBuf<int32_t> d_sc_seq_, d_sc_slot_, d_sc_pos_, d_sc_codes_; DevBuf<const float*> d_sc_tabs_; DevBuf<int64_t> d_sc_tab_rows_;
    DevBuf<float> d_sc_tlogits_, d_sc_hidden_, d_sc_hproj_, d_sc_in_, d_sc_plogits_, d_sc_out_;
    std::mutex sc_mu_; std::atomic<bool> sc_ready_{false};
    // [EXT] candidate sets: the set ids (mu_), the counters
    int64_t next_set_ = 1;
    std::atomic<int64_t> cand_sets_{0}, cand_rows_saved_{0}, cand_pages_{0};
    std::map<int, std::unique_ptr<FrameGraph>> graphs_; // key = FrameVariant::key(width)
    bool instrument_ = false; bool pred_identity_pages_ = false;
    std::vector<std::vector<int32_t>> h_pend_; std::vector<int> h_pend_off_; // appended ids not yet on the device: ids [off, off+size)
    // scheduler state
    std::mutex mu_; std::condition_variable cv_;
    std::mutex step_mu_;               // step() is driven by one thread at a time (driver thread, wait() callers, generate_batch)
    std::map<int64_t, std::unique_ptr<Req>> reqs_;
    std::deque<Req*> pending_;
    std::vector<Req*> slot_req_;
    std::vector<int> cs_free_;          // free codec streams
    int64_t next_id_ = 1;
    int n_active_ = 0, n_draining_ = 0;
    // [EXT] decoding given frames: the queue decode-only requests wait in for a codec stream, how many hold one (they count in n_draining_
    // too), the limit, and the counters
    std::deque<Req*> decode_q_; int n_decoding_ = 0, decode_w_ = 0;
    std::vector<Req*> dec_admitted_;    // admitted in this step, tasks not yet enqueued (scheduler thread only)
    std::atomic<int64_t> dec_reqs_{0};
    // [EXT] codec preambles and prompt stems (all under mu_) live in one HeldTable each (sched_logic.h): the live objects by id, the next id,
    // the engine-level setting and every count of who holds what are the table's.  The engine keeps what the two kinds differ in: what an
    // object owns (its payload) and how a recycled payload is disposed of (recycled()).
    //   preamble  its snapshot and its pinned tail ([Q3TTS_MAX_PREAMBLES][Q3_PCM_HIST] floats, allocated with the codec's staging; free entries
    //             in pre_tail_free_); both go back in place, which is host bookkeeping only
    //   stem      its rows, its device store and the store's bytes; the store goes to stem_garbage_ for the scheduler thread to free (no HIP
    //             call in a caller's thread), which is woken
    struct PreHeld { int snap = -1, tail = -1; };
    struct StemHeld { std::shared_ptr<const std::vector<float>> rows; uint16_t* store = nullptr; int64_t bytes = 0; };
    HeldTable<PreHeld> pres_{"preamble"}; HeldTable<StemHeld> stems_{"stem"};
    float* pre_tails_ = nullptr; std::vector<int> pre_tail_free_;
    std::vector<std::pair<uint16_t*, int64_t>> stem_garbage_;
    std::atomic<int64_t> pre_built_{0};
    std::atomic<int64_t> stem_built_{0}, stem_restores_{0}, stem_rows_{0}, stem_pages_{0}, stem_miss_{0}, stem_bytes_{0};
    void recycled(const std::optional<PreHeld>& p);  // nothing when the table handed nothing back (mu_ held, as everything below)
    void recycled(const std::optional<StemHeld>& s);
    void pre_attach(Req* r, int pid);   // r is primed with READY preamble pid and holds it
    void stem_match(Req* const* rs, int n_reqs, int asked); // the take rule at submit: the requests take the stem and hold it, or run plain (takes mu_ itself)
    void drop_held(Req* r);             // r has ended, or never ran: the preamble and the stem it holds
    void end_build(Req* r);             // the hidden request of a finished build is nobody's to release
    // what the public twins above are one call of each (they take mu_ themselves); field: &Voice::preamble / &Voice::stem, null = the engine level
    template <class T> void held_poll(T& tab, int id, int* state, int* n);
    template <class T> bool held_wait(T& tab, int id, double timeout_ms);
    template <class T> void held_release(T& tab, int id);
    template <class T> void held_set(T& tab, int Voice::*field, int voice_id, int id);
    int voice_setting(int Voice::*field, int voice_id);
    bool trail_dirty_ = false;          // an append arrived since the scheduler last looked (mu_)
    std::vector<int64_t> cancel_ids_;   // cancelled requests the scheduler has not dealt with yet (mu_)
    uint64_t wake_ = 0;                 // bumped by every submit / append / cancel: a driver idling on stalled slots sleeps until it changes (mu_)
    bool stalled_idle_ = false;         // the last step() ran nothing: every live slot waits for text and nothing else is in flight
    std::vector<Voice> voices_;
    std::thread driver_; bool driver_on_ = false, driver_stop_ = false;
    LaunchTimer timer_, timer_gu_;
};

} // namespace q3
