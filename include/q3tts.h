/*
 * q3tts.h -- C ABI of the MI355X-native Qwen3-TTS engine ("Boundary B").
 *
 * This is what the reference's `src/tts` layer binds instead of llama.cpp + ONNX Runtime:
 *   q3tts_engine_create      <- TtsEngine::new                (/root/reference/src/tts/engine.rs:84-169)
 *   q3tts_generate_batch     <- TtsEngine::run_inference_stream (engine.rs:445-656), batched over requests
 *   q3tts_prompt_*           <- PromptBuilder::{build_core, build_clone_prompt} (src/tts/prompt.rs:28-277)
 *   q3tts_sampler_*          <- LlamaSampler::{new, greedy, sample} (src/models/llama/mod.rs:627-776)
 *   q3tts_chunker_*          <- decoder-thread chunker (engine.rs:495-543)
 *   q3tts_decoder_*          <- AudioDecoder::{load, create_state, decode} (src/models/onnx.rs:324-496)
 *   q3tts_assets_*           <- Assets::{load, project, get_codec_embedding, get_text_embedding} (src/assets_manager.rs)
 *   q3tts_mel                <- SpeakerEncoder::compute_mel (src/models/onnx.rs:167-320)
 * "Boundary A", the 28 llama_* symbols the unmodified reference dlopens, is declared in q3tts_llama.h.
 *
 * Rules: plain pointers and sizes, caller-owned buffers, int status (0 = ok, like llama_decode), no
 * exceptions/aborts across the ABI; q3tts_last_error() returns the thread's last message.
 * The HIP path is the only path: with no usable GPU the compute entry points return an error.
 */
#ifndef Q3TTS_H
#define Q3TTS_H
#include <stdint.h>
#include <stddef.h>
#include "q3tts_spec.h"   /* q3tts_pcm_format ("output formats") */
#ifdef __cplusplus
extern "C" {
#endif

#define Q3TTS_OK 0
#define Q3TTS_ERR -1

const char* q3tts_last_error(void);
int q3tts_version(void);
int q3tts_device_count(void); /* visible HIP devices (0 when none) */

/* ---- SamplerConfig (engine.rs:13-45) ---- */
typedef struct q3tts_sampler_config {
    float temperature; /* default 0.7, <= 0 = greedy */
    int32_t top_k;     /* default 40, 0 = disabled   */
    float top_p;       /* default 0.9, 1.0 = disabled */
    int32_t has_seed;  /* 0 => wall-clock nanoseconds (engine.rs:473-478) */
    uint64_t seed;
} q3tts_sampler_config;
void q3tts_sampler_config_default(q3tts_sampler_config* c);

/* ---- generation controls beyond the reference [EXT] (q3tts_spec.h: definitions) ----
 * Upstream (transformers' Qwen3-Omni talker) decodes with repetition_penalty 1.05 and samples the 15 residual codes with top_k 50 /
 * top_p 0.8 whenever the talker samples.  The defaults below reproduce the reference: no penalty, greedy code predictor. */
typedef struct q3tts_gen_options {
    float repetition_penalty;      /* talker code_0; 1.0 = off (reference); must be finite and > 0 */
    float predictor_temperature;   /* <= 0: greedy predictor (reference) */
    int32_t predictor_top_k;       /* 0 = disabled; >= 0 */
    float predictor_top_p;         /* 1.0 = disabled; in (0, 1] */
} q3tts_gen_options;
void q3tts_gen_options_default(q3tts_gen_options* o);

/* ---- engine ---- */
typedef struct q3tts_engine q3tts_engine;
typedef struct q3tts_engine_params {
    const char* model_dir; /* holds gguf*, onnx/ (engine.rs:91-124) */
    const char* quant;     /* "q8_0" | "q5_k_m" | "none" ... */
    int32_t device;        /* HIP device ordinal */
    int32_t max_batch;     /* lock-stepped sequences per step */
    int32_t max_prompt;    /* <= 1024 (reference's effective cap, llama/mod.rs:567-581) */
    int32_t max_steps;     /* default 512 (engine.rs:152) */
    int32_t load_codec;    /* 0: codes only */
    int32_t use_graph;     /* 1: hipGraph frame replay */
} q3tts_engine_params;
void q3tts_engine_params_default(q3tts_engine_params* p);
int q3tts_engine_create(const q3tts_engine_params* p, q3tts_engine** out);
void q3tts_engine_destroy(q3tts_engine* e);

typedef struct q3tts_request {
    const float* prompt;   /* [n_prompt][2048] f32 embedding rows (PromptData.embd) */
    int32_t n_prompt;
    q3tts_sampler_config sampler;
    int32_t max_steps;
    int32_t mask_eos;      /* test/bench knob: never emit EOS (fixed-length runs) */
    int32_t* codes_out;    /* capacity max_steps*16 */
    float* pcm_out;        /* capacity pcm_capacity floats (may be NULL) */
    int64_t pcm_capacity;
    /* results */
    int32_t n_frames;
    int64_t n_pcm;
    double prefill_ms, first_chunk_ms, total_ms;
} q3tts_request;
/* runs all requests to completion in lock step (request-level batching) */
int q3tts_generate_batch(q3tts_engine* e, q3tts_request* reqs, int32_t n_reqs, int32_t want_pcm);
/* the same with q3tts_gen_options: opts is NULL (defaults for every request) or an array parallel to reqs; invalid options fail the call
 * before anything is queued */
int q3tts_generate_batch_ex(q3tts_engine* e, q3tts_request* reqs, int32_t n_reqs, int32_t want_pcm, const q3tts_gen_options* opts);
/* [EXT] streaming-text talker input (q3tts_spec.h): trail_ids[i] / n_trail[i] are request i's trailing text ids (each n_trail[i] in
 * [0, max_prompt], ids non-NULL when n_trail[i] > 0); n_trail NULL = none for every request; opts as in _ex */
int q3tts_generate_batch_trailing(q3tts_engine* e, q3tts_request* reqs, int32_t n_reqs, int32_t want_pcm, const q3tts_gen_options* opts,
                                  const int32_t* const* trail_ids, const int32_t* n_trail);

typedef struct q3tts_stats {
    double frame_loop_ms; int64_t frames; double prefill_ms;
    double gemv_ms; int64_t gemv_launches; double gemv_bytes; /* instrumented leg only */
    double codec_ms; int64_t codec_calls;
    double talker_weight_bytes, predictor_weight_bytes, kv_bytes_per_token;
    double gu_ms; int64_t gu_launches; double gu_bytes;       /* talker gate/up kernel alone (instrumented leg) */
    int64_t sched_steps; double slot_frames;                  /* scheduler: frame groups launched, sum of graph width x frames */
    int64_t graph_frames;                                     /* frame-graph replays (each advances every active slot by one frame) */
} q3tts_stats;
int q3tts_engine_stats(q3tts_engine* e, q3tts_stats* out);
void q3tts_engine_reset_stats(q3tts_engine* e);
void q3tts_engine_set_instrument(q3tts_engine* e, int32_t on);
double q3tts_engine_bytes_per_step(q3tts_engine* e, int32_t batch, double mean_ctx);
/* device bytes of the code predictor's layer-0 q/k/v table: for predictor passes 1..14 the engine builds, once at creation, the layer-0
 * attention norm + q/k/v projection of every projected codec row (f32, 14 x rows x (n_head + 2 n_kv) * 128 floats; about 470 MB at full size)
 * and the frame reads rows of it instead of recomputing them.  Same tokens either way.  0 = off: Q3_PRED_L0_TABLE=0 at creation, or Q3_SPEC=ggml */
int64_t q3tts_pred_table_bytes(q3tts_engine* e);

/* ---- continuous-batching scheduler (SURVEY 8b "q3tts_submit / q3tts_poll"; BASELINE config 3) ----
 * Requests queue up and are admitted into the engine's max_batch sequence slots as slots free up; every slot advances
 * one frame per graph replay; finished sequences retire on EOS (engine.rs:558-561) or max_steps.  Results are identical
 * to running each request alone (the arithmetic is batch-invariant).  Either call q3tts_sched_start once (background
 * driver thread) or drive it yourself with q3tts_sched_step / q3tts_wait.  q3tts_generate_batch is submit-all + wait-all. */
#define Q3TTS_REQ_QUEUED 0
#define Q3TTS_REQ_RUNNING 1
#define Q3TTS_REQ_DRAINING 2 /* all frames generated, codec still decoding the tail */
#define Q3TTS_REQ_DONE 3
#define Q3TTS_REQ_CANCELLED 4 /* [EXT] stopped by q3tts_cancel; terminal like DONE and FAILED, partial results stay fetchable until release */
#define Q3TTS_REQ_FAILED (-1)
typedef struct q3tts_req_status {
    int32_t state; int32_t n_frames; int64_t n_pcm; /* frames emitted / PCM samples decoded so far (streamable) */
    double queue_ms, prefill_ms, first_chunk_ms, total_ms;
} q3tts_req_status;
/* r->prompt/n_prompt/sampler/max_steps/mask_eos are read (the prompt is copied); output fields of r are ignored */
int q3tts_submit(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, int64_t* req_id);
int q3tts_submit_ex(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts /* NULL = defaults */,
                    int64_t* req_id);
/* [EXT] a raw prompt plus trailing text ids, one added to the feedback per frame (q3tts_spec.h); the ids are copied.  The first request
 * with n_trail > 0 uploads the text table to the device (~1.24 GB f32 for the real model) */
int q3tts_submit_trailing(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts /* NULL = defaults */,
                          const int32_t* trail_ids, int32_t n_trail, int64_t* req_id);
/* [EXT] live text append (q3tts_spec.h): like q3tts_submit_trailing, but the trail stays open: n_trail may be 0; frames past the appended
 * ids wait (they change nothing the request owns) until q3tts_trail_append brings more.  Appends may come from any thread while the
 * request is queued, being prefilled or running */
int q3tts_submit_trailing_open(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                               const int32_t* trail_ids, int32_t n_trail, int64_t* req_id);
/* appends raw trailing ids (copied); close = 1 closes the trail (n may be 0).
 * 0: appended; 1: the request no longer takes text (finished by EOS / max_steps, done or failed) -- nothing appended;
 * (the same from the moment q3tts_cancel returned 0);
 * < 0: unknown id, request not open, already closed, n < 0, ids NULL with n > 0, or the total would exceed max_prompt (nothing appended) */
int q3tts_trail_append(q3tts_engine* e, int64_t req_id, const int32_t* ids, int32_t n, int32_t close);
/* appended ids, ids consumed by the feedback so far (min(n_frames, appended)), closed flag (1 for a request not submitted open) */
int q3tts_trail_progress(q3tts_engine* e, int64_t req_id, int32_t* n_appended, int32_t* n_consumed, int32_t* closed);
int q3tts_poll(q3tts_engine* e, int64_t req_id, q3tts_req_status* out);
/* streaming read: frames [frame_off, frame_off+max_frames) and PCM [pcm_off, pcm_off+pcm_cap) available right now */
int q3tts_fetch(q3tts_engine* e, int64_t req_id, int32_t* codes_out, int32_t frame_off, int32_t max_frames, float* pcm_out,
                int64_t pcm_off, int64_t pcm_cap, int32_t* got_frames, int64_t* got_pcm);
int q3tts_wait(q3tts_engine* e, int64_t req_id, double timeout_ms /* <0: forever */); /* 0 done, 1 timeout, <0 error */
int q3tts_release(q3tts_engine* e, int64_t req_id);
/* [EXT] stops a request wherever it is.  Thread-safe, issues no HIP call (the scheduler does the device work between two frame groups).
 * 0: cancellation requested (the request reaches Q3TTS_REQ_CANCELLED within the scheduler's next steps; a second call while that is
 *    pending returns 0 again);  1: the request had already ended (done, failed or cancelled) -- nothing changes;  < 0: unknown id.
 * A queued request is CANCELLED at once.  A running one keeps the frames harvested before the scheduler honoured the cancel (bit-identical
 * to the same prefix of the uncancelled run) and the PCM of the whole 4-frame chunks whose decode had been enqueued by then; the tail is
 * not flushed and chunks the decoder thread had not taken are dropped.  The state turns CANCELLED only when nothing of the request is in
 * flight any more: its codec work has completed, its PCM has left the staging region, its codec stream, slot and KV pages are free.
 * q3tts_wait returns 0 on it, q3tts_release accepts it.  Other requests in the batch are untouched.  q3tts_generate_batch* cannot be cancelled */
int q3tts_cancel(q3tts_engine* e, int64_t req_id);
/* [EXT] resume (q3tts_spec.h): r, opts, trail as q3tts_submit_trailing / _open (open != 0: the trail stays open);
 * prefix_codes [n_prefix][16] copied.  n_prefix = 0 is the plain submission.
 * The request continues from frames it is handed instead of generating them: frames 0 .. n_prefix-1 are prefix_codes, frame n_prefix on is
 * generated, and every frame equals the frame the uninterrupted request emits (codes bit-identical, PCM within 1e-4 RMS with the same
 * sample count).  The prefix comes from q3tts_fetch of a cancelled, failed or still running request, on this engine or another one with
 * the same model.  n_frames starts at n_prefix and the prefix is fetchable at once; its PCM is decoded again once the request is admitted.
 * The prompt, sampler, options and trailing ids must be those of the original request.  Exact continuation of a sampled request needs the
 * ORIGINAL seed: has_seed = 0 draws a fresh one as always (the new frames are then a fresh draw behind the kept prefix; so with another seed).
 * Refused (< 0, q3tts_last_error says why, nothing is queued): n_prefix < 0; n_prefix >= max_steps; prefix_codes NULL with n_prefix > 0;
 * a prefix code_0 outside [0, Q3_SAMPLE_END) or equal to Q3_CODEC_EOS; a residual code outside [0, 2048); an open trail with
 * n_trail < n_prefix (those frames ran, so their ids were known); n_prompt + n_prefix beyond the slot's KV capacity; n_prefix > 0 under
 * Q3_SPEC=ggml (as trailing ids there) */
int q3tts_submit_resume(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                        const int32_t* trail_ids, int32_t n_trail, int32_t open,
                        const int32_t* prefix_codes, int32_t n_prefix, int64_t* req_id);
/* [EXT] token log-probabilities (q3tts_spec.h): per frame 17 floats -- log softmax of the RAW head logits (before the repetition penalty,
 * temperature / top-k / top-p and the mask_eos knob) at code_0 (column 0), at the 15 predictor codes (columns 1..15) and at Q3_CODEC_EOS in
 * code_0's talker row (column 16: how close the model was to stopping).  Values are <= 0, within 1e-5 * max(1, |lp|) of the float64
 * log-softmax of the same f32 logits; Q3TTS_LOGPROB_NONE marks a value nothing computed (the prefix rows of a resumed request).
 * Recording is opt-in and changes neither codes nor PCM; with it off the frame graphs are exactly those of an engine that never heard of it.
 * The first enable allocates [max_batch][max_steps + 1][17] + [15][max_batch][2048] floats on the device. */
#define Q3TTS_LOGPROB_COLS 17
#define Q3TTS_LOGPROB_NONE 1.0f
/* requests submitted from now on (any q3tts_submit* form) record log-probabilities; thread-safe; the flag is read once per request at submit.
 * q3tts_generate_batch* never records.  < 0: Q3_SPEC=ggml (as the other [EXT] features there) */
int q3tts_engine_set_logprobs(q3tts_engine* e, int32_t on);
/* rows [frame_off, frame_off+max_frames) available now, [got][17]; got_frames is what q3tts_fetch reports for the same arguments: the two grow
 * together.  A cancelled request keeps the rows of the frames it keeps.  < 0: unknown id, or the request was not recording */
int q3tts_fetch_logprobs(q3tts_engine* e, int64_t req_id, float* out, int32_t frame_off, int32_t max_frames, int32_t* got_frames);
/* [EXT] output formats (q3tts_spec.h "output formats"): the PCM of a request resampled to one of eight rates and / or quantised to int16 on
 * the device, behind the codec, before it crosses to the host.  Opt-in per request; the native path -- its launches, its bytes -- is
 * untouched, and the codes of a request do not depend on its format.
 * q3tts_engine_set_output_format: requests submitted from now on, through any q3tts_submit* form with want_pcm (text, trailing, resume,
 * candidates, decode), deliver *f.  The format is read once per request at submit and once per candidate set, as q3tts_engine_set_logprobs
 * is.  NULL = native, {24000, f32}.  Thread-safe; works under Q3_SPEC=ggml.  < 0: an unknown rate or encoding, f32 above 24000 Hz, or an
 * engine without a codec.  q3tts_generate_batch* always delivers native.
 * The converted stream is the native one DELAYED by Z F / L native samples (48 at 8000 Hz = 2 ms, 24 at 16000, 16 at 32000 / 44100 / 48000)
 * and nothing is flushed: the last Z F / L native samples of an utterance do not come out.  n frames give exactly n * 1920 * L / M samples.
 * q3tts_poll's n_pcm and every offset, capacity and count of the fetch calls are in samples of the request's format.
 * q3tts_request_format: the format a request delivers ({24000, f32} when none was set).
 * q3tts_fetch serves an f32 request at any rate; with pcm_out != NULL on an s16 request it returns < 0 (pcm_out == NULL works as ever).
 * q3tts_fetch_pcm16 is its PCM half for s16 requests and returns < 0 on an f32 request.
 * q3tts_engine_pcm_out_stats: stream chunks the converter has taken and output samples it has made (0, 0 while no request converted). */
int q3tts_engine_set_output_format(q3tts_engine* e, const q3tts_pcm_format* f);
int q3tts_request_format(q3tts_engine* e, int64_t req_id, q3tts_pcm_format* out);
int q3tts_fetch_pcm16(q3tts_engine* e, int64_t req_id, int16_t* out, int64_t off, int64_t cap, int64_t* got);
int q3tts_engine_pcm_out_stats(q3tts_engine* e, int64_t* chunks_converted, int64_t* samples_out);
/* [EXT] speaking rate (q3tts_spec.h "speaking rate"): a pitch-preserving time-scale change (WSOLA) of a request's PCM on the device, behind
 * the codec, before it crosses to the host.  Opt-in per request; an ordinary request keeps its launches and its bytes, and the codes and
 * log-probability rows of a request do not depend on its rate.
 * q3tts_engine_set_speech_rate: requests submitted from now on, through any q3tts_submit* form with want_pcm (text, trailing, open, resume,
 * candidates, decode), are spoken at rate_pct percent of the native tempo, an integer in [50, 200]; 100 = off.  Read once per request at submit
 * and once per candidate set.  Thread-safe; works under Q3_SPEC=ggml.  < 0: out of range, or an engine without a codec.
 * A request with a rate other than 100 delivers 24000 Hz, f32 or s16 (q3tts_engine_set_output_format), and
 * q3tts_tsm_samples(rate, max_steps * 1920, 1) samples of its encoding must fit the engine's staging for one request, max_steps(engine) * 1920
 * * 4 bytes: slowing down makes more samples than native.  Otherwise the submit fails and nothing is queued.
 * While it runs, N native samples have delivered q3tts_tsm_samples(rate, N, 0) samples; at its end the stretcher is flushed and a request of n
 * frames delivers q3tts_tsm_samples(rate, n * 1920, 1).  A cancelled request keeps the whole hops it has and is not flushed.
 * q3tts_poll's n_pcm and every offset, capacity and count of the fetch calls are in delivered samples.
 * Not stretched: want_pcm = 0, q3tts_generate_batch*, scoring, preamble builds.  A primed request's stretcher starts from a reset.
 * q3tts_request_speech_rate: the rate a request was submitted with (100 when none was set).
 * q3tts_engine_tsm_stats: stream chunks the stretcher has taken, synthesis frames (480 samples each) it has made, and flushes (all 0 while no
 * request had a rate). */
int q3tts_engine_set_speech_rate(q3tts_engine* e, int32_t rate_pct);
int q3tts_request_speech_rate(q3tts_engine* e, int64_t req_id, int32_t* rate_pct);
int q3tts_engine_tsm_stats(q3tts_engine* e, int64_t* chunks, int64_t* frames_out, int64_t* flushes);
/* [EXT] pitch (q3tts_spec.h "pitch"): a request's pitch is shifted on the device, behind the codec, with or without a speaking rate: the
 * stretcher at the tempo rate / pitch and an L / M = 100 / pitch resampler behind it, in one launch.  The duration is that of the rate alone.
 * Opt-in per request; a request with pitch 100 keeps its launches and its bytes (a rate-only one those of "speaking rate"), and codes and
 * log-probability rows never depend on the pitch.
 * q3tts_engine_set_pitch: requests submitted from now on, through any q3tts_submit* form with want_pcm (text, trailing, open, resume,
 * candidates, decode), have their fundamental multiplied by pitch_pct / 100, an integer in [50, 200]; 100 = off.  Read once per request at
 * submit and once per candidate set, together with the speaking rate.  Thread-safe; works under Q3_SPEC=ggml.  < 0: out of range, or an engine
 * without a codec.
 * The pair is judged at submit: rate / pitch must lie in [1/2, 2].  A request with a pitch delivers 24000 Hz, f32 or s16, and
 * q3tts_pitch_samples(rate, pitch, max_steps * 1920, 1) samples of its encoding must fit the engine's staging for one request.  Otherwise the
 * submit fails and nothing is queued.
 * While it runs, N native samples have delivered q3tts_pitch_samples(rate, pitch, N, 0) samples; at its end both stages are flushed and a
 * request of n frames delivers q3tts_pitch_samples(rate, pitch, n * 1920, 1).  A cancelled request keeps what it has and is not flushed.
 * q3tts_poll's n_pcm and every offset, capacity and count of the fetch calls are in delivered samples.
 * Not shifted: want_pcm = 0, q3tts_generate_batch*, scoring, preamble builds.  A primed request starts both stages from a reset.
 * q3tts_request_pitch: the pitch a request was submitted with (100 when none was set).
 * q3tts_engine_pitch_stats: stream chunks the shifter has taken, samples it has delivered, flushes, and the bytes of tap tables on the device
 * (all 0 while no request had a pitch; the tables of all 151 pitches are built and uploaded once, by the first such request). */
int q3tts_engine_set_pitch(q3tts_engine* e, int32_t pitch_pct);
int q3tts_request_pitch(q3tts_engine* e, int64_t req_id, int32_t* pitch_pct);
int q3tts_engine_pitch_stats(q3tts_engine* e, int64_t* chunks, int64_t* samples_out, int64_t* flushes, int64_t* table_bytes);
/* [EXT] volume (q3tts_spec.h "volume"): a request's loudness is changed on the device, behind the output conv and in front of every other
 * output stage: a gain in dB with a look-ahead peak limiter, so that a boost never clips and an s16 request is quantised after the gain, not
 * before it.  Opt-in per request; a request with volume 0 keeps its launches and its bytes, and codes and log-probability rows never depend
 * on the volume.
 * q3tts_engine_set_volume: requests submitted from now on, through any q3tts_submit* form with want_pcm (text, trailing, open, resume,
 * candidates, decode), get a gain of db10 tenths of a dB, an integer in [-400, 200]; 0 = off.  Read once per request at submit and once per
 * candidate set, together with the speaking rate and the pitch.  Thread-safe; works under Q3_SPEC=ggml.  < 0: out of range, or an engine
 * without a codec.
 * It composes with every output format, rate and pitch, whose counts, offsets and staging rules are unchanged: n native samples in give n
 * out.  The stream is delayed by Q3_VOL_DELAY = 127 native samples (5.3 ms), which are not flushed: the first 127 native samples of a
 * request with a volume are zeros and its last 127 do not come out.  A cancelled request keeps what it has.
 * Not volumed: want_pcm = 0, q3tts_generate_batch*, scoring, preamble builds.  A primed request starts the stage from a reset; one with a
 * converted format keeps the converter's restored history, the preamble's last native samples as they were decoded, without the gain.
 * q3tts_request_volume: the volume a request was submitted with (0 when none was set).
 * q3tts_engine_volume_stats: stream chunks the stage has taken and native samples it has rewritten (both 0 while no request had a volume;
 * the state store is allocated by the first such request). */
int q3tts_engine_set_volume(q3tts_engine* e, int32_t db10);
int q3tts_request_volume(q3tts_engine* e, int64_t req_id, int32_t* db10);
int q3tts_engine_volume_stats(q3tts_engine* e, int64_t* chunks, int64_t* samples);
/* [EXT] loudness (q3tts_spec.h "loudness"): a request's loudness is measured on the device, as ITU-R BS.1770-4 defines it: K-weighting and
 * the energy and sample peak of every 100 ms block of the native 24000 Hz stream, read behind the output conv and in front of the volume
 * and every other output stage, so the meter sees what the model made whatever the request is delivered as (s16, 8000 Hz, a rate, a pitch,
 * a volume).  The gate runs on the host.  Opt-in per request; an unmetered request keeps its launches, and codes, log-probability rows and
 * PCM never depend on the meter.
 * q3tts_engine_set_loudness: requests submitted from now on, through any q3tts_submit* form with want_pcm (text, trailing, open, resume,
 * candidates, decode), are metered (on != 0) or not.  Read once per request at submit and once per candidate set, together with the other
 * output settings.  Thread-safe; works under Q3_SPEC=ggml.  < 0: an engine without a codec.
 * Not metered: want_pcm = 0, q3tts_generate_batch*, scoring, preamble builds.  A primed request starts the meter from a reset.
 * q3tts_fetch_loudness: rows [block_off, block_off + max_blocks) that are available now into out [got][2] = {energy, peak}: the sum of the
 * squared K-weighted samples of the block and the largest |x| in it.  The rows grow with q3tts_poll's n_pcm; n frames give floor(0.8 n) at
 * the end, the unfinished last block does not come out, and a cancelled request keeps the rows of the chunks it keeps.  < 0: an unknown
 * id, or a request that is not metered.
 * q3tts_request_loudness: q3tts_loudness_gate over the rows so far.
 * q3tts_request_metered: whether a request was submitted metered.
 * q3tts_engine_loudness_stats: stream chunks the meter has taken and blocks it has completed (both 0, and nothing allocated, while no
 * request was metered).
 * To bring a request to a target loudness: meter it, take q3tts_loudness_gain_db10(integrated_lufs, target), set that volume and
 * q3tts_submit_decode the request's frames. */
typedef struct { double integrated_lufs, momentary_max_lufs, peak_dbfs; int32_t n_blocks, n_gated; } q3tts_loudness;
int q3tts_engine_set_loudness(q3tts_engine* e, int32_t on);
int q3tts_fetch_loudness(q3tts_engine* e, int64_t req_id, double* out /* [got][2] */, int64_t block_off, int64_t max_blocks, int64_t* got);
int q3tts_request_loudness(q3tts_engine* e, int64_t req_id, q3tts_loudness* out);
int q3tts_request_metered(q3tts_engine* e, int64_t req_id, int32_t* on);
int q3tts_engine_loudness_stats(q3tts_engine* e, int64_t* chunks, int64_t* blocks);
/* [EXT] codec preambles (q3tts_spec.h "codec preambles"): a request's codec stream starts from the state behind given frames -- a clone
 * voice's reference codes -- instead of zeros, so its first sample is already "in the voice".  The state is built once per preamble and
 * kept on the device; a primed request restores it with one device-to-device launch where the zeroing launch ran.  Opt-in; codes,
 * log-probability rows and every unprimed request are unchanged, only the PCM of a primed request differs: it is decode(preamble ++ frames)
 * without the preamble's samples, at the sample count of the unprimed request.
 * q3tts_preamble_create: codes [n][16] as q3tts_submit_decode takes them; built like a decode-only request (it waits for a codec stream and
 * passes through the decoder thread).  Thread-safe, no HIP call in the caller's thread.  < 0 and nothing queued: q3tts_submit_decode's
 * refusals, Q3TTS_MAX_PREAMBLES live preambles, or n + max_steps above Q3TTS_CODEC_MAX_FRAMES.
 * q3tts_preamble_poll / _wait: state and frame count; _wait returns 0 once the preamble is READY or FAILED, 1 on timeout, and drives the
 * scheduler itself when no driver thread runs, as q3tts_wait does.
 * q3tts_preamble_release: the creator's reference goes.  Voices, the engine-level setting and submitted requests hold their own; the
 * snapshot's slot is recycled when the last one is gone and every restore enqueued from it has completed.  The id is never reused.
 * q3tts_voice_set_preamble: requests submitted through any q3tts_submit_text* form with that voice and want_pcm are primed (-1: none); the
 * engine-level setting does not apply to text forms.  q3tts_engine_set_preamble: read once per request at submit and once per candidate
 * set by the raw-prompt forms (q3tts_submit, _ex, _trailing, _trailing_open, _resume, _candidates, _decode) with want_pcm (-1: none).
 * Both refuse a preamble that is not READY.  want_pcm = 0 and q3tts_generate_batch* are never primed.
 * q3tts_request_preamble: the preamble a request was primed with, -1 when none.
 * q3tts_engine_preamble_stats: preambles built, restores enqueued, device bytes of one snapshot (NULL pointers are skipped). */
/* Q3TTS_MAX_PREAMBLES and the Q3TTS_PREAMBLE_* states: q3tts_spec.h */
int q3tts_preamble_create(q3tts_engine* e, const int32_t* codes, int32_t n, int32_t* preamble_id);
int q3tts_preamble_poll(q3tts_engine* e, int32_t preamble_id, int32_t* state, int32_t* n_frames);
int q3tts_preamble_wait(q3tts_engine* e, int32_t preamble_id, double timeout_ms);
int q3tts_preamble_release(q3tts_engine* e, int32_t preamble_id);
int q3tts_voice_set_preamble(q3tts_engine* e, int32_t voice_id, int32_t preamble_id);
int q3tts_engine_set_preamble(q3tts_engine* e, int32_t preamble_id);
int q3tts_request_preamble(q3tts_engine* e, int64_t req_id, int32_t* preamble_id);
int q3tts_engine_preamble_stats(q3tts_engine* e, int64_t* built, int64_t* restores, int64_t* bytes_per_snapshot);
/* [EXT] prompt stems (q3tts_spec.h "prompt stems"): the head a voice's prompts share -- role, control and speaker rows, the reference text and
 * codes of a clone voice -- is prefilled once and its talker K/V kept on the device; a request whose prompt starts with exactly those rows
 * copies the K/V into its pages with one launch per admission wave and prefills only its own rows.  Opt-in; the codes, log-probability rows
 * and PCM of a request that takes a stem are bit-identical to the same request without one, and a request that does not match runs the
 * plain path (counted as a mismatch, never an error).
 * q3tts_stem_create: rows [n_rows][2048] f32, copied.  Thread-safe, no HIP call in the caller's thread: the build is an internal member of
 * the next admission wave (a slot for one wave, no head, no frame).  < 0 and nothing queued: NULL rows, n_rows outside [1, max_prompt),
 * Q3TTS_MAX_STEMS live stems, a Q3_SPEC=ggml engine.
 * q3tts_voice_stem_create: the rows the q3tts_submit_text* forms build in front of the task text for that voice, lang_id and instruction
 * (NULL / 0: none), through the text BOS row; taken from the prompt builder's own output.
 * q3tts_stem_poll / _wait: state (Q3TTS_STEM_*) and row count; _wait returns 0 once the stem is READY or FAILED, 1 on timeout, and drives the
 * scheduler itself when no driver thread runs, as q3tts_wait does.
 * q3tts_stem_release: the creator's reference goes.  Voices, the engine-level setting and the requests that took the stem hold their own; the
 * device store is freed (by the scheduler thread) when the last one is gone.  The id is never reused.
 * q3tts_voice_set_stem: applies the stem to requests of any q3tts_submit_text* form with that voice (-1: none); a changed lang_id or
 * instruction makes other rows, so such a request runs plain.  q3tts_engine_set_stem: applies it to the raw-prompt forms (q3tts_submit, _ex,
 * _trailing, _trailing_open, _resume, _candidates), read once per request at submit and once per candidate set (-1: none).  Both refuse a
 * stem that is not READY.  q3tts_submit_score, q3tts_submit_decode and q3tts_generate_batch* never take a stem.
 * q3tts_request_stem: the stem a request took and the prompt rows it did not prefill; -1 / 0 when none.
 * q3tts_engine_stem_stats: stems built, restores (requests restored), prompt rows not prefilled, pages copied (per destination), requests a
 * stem applied to that ran plain, device bytes the stores hold now. */
/* Q3TTS_MAX_STEMS and the Q3TTS_STEM_* states: q3tts_spec.h */
typedef struct q3tts_stem_stats { int64_t built, restores, rows_not_prefilled, pages_copied, mismatches, device_bytes; } q3tts_stem_stats;
int q3tts_stem_create(q3tts_engine* e, const float* rows, int32_t n_rows, int32_t* stem_id);
int q3tts_voice_stem_create(q3tts_engine* e, int32_t voice_id, int32_t lang_id, const int32_t* instr_ids, int32_t n_instr, int32_t* stem_id);
int q3tts_stem_poll(q3tts_engine* e, int32_t stem_id, int32_t* state, int32_t* n_rows);
int q3tts_stem_wait(q3tts_engine* e, int32_t stem_id, double timeout_ms);
int q3tts_stem_release(q3tts_engine* e, int32_t stem_id);
int q3tts_voice_set_stem(q3tts_engine* e, int32_t voice_id, int32_t stem_id);
int q3tts_engine_set_stem(q3tts_engine* e, int32_t stem_id);
int q3tts_request_stem(q3tts_engine* e, int64_t req_id, int32_t* stem_id, int32_t* rows_reused);
int q3tts_engine_stem_stats(q3tts_engine* e, q3tts_stem_stats* out);
/* [EXT] score (q3tts_spec.h "scoring"): the teacher-forced log-probabilities of frames the caller already holds -- codes [n][16] behind
 * prompt [n_prompt][2048] and optional CLOSED trailing ids [n_trail] (NULL / 0: none).  Queued like any request; ends Q3TTS_REQ_DONE with
 * n_frames = n and no PCM.  prompt, ids and codes are copied.  Row f of q3tts_fetch_logprobs is the row a recording request that emitted
 * exactly these codes shows for frame f (raw logits: no penalty, temperature, top-k / top-p or EOS mask; within 1e-5 * max(1, |lp|) of the
 * float64 log-softmax of the same f32 logits); q3tts_fetch returns the given codes.  Both report 0 frames until the request is DONE and n
 * afterwards.  q3tts_poll / q3tts_wait / q3tts_release as for any request; q3tts_cancel gives CANCELLED with 0 frames; q3tts_trail_append
 * returns < 0 (the trail is not open).  Scoring neither needs q3tts_engine_set_logprobs nor changes it, and no running request is disturbed.
 * The request is prefilled in the ordinary admission waves, holds one slot and its KV pages until its rows are computed and never joins the
 * frame graph.  The first call allocates the scoring state (a second predictor context of 16 * score_width tokens and
 * [max_batch][max_steps][17] floats of rows).
 * Refused (< 0, q3tts_last_error says why, nothing is queued): n <= 0; n > the engine's max_steps; codes or prompt NULL; n_prompt < 1 or
 * > max_prompt; a code_0 outside [0, Q3_SAMPLE_END) or equal to Q3_CODEC_EOS; a residual code outside [0, 2048); n_trail < 0 or
 * > max_prompt, or trail_ids NULL with n_trail > 0; n_prompt + n beyond the slot's KV capacity; Q3_SPEC=ggml */
int q3tts_submit_score(q3tts_engine* e, const float* prompt, int32_t n_prompt, const int32_t* trail_ids, int32_t n_trail,
                       const int32_t* codes, int32_t n, int64_t* req_id);
int32_t q3tts_engine_score_width(q3tts_engine* e);   /* frames per predictor scoring pass */
/* [EXT] candidate sets (q3tts_spec.h "candidate sets"): n sampled takes of ONE prompt behind ONE prefill, for best-of-n ranking with
 * q3tts_fetch_logprobs / q3tts_submit_score and q3tts_cancel.  Candidate i is exactly what q3tts_submit_trailing(e, r, want_pcm, opts,
 * trail_ids, n_trail) queues with r->sampler.has_seed = 1 and seed = seeds[i] -- its codes, PCM and log-probability rows are those of that
 * request run alone, bit for bit -- with its own talker and predictor streams (seed ^ Q3_PRED_SEED_XOR); r->sampler.seed / has_seed are
 * ignored.  Options and the closed trail are shared, the recording flag is read once for the set, and prompt and ids are copied once.
 * The n requests are queued together and admitted whole into one wave: the set waits at the head of the queue until n slots (and, with
 * want_pcm, n codec streams) are free, and nothing behind it overtakes.  The first member not cancelled in the queue is prefilled; its
 * ceil(n_prompt / 64) KV pages are copied whole into the other members' pages by one kernel launch, and every member draws its first
 * code_0 from the last prompt row's logits.  From then on the members are ordinary requests: req_ids[0 .. n-1] take q3tts_poll / _fetch /
 * _wait / _cancel / _release / _fetch_logprobs one by one, and a cancelled member -- the prefilled one included -- leaves the others as
 * they are.  n = 1 is q3tts_submit_trailing.  Greedy sampling is allowed: every candidate is then the plain greedy run.
 * No resumed prefix and no open trail: a set is made of fresh requests with a closed trail (use q3tts_submit_resume / _trailing_open singly).
 * Refused (< 0, q3tts_last_error says why, nothing is queued, req_ids untouched): n < 1; n > max_batch; seeds or req_ids NULL; n_trail < 0 or
 * > max_prompt, or trail_ids NULL with n_trail > 0; a prompt, max_steps or options q3tts_submit_ex refuses; Q3_SPEC=ggml */
int q3tts_submit_candidates(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                            const int32_t* trail_ids, int32_t n_trail, const uint64_t* seeds, int32_t n, int64_t* req_ids);
/* sets of n >= 2 accepted; prompt rows whose prefill a copy replaced ((members prefilled together - 1) * n_prompt per set); KV pages copied,
 * counted per destination.  Any pointer may be NULL */
int q3tts_engine_candidate_stats(q3tts_engine* e, int64_t* sets, int64_t* prefill_rows_saved, int64_t* pages_copied);
/* [EXT] decode given frames (q3tts_spec.h "decoding given frames"): the PCM of frames the caller already holds -- codes [n][16] as q3tts_fetch
 * returns them, copied -- through the engine's own codec: no second copy of the codec weights, and the chunks share decode passes with those
 * of the running requests.  For the winner of a codes-only candidate set, for utterances cached as codes, for a request that ran with
 * want_pcm = 0, for frames another engine generated.  The PCM is that of a request that emitted exactly these frames and ended after frame
 * n - 1: same sample count, within 1e-4 RMS (the stream is reset, the frames are clamped and cut into 4-frame chunks and the n % 4 left are
 * flushed, as for a generating request).  The request takes no talker slot and no KV pages, is never prefilled and never part of the frame
 * graph; it holds one codec stream and its PCM staging region from admission to its fence.  It waits in a queue of its own -- requests
 * waiting for a slot do not hold it up -- and is admitted, after the step's generating wave has taken its streams, while a stream is free
 * and fewer than q3tts_engine_decode_width such requests hold one.  Its chunks reach the decoder thread together with the chunks of that
 * step's frame group (at once on an engine that steps nothing) and take the seats the running requests' chunks leave in a decode
 * pass, and lead every fifth pass when they would otherwise wait.  No other request's codes change; its PCM stays within the same tolerance.
 * Q3TTS_REQ_QUEUED until it holds a stream, then Q3TTS_REQ_DRAINING, Q3TTS_REQ_DONE behind its fence.  q3tts_poll reports n_frames = n from
 * submission on, prefill_ms = 0, and n_pcm growing chunk by chunk; q3tts_fetch returns the given codes at once and the PCM decoded so far;
 * q3tts_wait / q3tts_release as for any request.  q3tts_cancel: a queued request is CANCELLED at once with no PCM; one that holds a stream
 * keeps the PCM of the chunks already enqueued and turns CANCELLED behind its fence, as a draining request does.  q3tts_fetch_logprobs,
 * q3tts_trail_append and q3tts_trail_progress return < 0 (nothing is recorded, there is no trail).  Works under Q3_SPEC=ggml: nothing of the
 * talker runs.  Thread-safe, and free of HIP calls in the caller's thread.
 * Refused (< 0, q3tts_last_error says why, nothing is queued, *req_id untouched): e, codes or req_id NULL; n < 1; n > the engine's max_steps
 * (a stream's staging region holds max_steps frames); an engine created with load_codec = 0; a code_0 outside [0, Q3_SAMPLE_END) or equal
 * to Q3_CODEC_EOS; a residual code outside [0, 2048) */
int q3tts_submit_decode(q3tts_engine* e, const int32_t* codes, int32_t n, int64_t* req_id);
int32_t q3tts_engine_decode_width(q3tts_engine* e);  /* decode-only requests that may hold a codec stream at once: max(1, (streams - max_batch) / 2); 0 without a codec */
/* decode-only requests accepted; their chunks decoded; of those, chunks that shared a pass with at least one chunk of a generating request.
 * Any pointer may be NULL */
int q3tts_engine_decode_stats(q3tts_engine* e, int64_t* requests, int64_t* chunks, int64_t* chunks_shared);
/* rows of one talker prefill launch: a longer admission wave (prompts + resumed prefixes) is prefilled in chunks of this many rows
 * (an asynchronous wave, admitted beside running requests, in chunks of at most 256) */
int32_t q3tts_engine_prefill_width(q3tts_engine* e);
int q3tts_sched_start(q3tts_engine* e);
int q3tts_sched_stop(q3tts_engine* e);
int q3tts_sched_step(q3tts_engine* e, int32_t* busy);
/* voices: the engine-side analogue of VoiceFile (utils/voice_file.rs:5-22).  ref_codes [n_ref_frames*16] / ref_text_ids may be
 * NULL for preset voices.  In multi-GPU serving the owning rank broadcasts these arrays first (q3tts.dist.broadcast_voice). */
int q3tts_voice_register(q3tts_engine* e, const float* spk_emb2048, const int32_t* ref_codes, int32_t n_ref_codes,
                         const int32_t* ref_text_ids, int32_t n_ref_text, int32_t* voice_id);
/* generate_with_voice_ids (engine.rs:390-435): builds the preset or clone prompt from the voice + token ids, then submits */
int q3tts_submit_text(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                      const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                      int32_t mask_eos, int32_t want_pcm, int64_t* req_id);
int q3tts_submit_text_ex(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                         const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                         int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id);
/* [EXT] q3tts_submit_text_ex in the streaming-text layout (q3tts_prompt_build_streaming); n_text >= 1 */
int q3tts_submit_text_streaming(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                                int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id);
/* [EXT] text level: the streaming layout from the text known so far (n_text >= 1, only t_0 enters the prompt; t_1 .. become the open
 * trail).  open(t[:k]) + q3tts_text_append(t[k:], is_last = 1) gives what q3tts_submit_text_streaming(t) gives */
int q3tts_submit_text_streaming_open(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                     const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                                     int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id);
/* appends text ids; is_last = 1 also appends Q3_TEXT_EOS and closes.  Return codes as q3tts_trail_append */
int q3tts_text_append(q3tts_engine* e, int64_t req_id, const int32_t* text_ids, int32_t n, int32_t is_last);

/* ---- multi-GPU: request sharding, weights replicated per device, no collective on the data path ----
 * q3tts_group_*: ONE process, N devices.  One engine (+ scheduler thread + decoder thread) per entry of device_ids; requests go round-robin
 * (request i -> engine i % n); group request ids carry the engine index.  q3tts_group_voice_register uploads the VoiceFile payload
 * (utils/voice_file.rs:5-22) to the first device and broadcasts it device-to-device -- ncclBroadcast over communicators from
 * ncclCommInitAll (RCCL over xGMI; librccl.so is bound at run time) or, when RCCL is unavailable or a device is listed twice,
 * hipMemcpyPeerAsync -- and every engine registers the voice from its own device's copy.  Register voices through the group only, so
 * that one voice id is valid on every engine.  p->device is ignored. */
typedef struct q3tts_group q3tts_group;
int q3tts_group_create(const q3tts_engine_params* p, const int32_t* device_ids, int32_t n_dev, q3tts_group** out);
void q3tts_group_destroy(q3tts_group* g);
int32_t q3tts_group_size(q3tts_group* g);
q3tts_engine* q3tts_group_engine(q3tts_group* g, int32_t i);   /* borrowed: stats, assets, per-engine calls */
int32_t q3tts_group_uses_rccl(q3tts_group* g);                 /* 1: registrations go through ncclBroadcast, 0: peer copies */
/* What the group's one exchange step actually runs on, so a multi-GPU harness can ASSERT "RCCL, N ranks" instead of assuming it: rccl_ranks = size of
 * the ncclCommInitAll communicator set (0 = peer copies: one device, a device listed twice, or librccl absent), and how many registrations took
 * which path so far.  The first registration also prints one line to stderr naming the path. */
typedef struct q3tts_group_info_t {
    int32_t n_devices, rccl_loaded, rccl_ranks, distinct_devices;
    int64_t registrations_rccl, registrations_peer_copy;
} q3tts_group_info_t;
int q3tts_group_info(q3tts_group* g, q3tts_group_info_t* out);
int q3tts_group_voice_register(q3tts_group* g, const float* spk_emb2048, const int32_t* ref_codes, int32_t n_ref_codes,
                               const int32_t* ref_text_ids, int32_t n_ref_text, int32_t* voice_id);
int q3tts_group_submit(q3tts_group* g, const q3tts_request* r, int32_t want_pcm, int64_t* req_id);
int q3tts_group_submit_text(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                            const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                            int32_t mask_eos, int32_t want_pcm, int64_t* req_id);
int q3tts_group_submit_ex(q3tts_group* g, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id);
int q3tts_group_submit_text_ex(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                               const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                               int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id);
int q3tts_group_submit_text_streaming(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                      const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                                      int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id);
/* [EXT] live text append through a group: append / progress are routed by the engine index the group request id carries */
int q3tts_group_submit_text_streaming_open(q3tts_group* g, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                           const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler,
                                           int32_t max_steps, int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts,
                                           int64_t* req_id);
int q3tts_group_text_append(q3tts_group* g, int64_t req_id, const int32_t* text_ids, int32_t n, int32_t is_last);
int q3tts_group_trail_append(q3tts_group* g, int64_t req_id, const int32_t* ids, int32_t n, int32_t close);
int q3tts_group_trail_progress(q3tts_group* g, int64_t req_id, int32_t* n_appended, int32_t* n_consumed, int32_t* closed);
int32_t q3tts_group_device_of(q3tts_group* g, int64_t req_id); /* HIP device a request was sharded to */
int q3tts_group_poll(q3tts_group* g, int64_t req_id, q3tts_req_status* out);
int q3tts_group_fetch(q3tts_group* g, int64_t req_id, int32_t* codes_out, int32_t frame_off, int32_t max_frames, float* pcm_out,
                      int64_t pcm_off, int64_t pcm_cap, int32_t* got_frames, int64_t* got_pcm);
int q3tts_group_wait(q3tts_group* g, int64_t req_id, double timeout_ms);
int q3tts_group_release(q3tts_group* g, int64_t req_id);
int q3tts_group_cancel(q3tts_group* g, int64_t req_id);       /* [EXT] q3tts_cancel, routed by the engine index the id carries */
/* [EXT] q3tts_submit_resume on engine engine_index (-1 = round robin): a request cancelled or failed on one engine goes on on another */
int q3tts_group_submit_resume(q3tts_group* g, int32_t engine_index, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                              const int32_t* trail_ids, int32_t n_trail, int32_t open,
                              const int32_t* prefix_codes, int32_t n_prefix, int64_t* req_id);
/* [EXT] q3tts_submit_score on engine engine_index (-1 = round robin) */
int q3tts_group_submit_score(q3tts_group* g, int32_t engine_index, const float* prompt, int32_t n_prompt, const int32_t* trail_ids,
                             int32_t n_trail, const int32_t* codes, int32_t n, int64_t* req_id);
/* [EXT] q3tts_submit_candidates on engine engine_index (-1 = round robin): the whole set goes to ONE engine, every id carries its index */
/* [EXT] q3tts_submit_decode on engine engine_index (-1 = round robin); the id carries the engine, so q3tts_group_poll / _fetch / _wait / _cancel /
 * _release serve it */
int q3tts_group_submit_decode(q3tts_group* g, int32_t engine_index, const int32_t* codes, int32_t n, int64_t* req_id);
int q3tts_group_submit_candidates(q3tts_group* g, int32_t engine_index, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                                  const int32_t* trail_ids, int32_t n_trail, const uint64_t* seeds, int32_t n, int64_t* req_ids);
int q3tts_group_set_logprobs(q3tts_group* g, int32_t on);      /* [EXT] q3tts_engine_set_logprobs on every engine */
int q3tts_group_fetch_logprobs(q3tts_group* g, int64_t req_id, float* out, int32_t frame_off, int32_t max_frames, int32_t* got_frames);
int q3tts_group_set_output_format(q3tts_group* g, const q3tts_pcm_format* f);   /* [EXT] q3tts_engine_set_output_format on every engine */
int q3tts_group_fetch_pcm16(q3tts_group* g, int64_t req_id, int16_t* out, int64_t off, int64_t cap, int64_t* got);
int q3tts_group_request_format(q3tts_group* g, int64_t req_id, q3tts_pcm_format* out);
int q3tts_group_set_speech_rate(q3tts_group* g, int32_t rate_pct);   /* [EXT] q3tts_engine_set_speech_rate on every engine */
int q3tts_group_request_speech_rate(q3tts_group* g, int64_t req_id, int32_t* rate_pct);
int q3tts_group_set_pitch(q3tts_group* g, int32_t pitch_pct);   /* [EXT] q3tts_engine_set_pitch on every engine */
int q3tts_group_request_pitch(q3tts_group* g, int64_t req_id, int32_t* pitch_pct);
int q3tts_group_set_volume(q3tts_group* g, int32_t db10);   /* [EXT] q3tts_engine_set_volume on every engine */
int q3tts_group_request_volume(q3tts_group* g, int64_t req_id, int32_t* db10);
int q3tts_group_set_loudness(q3tts_group* g, int32_t on);   /* [EXT] q3tts_engine_set_loudness on every engine */
int q3tts_group_fetch_loudness(q3tts_group* g, int64_t req_id, double* out, int64_t block_off, int64_t max_blocks, int64_t* got);
int q3tts_group_request_loudness(q3tts_group* g, int64_t req_id, q3tts_loudness* out);
int q3tts_group_request_metered(q3tts_group* g, int64_t req_id, int32_t* on);
/* [EXT] codec preambles on every engine under one id, as voices are (create preambles through the group only); _wait waits for all of them */
int q3tts_group_preamble_create(q3tts_group* g, const int32_t* codes, int32_t n, int32_t* preamble_id);
int q3tts_group_preamble_wait(q3tts_group* g, int32_t preamble_id, double timeout_ms);
int q3tts_group_preamble_release(q3tts_group* g, int32_t preamble_id);
int q3tts_group_voice_set_preamble(q3tts_group* g, int32_t voice_id, int32_t preamble_id);
int q3tts_group_set_preamble(q3tts_group* g, int32_t preamble_id);
int q3tts_group_request_preamble(q3tts_group* g, int64_t req_id, int32_t* preamble_id);
/* [EXT] prompt stems on every engine under one id, as preambles are (create stems through the group only); _wait waits for all of them, the
 * setters take a stem that is READY on every engine, _stem_stats adds the engines' counters up */
int q3tts_group_stem_create(q3tts_group* g, const float* rows, int32_t n_rows, int32_t* stem_id);
int q3tts_group_voice_stem_create(q3tts_group* g, int32_t voice_id, int32_t lang_id, const int32_t* instr_ids, int32_t n_instr, int32_t* stem_id);
int q3tts_group_stem_wait(q3tts_group* g, int32_t stem_id, double timeout_ms);
int q3tts_group_stem_release(q3tts_group* g, int32_t stem_id);
int q3tts_group_voice_set_stem(q3tts_group* g, int32_t voice_id, int32_t stem_id);
int q3tts_group_set_stem(q3tts_group* g, int32_t stem_id);
int q3tts_group_request_stem(q3tts_group* g, int64_t req_id, int32_t* stem_id, int32_t* rows_reused);
int q3tts_group_stem_stats(q3tts_group* g, q3tts_stem_stats* out);
int q3tts_group_start(q3tts_group* g);                         /* q3tts_sched_start on every engine */
int q3tts_group_stop(q3tts_group* g);
/* q3tts_comm_*: ONE process per GPU (what `bench.py --gpus N` / torchrun-style launchers use).  Rank 0 makes the 128-byte id and ships it to
 * the other ranks by any means (environment, file, socket); every rank creates its communicator (ncclCommInitRank) and calls
 * q3tts_comm_voice_register collectively: the root passes the voice, the other ranks pass NULL / 0 and receive it; each registers it on
 * its own engine. */
typedef struct q3tts_comm q3tts_comm;
int q3tts_comm_available(void);                                /* 1 when librccl.so could be loaded */
int q3tts_comm_unique_id(uint8_t out_id[128]);
int q3tts_comm_create(const uint8_t id[128], int32_t rank, int32_t world, int32_t device, q3tts_comm** out);
void q3tts_comm_destroy(q3tts_comm* c);
int q3tts_comm_voice_register(q3tts_comm* c, q3tts_engine* e, int32_t root, const float* spk_emb2048, const int32_t* ref_codes,
                              int32_t n_ref_codes, const int32_t* ref_text_ids, int32_t n_ref_text, int32_t* voice_id);
int32_t q3tts_engine_device(q3tts_engine* e);

/* ---- assets + prompt builder (host) ---- */
typedef struct q3tts_assets q3tts_assets;
int q3tts_assets_open(const char* gguf_path, q3tts_assets** out);
void q3tts_assets_close(q3tts_assets* a);
const q3tts_assets* q3tts_engine_assets(q3tts_engine* e);
int q3tts_assets_codec_embedding(const q3tts_assets* a, int32_t q, int32_t code, float* out2048);
int q3tts_assets_text_embedding(const q3tts_assets* a, int64_t token, float* out2048);
int q3tts_assets_tts_pad(const q3tts_assets* a, float* out2048);
/* returns rows written (each 2048 f32) or <0; lang_id/spk_id < 0 mean None; pointers may be NULL */
int q3tts_prompt_build_core(const q3tts_assets* a, const int32_t* text_ids, int32_t n_text, int32_t lang_id, int32_t spk_id,
                            const float* spk_emb2048, const int32_t* instr_ids, int32_t n_instr, const float* mid_rows,
                            int32_t n_mid, float* out, int32_t max_rows);
int q3tts_prompt_build_clone(const q3tts_assets* a, const int32_t* text_ids, int32_t n_text, const int32_t* ref_codes,
                             int32_t n_ref_codes, const int32_t* ref_text_ids, int32_t n_ref_text, const float* spk_emb2048,
                             int32_t lang_id, const int32_t* instr_ids, int32_t n_instr, float* out, int32_t max_rows);
/* [EXT] streaming-text layout (q3tts_spec.h): the prompt of build_core (ref_codes NULL / n_ref_codes 0) or of build_clone (ref_codes given:
 * clone voice, spk_emb2048 and lang_id required, spk_id ignored) cut after [text(BOS) + E0(PAD)] and ended by [text(t_0) + E0(BOS)];
 * trail_ids (capacity trail_cap) receives t_1 .. t_{n-1}, TEXT_EOS and *n_trail = n_text.  n_text >= 1.  Returns rows written or < 0 */
int q3tts_prompt_build_streaming(const q3tts_assets* a, const int32_t* text_ids, int32_t n_text, int32_t lang_id, int32_t spk_id,
                                 const float* spk_emb2048, const int32_t* instr_ids, int32_t n_instr, const int32_t* ref_codes,
                                 int32_t n_ref_codes, const int32_t* ref_text_ids, int32_t n_ref_text, float* out, int32_t max_rows,
                                 int32_t* trail_ids, int32_t trail_cap, int32_t* n_trail);

/* ---- sampler (host) ---- */
typedef struct q3tts_sampler q3tts_sampler;
q3tts_sampler* q3tts_sampler_new(float temperature, int32_t top_k, float top_p, uint64_t seed);
void q3tts_sampler_free(q3tts_sampler* s);
int32_t q3tts_sampler_sample(q3tts_sampler* s, const float* logits, int32_t n_vocab, int32_t start, int32_t end);

/* ---- chunker (host) ---- */
typedef void (*q3tts_decode_cb)(void* user, const int64_t* codes, int32_t n_codes, int32_t is_final);
typedef struct q3tts_chunker q3tts_chunker;
q3tts_chunker* q3tts_chunker_new(q3tts_decode_cb cb, void* user);
void q3tts_chunker_free(q3tts_chunker* c);
int q3tts_chunker_push(q3tts_chunker* c, const int64_t* codes, int32_t n, int32_t is_final);

/* ---- streaming codec decoder (device) ---- */
/* A stream carries at most this many frames between resets (12.5 frames/s: about 87 minutes): its RoPE positions 0 .. Q3TTS_CODEC_MAX_FRAMES-1
 * match the oracle's unbounded n_seen + t.  A decode call that would take a stream past it returns an error before anything is uploaded or
 * launched and leaves every stream's state unchanged; _state_import refuses a frame counter above it. */
#define Q3TTS_CODEC_MAX_FRAMES 65536
typedef struct q3tts_decoder q3tts_decoder;
int q3tts_decoder_create(const char* codec_gguf, int32_t n_streams, q3tts_decoder** out);
void q3tts_decoder_destroy(q3tts_decoder* d);
/* batched form: one pass decodes up to max_group streams that each contribute the same number of new frames */
int q3tts_decoder_create_ex(const char* codec_gguf, int32_t n_streams, int32_t max_frames_per_call, int32_t max_group, q3tts_decoder** out);
/* streams [G] distinct; codes [G][n_frames][16] i64; wav_out [G][n_frames*samples_per_frame] f32 */
int q3tts_decoder_decode_group(q3tts_decoder* d, int32_t G, const int32_t* streams, const int64_t* codes, int32_t n_frames, float* wav_out);
int q3tts_decoder_samples_per_frame(q3tts_decoder* d);
int q3tts_decoder_reset(q3tts_decoder* d, int32_t stream);
/* codes [n_frames][16] i64; writes up to n_frames*samples_per_frame floats; *valid_samples = prefix to keep */
int q3tts_decoder_decode(q3tts_decoder* d, int32_t stream, const int64_t* codes, int32_t n_frames, int32_t is_last,
                         float* final_wav, int64_t* valid_samples);

/* DecoderState (onnx.rs:461-496) export / import: one stream's streaming state as a flat f32 blob whose layout is a list of named tensors
 * (pre_conv_history, past_key_i / past_value_i, the conv_history pieces, counters) -- to checkpoint a stream, move it to another decoder
 * or device, or inspect it.  q3tts_decoder_state_entry(i) describes entry i and returns the entry count. */
int64_t q3tts_decoder_state_floats(q3tts_decoder* d);
/* n_floats = the caller's buffer length; it must equal q3tts_decoder_state_floats().  _import also validates the blob's trailer (cached-position
 * count within the attention window, frame counter finite and non-negative) before anything is committed, so a blob from another decoder
 * configuration or a corrupted one is an error, not an out-of-range device access on the next decode. */
int q3tts_decoder_state_export(q3tts_decoder* d, int32_t stream, float* out, int64_t n_floats);
int q3tts_decoder_state_import(q3tts_decoder* d, int32_t stream, const float* in, int64_t n_floats);
int32_t q3tts_decoder_state_entry(q3tts_decoder* d, int32_t i, const char** name, int64_t* offset, int32_t* rows, int32_t* cols);
/* [EXT] codec preambles (q3tts_spec.h "codec preambles"): a device-side copy of one stream's whole state -- the history slots of every state
 * tensor and the two counters -- made and put back by one launch each on the decoder's own HIP stream, in order with its decodes and without
 * any synchronisation.  _create snapshots `stream` as it stands behind the decodes issued so far; _restore writes a snapshot into any stream
 * (the stream's next decode continues the snapshotted one bit for bit, other streams are not touched); _free gives the slot back.  A
 * snapshot outlives resets and decodes of its source stream.  < 0 before anything is launched: a stream or snapshot out of range, a freed
 * snapshot.  q3tts_decoder_snapshot_bytes: device bytes of one snapshot (the blob without its two counters). */
int q3tts_decoder_snapshot_create(q3tts_decoder* d, int32_t stream, int32_t* snapshot);
int q3tts_decoder_snapshot_restore(q3tts_decoder* d, int32_t snapshot, int32_t stream);
int q3tts_decoder_snapshot_free(q3tts_decoder* d, int32_t snapshot);
int64_t q3tts_decoder_snapshot_bytes(q3tts_decoder* d);

/* ---- mel front end (device) ---- */
/* q3tts_mel_frames is the number of frames q3tts_mel writes: 0 below 256 samples (no whole frame fits the padded clip), n / 256 from there on.
 * q3tts_mel_tables (host only, no device needed) fills the f32 periodic Hann window and Slaney filterbank the kernel reads. */
int q3tts_mel_frames(int32_t n_samples);
int q3tts_mel(const float* audio, int32_t n_samples, float* mel_out /* [frames][128] */);
int q3tts_mel_tables(float* hann /* [1024] */, float* fb /* [128][513] */);

/* ---- transformer contexts (shared with the llama shim; also the layer-level parity surface) ---- */
typedef struct q3tts_tf q3tts_tf;
int q3tts_tf_open(const char* gguf_path, int32_t n_ctx, int32_t max_tok, q3tts_tf** out);
void q3tts_tf_close(q3tts_tf* t);
int q3tts_tf_dims(q3tts_tf* t, int32_t* n_embd, int32_t* n_layer, int32_t* n_head, int32_t* n_vocab);
void q3tts_tf_clear(q3tts_tf* t);
/* ntok tokens of one sequence: x [ntok][n_embd]; pos [ntok][4]; appends to the KV cache.
 * hidden_out [ntok][n_embd] (final-norm) and logits_out [ntok][row1-row0] may be NULL. */
int q3tts_tf_eval(q3tts_tf* t, const float* x, const int32_t* pos4, int32_t ntok, float* hidden_out, float* logits_out,
                  int32_t row0, int32_t row1);

/* ---- tokenizer (host code) ----
 * Byte-level BPE over a HuggingFace tokenizer.json: what the reference's Tokenizer::{load, encode, decode} get from the `tokenizers` crate
 * (/root/reference/src/utils/tokenizer.rs:9-38): <model_dir>/tokenizer/tokenizer.json, encode(text, add_special_tokens = false),
 * decode(ids, skip_special_tokens = false).  Qwen2-family files: added tokens, Split(Qwen2 pattern) + ByteLevel, BPE merges. */
typedef struct q3tts_tokenizer q3tts_tokenizer;
int q3tts_tokenizer_open(const char* tokenizer_json, q3tts_tokenizer** out);
void q3tts_tokenizer_close(q3tts_tokenizer* t);
int32_t q3tts_tokenizer_encode(q3tts_tokenizer* t, const char* text_utf8, int32_t* ids, int32_t cap); /* count (may exceed cap), < 0 error */
int64_t q3tts_tokenizer_decode(q3tts_tokenizer* t, const int32_t* ids, int32_t n, char* buf, int64_t cap); /* byte length, < 0 error */
int32_t q3tts_tokenizer_vocab_size(q3tts_tokenizer* t);
int64_t q3tts_text_nfc(const char* utf8, char* out, int64_t cap); /* NFC as the tokenizer's normaliser applies it; returns the size needed (with NUL) */

/* ---- ONNX graph ingestion (host code, no GPU needed) ----
 * A minimal reader of ONNX ModelProto files (protobuf wire format walked by hand): what `ort::Session` parses for the reference's
 * qwen3_tts_decoder.onnx / codec_encoder.onnx / speaker_encoder.onnx (/root/reference/src/models/onnx.rs:97-163, 324-347).  It exposes
 * the node list with attributes, the initialisers (weights, zero-copy into the mapped file), graph inputs / outputs, the op -> HIP
 * kernel table of this engine, and a check of the streaming-decoder I/O contract (onnx.rs:355-455).  tools/q3onnx_dump prints all of it. */
typedef struct q3tts_onnx q3tts_onnx;
int q3tts_onnx_open(const char* path, q3tts_onnx** out);
void q3tts_onnx_close(q3tts_onnx* m);
int q3tts_onnx_counts(q3tts_onnx* m, int32_t* n_nodes, int32_t* n_initializers, int32_t* n_inputs, int32_t* n_outputs);
int64_t q3tts_onnx_summary(q3tts_onnx* m, char* buf, int64_t cap); /* returns the size needed (with NUL) */
int q3tts_onnx_node(q3tts_onnx* m, int32_t i, const char** op_type, const char** name, int32_t* n_in, int32_t* n_out, int32_t* n_attr);
const char* q3tts_onnx_node_input(q3tts_onnx* m, int32_t i, int32_t j);
const char* q3tts_onnx_node_output(q3tts_onnx* m, int32_t i, int32_t j);
int32_t q3tts_onnx_node_attr_ints(q3tts_onnx* m, int32_t i, const char* attr, int64_t* out, int32_t cap); /* count, -1 = absent */
int32_t q3tts_onnx_node_attr_float(q3tts_onnx* m, int32_t i, const char* attr, float* out);
int q3tts_onnx_initializer(q3tts_onnx* m, int32_t i, const char** name, int32_t* dtype, int64_t* dims8, int32_t* ndims, const void** data,
                           int64_t* nbytes);
const char* q3tts_onnx_op_kernel(const char* op_type);            /* HIP kernel serving the op, NULL = none yet */
int q3tts_onnx_decoder_contract(q3tts_onnx* m, char* buf, int64_t cap); /* 0 satisfied, 1 missing (names in buf) */

/* ---- ONNX graph execution on the GPU (second half; row a17) ----
 * What `ort::Session::run` is to the reference's encoders (/root/reference/src/models/onnx.rs:97-121 `AudioEncoder::encode`:
 * "input_values" [1, T] f32 -> "audio_codes" [1, F, 16] i64; :140-163 `SpeakerEncoder::encode`: "mels" [1, n, 128] f32 -> "spk_emb" [1, 2048]):
 * a general interpreter of the operator set such exports use, one HIP launch per node, float tensors resident in HBM, shape arithmetic on the
 * host.  dtype codes are ONNX's (1 = f32, 7 = i64, 9 = bool, fetched as f32 0 / 1).  q3tts_onnx_session_unsupported lists op types of the
 * graph without a kernel (0 = the graph is executable). */
typedef struct q3tts_onnx_session q3tts_onnx_session;
int q3tts_onnx_session_open(const char* path, int32_t device, q3tts_onnx_session** out);
void q3tts_onnx_session_close(q3tts_onnx_session* s);
int32_t q3tts_onnx_session_unsupported(q3tts_onnx_session* s, char* buf, int64_t cap); /* count; names comma-separated in buf */
int q3tts_onnx_session_set_input(q3tts_onnx_session* s, const char* name, int32_t dtype, const void* data, const int64_t* shape, int32_t rank);
int q3tts_onnx_session_run(q3tts_onnx_session* s);
int q3tts_onnx_session_output_info(q3tts_onnx_session* s, const char* name, int32_t* dtype, int32_t* rank, int64_t* shape8);
int q3tts_onnx_session_output(q3tts_onnx_session* s, const char* name, void* dst, int64_t cap_bytes); /* f32 or i64 elements */
int64_t q3tts_onnx_session_launches(q3tts_onnx_session* s);                              /* kernel launches of all runs so far */
int q3tts_onnx_op_executable(const char* op_type);                                       /* 1 when the executor runs the op */
/* AudioDecoder over the executor (/root/reference/src/models/onnx.rs:322-458): the exported streaming decoder graph with its state
 * (pre_conv_history, latent_buffer, conv_history, past_key_i / past_value_i) carried on the device between chunks.  _decode returns the first
 * `valid_samples` samples of `final_wav`; *n_out receives their count.  The chunk's PCM stays in the handle until the next _decode / _reset:
 * when pcm is NULL or cap is too small the call returns 2 (state advanced, nothing lost) and q3tts_onnx_decoder_fetch copies the same chunk
 * out again into a buffer of at least *n_out samples. */
typedef struct q3tts_onnx_decoder q3tts_onnx_decoder;
int q3tts_onnx_decoder_open(const char* path, int32_t device, q3tts_onnx_decoder** out);
void q3tts_onnx_decoder_close(q3tts_onnx_decoder* d);
int q3tts_onnx_decoder_reset(q3tts_onnx_decoder* d);
int q3tts_onnx_decoder_decode(q3tts_onnx_decoder* d, const int64_t* codes, int32_t n_frames, int32_t is_final, float* pcm, int64_t cap, int64_t* n_out);
int q3tts_onnx_decoder_fetch(q3tts_onnx_decoder* d, float* pcm, int64_t cap, int64_t* n_out);

/* ---- kernel-level entry points used by the parity tests (host buffers in/out) ---- */
int q3tts_op_gemv_q8(const void* w_q8_0 /* GGUF Q8_0 rows [n][k/32][34 B] */, int32_t n, int32_t k, const int8_t* xq,
                     const uint16_t* xd, int32_t ntok, float* y /* [ntok][n] */, int32_t lpr);
/* batched layer path (>= 16 tokens): fused gate/up GEMM on the matrix cores + SwiGLU + int8 quantisation; w = [2*ff][k] Q8_0 rows
 * (gate rows first), k = 1024 or 2048; aq [ntok][ff], ad [ntok][ff/32] */
/* K-quant forms of the two entries above: the matrix is built from up to 3 tensors (raw GGUF rows of ggml type 8 = Q8_0, 13 = Q5_K, 14 = Q6_K; row counts
 * multiples of 32) into packed planes exactly as the engine does at load; >= 16 tokens with lpr = 0 take the matrix-core kernel (k_gemm_kq_mfma). */
int q3tts_op_gemv_kq(const void* const* raws, const int32_t* types, const int32_t* rows, int32_t nparts, int32_t k, const int8_t* xq, const uint16_t* xd,
                     int32_t ntok, float* y, int32_t lpr);
int q3tts_op_gateup_kq(const void* gate_raw, const void* up_raw, int32_t type, int32_t ff, int32_t k, const int8_t* xq, const uint16_t* xd, int32_t ntok,
                       int8_t* aq, uint16_t* ad);
int q3tts_op_gateup_q8(const void* w_q8_0, int32_t ff, int32_t k, const int8_t* xq, const uint16_t* xd, int32_t ntok, int8_t* aq,
                       uint16_t* ad);
/* float-weight matmul (spec S3 float form; ggml types 0 = f32, 1 = f16, 30 = bf16): ntok >= 12 runs the matrix-core kernel,
 * fewer tokens the one-wave-per-row GEMV; row0 selects a row range like the head of the code predictor does */
int q3tts_op_matmul_float(const void* w /* [n][k] */, int32_t type, int32_t n, int32_t k, int32_t row0, int32_t nrows,
                          const float* x /* [ntok][k] */, int32_t ntok, float* y /* [ntok][nrows] */);
int q3tts_op_rmsnorm_quant(const float* x, const float* g, int32_t d, int32_t ntok, float eps, int8_t* xq, uint16_t* xd,
                           float* xn);
int q3tts_op_swiglu_quant(const float* gu, int32_t ff, int32_t ntok, int8_t* aq, uint16_t* ad);
int q3tts_op_argmax(const float* logits, int32_t n, int32_t start, int32_t end, int32_t mask_idx, int32_t* out);
/* device sampler (llama/mod.rs:666-776): n_draws consecutive draws of one seeded sequence over logits[0,n), n <= 4096 */
int q3tts_op_sample(const float* logits, int32_t n, float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t mask_idx,
                    int32_t n_draws, int32_t* out);
/* [EXT] the frame graph's sampler launches over B rows of logits [B][n] (host buffers), n_draws consecutive draws per row:
 * kernel 0 = k_sample (talker; n <= 4096; penalty NULL = none, else per row with history hist[b*hist_cap + 0 .. hist_len[b]) of code_0 values,
 * packed into the engine's device layout: the last entry becomes the current frame's key), kernel 1 = k_sample_pred (code predictor;
 * n <= 2048; penalty must be NULL).  Row b's stream is seed_from_u64(seed[b]).  out [n_draws][B]. */
int q3tts_op_sample_rows(int32_t kernel, const float* logits, int32_t B, int32_t n, const float* temperature, const int32_t* top_k,
                         const float* top_p, const float* penalty, const uint64_t* seed, const int32_t* hist, const int32_t* hist_len,
                         int32_t hist_cap, int32_t n_draws, int32_t* out);
/* one row through k_project_mt, the per-frame projection: n_in % 512 == 0 and n_out % 16 == 0; any other shape is refused by the kernel's
 * launcher and leaves y unwritten */
int q3tts_op_project(const float* x, const float* w /* [n_out][n_in] */, const float* b, int32_t n_in, int32_t n_out, float* y);
/* [EXT] test surface of k_logprob_rows, host buffers: logits [B][stride] (n <= stride, n <= 4096), chosen [B], extra_idx < 0 = none;
 * out_chosen [B] = log softmax(row)[chosen], out_extra [B] (or NULL) = log softmax(row)[extra_idx] */
int q3tts_op_logprob_rows(const float* logits, int32_t B, int32_t n, int32_t stride, const int32_t* chosen, int32_t extra_idx,
                          float* out_chosen, float* out_extra);
/* [EXT] scoring test surfaces, host buffers.  k_score_rows: tlogits [F][t_stride] (the first Q3_SAMPLE_END columns of a row count; a
 * t_stride that is no multiple of 4 makes odd rows unaligned), plogits [15][F][2048], codes [F][16] -> out [F][17].  k_score_inputs:
 * hidden_proj [F][dP], tabs[q] = table q of tab_rows[q] rows of dP floats (q = 0..14), codes [F][16] -> out [16 F][dP], row p * F + f =
 * position p of frame f.  Both run with guard values around the device output and fail if the kernel wrote outside it */
int q3tts_op_score_rows(const float* tlogits, int32_t t_stride, const float* plogits, const int32_t* codes, int32_t F, float* out);
int q3tts_op_score_inputs(const float* hidden_proj, const float* const* tabs, const int64_t* tab_rows, int32_t dP, const int32_t* codes,
                          int32_t F, float* out);
/* [EXT] candidate sets test surface of k_kv_fork, host buffers: k_cache / v_cache [n_pages][n_layer][n_kv][8192] f16 bits, uploaded whole and
 * written back whole (a stray write shows); page_table [n_seq][max_pages].  Logical pages [0, ceil(n_positions / 64)) of src_seq are copied
 * into those of dst_seqs[0 .. n_dst-1].  Refused before anything is uploaded or launched: n_dst < 1; a sequence out of range; a destination
 * equal to the source or listed twice; n_positions < 1 or > max_pages * 64; a page-table entry of the copied range outside [0, n_pages);
 * two of the physical pages involved coincide */
int q3tts_op_kv_fork(uint16_t* k_cache, uint16_t* v_cache, int32_t n_pages, int32_t n_layer, int32_t n_kv, const int32_t* page_table,
                     int32_t n_seq, int32_t max_pages, int32_t src_seq, const int32_t* dst_seqs, int32_t n_dst, int32_t n_positions);
/* [EXT] prompt stems test surface of k_kv_stem, host buffers: k_cache / v_cache as q3tts_op_kv_fork takes them; store_k / store_v
 * [n_store_pages][n_layer][n_kv][8192] f16 bits, one arena the jobs' stores lie in; all four are uploaded whole and written back whole (a
 * stray write shows).  Job j: store pages [job_page0[j], job_page0[j] + job_n_pages[j]), slots[job_first[j] .. job_first[j] + job_n_dst[j]).
 * save = 0 restores store page l into logical page l of every listed slot, save = 1 saves logical page l of the job's one slot into store
 * page l; one launch for all jobs.  Refused before anything is uploaded or launched: n_jobs < 1; a job with n_pages outside [1, max_pages], a
 * store range outside the arena, a slot range outside slots, n_dst < 1 (save: != 1); a slot outside [0, n_seq); a page-table entry of a
 * copied range outside [0, n_pages); restore: two destination pages coincide; save: two jobs' store ranges overlap */
int q3tts_op_kv_stem(uint16_t* k_cache, uint16_t* v_cache, int32_t n_pages, int32_t n_layer, int32_t n_kv, const int32_t* page_table,
                     int32_t n_seq, int32_t max_pages, uint16_t* store_k, uint16_t* store_v, int32_t n_store_pages, int32_t n_jobs,
                     const int32_t* job_page0, const int32_t* job_n_pages, const int32_t* job_first, const int32_t* job_n_dst,
                     const int32_t* slots, int32_t n_slots, int32_t save);
/* [EXT] resume test surface, host buffers: rows [n][2048] = the feedback rows of codes [n][16] (+ trail ids [n_trail], row f takes id f
 * while f < n_trail; NULL / 0 = every row adds tts_pad) against the given tables (k_feedback_codes) */
int q3tts_op_feedback_rows(const q3tts_assets* a, const int32_t* codes, int32_t n, const int32_t* trail_ids, int32_t n_trail, float* rows);
/* One codec-decoder GEMM (csrc/codec.hip), as the decoder runs it or with a named kernel form forced.  out[m][n] = epilogue(sum_k A'[m][k] W[n][k]
 * + bias[n]) with K = taps * cin, k = j * cin + ci -> A' row m + (m / a_segT) * a_skip + j * dil, channel ci (a_segT = 0: unsegmented).  Output row m
 * starts at out_off + m * ldo + (m / o_segT) * o_skip floats of the out buffer, residual row m at m * ldr + (m / r_segT) * r_skip floats of res.
 * W is split into hi / lo f16 planes exactly as the decoder does at load.  `out` is read (uploaded) and written back whole, padding included. */
enum { Q3TTS_GEMM_AUTO = 0, Q3TTS_GEMM_SKINNY4 = 1, Q3TTS_GEMM_SKINNY8 = 2, Q3TTS_GEMM_SKINNY16 = 3, /* k_skinny_gemm<4|8|16>, exact f32 */
       Q3TTS_GEMM_F32_1 = 4, Q3TTS_GEMM_F32_2 = 5,                                                  /* k_conv_gemm<1|2>, f32 MFMA */
       Q3TTS_GEMM_H1 = 6, Q3TTS_GEMM_H1_EPL = 7, Q3TTS_GEMM_H2 = 8, Q3TTS_GEMM_H2_EPL = 9,           /* k_conv_gemm_h<MR, EPL>, split f16 */
       Q3TTS_GEMM_H3 = 10, Q3TTS_GEMM_H3_EPL = 11 };                                                /* k_conv_gemm_h3<..., EPL>, split f16 */
enum { Q3TTS_EPI_NONE = 0, Q3TTS_EPI_GELU = 1, Q3TTS_EPI_RES_SCALE = 2 /* res + scale[n] * v */, Q3TTS_EPI_RES = 3 /* res + v */,
       Q3TTS_EPI_SNAKE = 4 /* v + ib[n] * sin^2(ea[n] * v) */ };
typedef struct q3tts_codec_gemm_desc {
    int32_t M, N, cin, taps, dil;
    const float* A; int64_t a_rows; int32_t lda, a_segT, a_skip;      /* A: a_rows x lda floats, history rows included */
    int32_t a_split, o_split;                                          /* rows stored as [C x f16 hi][C x f16 lo] (input / output) */
    const float* W; const float* bias;                                 /* W [N][K] f32; bias [N] or NULL */
    int32_t epi; const float* res; int64_t res_floats; int32_t ldr, r_segT; int64_t r_skip;
    const float* scale; const float* snake_ea; const float* snake_ib;  /* [N] each, where the epilogue uses them */
    float* out; int64_t out_floats, out_off; int32_t ldo, o_segT; int64_t o_skip;
    int64_t ws_floats;                                                 /* split-K workspace */
    int32_t form, ksplit, reducer;  /* Q3TTS_GEMM_*; forced forms: ksplit >= 1 and reducer 0 = k_splitk_reduce, 1 = k_splitk_reduce4, -1 = none (ksplit 1) */
    int32_t form_ran, ksplit_ran, reducer_ran;                         /* out: what ran (AUTO: what the decoder's dispatcher chose) */
} q3tts_codec_gemm_desc;
/* test entry: runs the GEMM (a forced form whose preconditions fail returns an error and launches nothing) */
int q3tts_op_codec_gemm(q3tts_codec_gemm_desc* d);
/* host only (no device needed): the decoder's dispatch for d's shape -> form_ran / ksplit_ran / reducer_ran.  Pointers are not dereferenced:
 * NULL stands for a 16-byte aligned buffer (out_off still applies) */
int q3tts_codec_gemm_plan(q3tts_codec_gemm_desc* d);
/* host only: 1 if the GEMM d describes (form AUTO: as the decoder dispatches it; a forced form: form / ksplit as given) runs k_conv_gemm_h3's
 * tap-reusing main loop, 0 if it runs a tap-major loop, < 0 on a bad descriptor.  Pointers are not dereferenced */
int q3tts_codec_gemm_tap_reuse(const q3tts_codec_gemm_desc* d);

/* One codec-decoder kernel other than the GEMMs (csrc/codec.hip), launched as decode_group_async launches it.  R = G * T logical rows: stream g's
 * rows are g*T .. g*T+T-1.  An "extended" buffer is [G][H + T][C]: per stream H history rows (right-aligned), then the T new rows.
 *   RVQ_SUM         codes [R][n_q] (clamped to [0, cb_size)), in[0] codebooks [n_q][cb_size][C] -> out[0] extended, new rows written
 *   RMSNORM_ROWS    in[0] x [R][C] (NULL: in place on out[0]), p0 gain [C], eps -> out[0] [R][C]
 *   LAYERNORM_ROWS  the same with p0 weight, p1 bias (two-pass mean / variance)
 *   ROPE_APPEND     C = n_heads * head_dim; out[0] qkv [R][3C] rotated in place (NeoX, position meta[2G+g] + t, rope_base), out[1] K and out[2] V
 *                   extended (H = window - 1), new rows written.  Every position must be below Q3TTS_CODEC_MAX_FRAMES.
 *   WINDOW_ATTN     in[0] qkv [R][3C] (q read), in[1] K, in[2] V extended (H = window - 1, last meta[G+g] history rows valid) -> out[0] [R][C];
 *                   row t attends to the window - 1 positions before it and itself; head_dim and window <= 128
 *   SWIGLU_ROWS     in[0] gate|up [R][2C] -> out[0] [R][C]
 *   DWCONV7         in[0] extended (H = 6), p0 w [C][7], p1 bias [C] -> out[0] [R][C] (causal depthwise, tap 6 = the current row)
 *   SNAKE[_SPLIT]   in[0] [R][C], p0 exp(alpha) [C], p1 1/(exp(beta)+1e-9) [C] -> out[0] extended, new rows (SPLIT: [C f16 hi][C f16 lo]); C % 4 == 0
 *   CONV_OUT_WAVE / CONV_OUT_WIN  in[0] extended (H = 6), p0 w [7][C] (tap-major), bias -> out[0] pcm [R] clamped to [-1, 1];
 *                   C % 4 == 0; WIN (k_conv_out_win<96>): C == 96 and T % 128 == 0
 *   HIST_LOAD       in[0] store [n_streams][H][C] -> out[0] extended: stream g's history rows from slot meta[g]
 *   HIST_SAVE       in[0] extended -> out[0] store: the last H rows of (history + new rows) of stream g into slot meta[g]
 *   HIST_ZERO       out[0] store: slot `stream` zeroed
 * meta [3G] = stream slot, cached K/V rows, frames seen, as the decoder uploads it per call.  Outputs are uploaded and written back whole, so
 * anything a kernel writes outside its logical output shows.  A kernel whose preconditions fail returns an error and launches nothing. */
enum { Q3TTS_CK_RVQ_SUM = 0, Q3TTS_CK_RMSNORM_ROWS = 1, Q3TTS_CK_LAYERNORM_ROWS = 2, Q3TTS_CK_ROPE_APPEND = 3, Q3TTS_CK_WINDOW_ATTN = 4,
       Q3TTS_CK_SWIGLU_ROWS = 5, Q3TTS_CK_DWCONV7 = 6, Q3TTS_CK_SNAKE = 7, Q3TTS_CK_SNAKE_SPLIT = 8, Q3TTS_CK_CONV_OUT_WAVE = 9,
       Q3TTS_CK_CONV_OUT_WIN = 10, Q3TTS_CK_HIST_LOAD = 11, Q3TTS_CK_HIST_SAVE = 12, Q3TTS_CK_HIST_ZERO = 13 };
typedef struct q3tts_codec_kernel_desc {
    int32_t kernel;
    int32_t G, T, C, H;                                   /* streams, new rows per stream, channels, history rows per extended segment */
    int32_t n_heads, head_dim, window; float rope_base, eps, bias;
    const int64_t* meta;                                  /* [3G] */
    const int64_t* codes; int32_t n_q, cb_size;           /* RVQ_SUM */
    int32_t n_streams, stream;                            /* HIST_*: slots of the store; HIST_ZERO: the slot */
    const float* in[3]; int64_t in_floats[3];
    const float* p0; const float* p1; int64_t p0_floats, p1_floats;
    float* out[3]; int64_t out_floats[3];
} q3tts_codec_kernel_desc;
int q3tts_op_codec_kernel(q3tts_codec_kernel_desc* d);

/* One transformer attention step (spec S4' per-head RMSNorm, S5 M-RoPE, S6 f16 KV append, S7 causal GQA attention, S2 quantisation of the
 * output) for one layer, as Transformer::forward dispatches it or with a named kernel form forced.  Every buffer is a host buffer.
 *   qkv      [ntok] rows of qkv_stride floats: n_head q heads, n_kv k heads, n_kv v heads of 128 each
 *   tokens   uniform_pos >= 0: token t is sequence t at slot uniform_pos, all four position streams = uniform_pos (seq / slot / pos unused);
 *            otherwise seq[t], slot[t] (the cache position written, = #cached before it) and pos[t][4]
 *   paging   page_table [n_seq][max_pages] of physical pages, or NULL = identity (sequence s owns page s; slots < 64)
 *   caches   K [n_pages][n_layer][n_kv][16][64][8] and V [n_pages][n_layer][n_kv][64][128] f16, uploaded and written back whole
 *   RoPE     tables built as the Transformer builds them from rope_base for n_ctx positions; positions are clamped to [0, n_ctx-1]
 *   outputs  att [ntok][n_head*128] f32 (UNFUSED, SHORT1/2, GGML; may be NULL), aq [ntok][n_head*128] / ad [ntok][n_head*4] (every form but GGML)
 * AUTO runs what plan_attention picks for the flags below (hpw1_max <= 0: the engine's threshold); form_ran reports the form.  A form whose
 * preconditions fail returns an error and launches nothing. */
enum { Q3TTS_ATTN_AUTO = 0, Q3TTS_ATTN_UNFUSED = 1 /* k_qk_rope_append + k_attention */, Q3TTS_ATTN_FUSED = 2 /* k_attention_fused */,
       Q3TTS_ATTN_SHORT1 = 3, Q3TTS_ATTN_SHORT2 = 4 /* k_attention_short<1|2> */, Q3TTS_ATTN_GGML = 5 /* k_gg_qk_rope_append + k_gg_attention */ };
typedef struct q3tts_attention_desc {
    int32_t n_head, n_kv, n_layer, layer, ntok;
    const float* qkv; int32_t qkv_stride;
    const float* q_norm; const float* k_norm;                          /* [128] each */
    float eps, rope_base; int32_t n_ctx; int32_t mrope_sec[4];
    const int32_t* seq; const int32_t* slot; const int32_t* pos; int32_t uniform_pos;
    const int32_t* page_table; int32_t n_seq, max_pages;
    uint16_t* k_cache; uint16_t* v_cache; int32_t n_pages;
    int32_t fused, fused_max_tok, same_seq, short_attn_min, hpw1_max, float_mode, ggml_mode; /* AUTO's Transformer flags */
    int32_t form;
    float* att; int8_t* aq; uint16_t* ad;
    int32_t form_ran;
} q3tts_attention_desc;
int q3tts_op_attention(q3tts_attention_desc* d);
/* the same step with d->qkv holding a table of qkv_rows rows (qkv_stride floats each): token t reads the row the low word of
 * keys[t * key_stride] selects (an argmax key, q3tts_argmax_key), as the code predictor's layer 0 reads its q/k/v table.  Every form but GGML.
 * The table is uploaded whole and written back whole into d->qkv. */
int q3tts_op_attention_keyed(q3tts_attention_desc* d, const uint64_t* keys, int32_t key_stride, int32_t qkv_rows);
/* host only (no device needed): the form AUTO picks for d's ntok / n_head / n_kv / flags -> form_ran; no buffer is read */
int q3tts_attention_plan(q3tts_attention_desc* d);

/* One talker / predictor linear-layer operation (csrc/kernels.hip, kernels_fused.hip) with a form forced, or as the engine dispatches it (AUTO).
 * Ops: GEMV int8 x -> f32 super-segment slabs out[out_off + (s*ntok + t)*out_stride + r], s < ceil(K/2048), NOT summed;
 *      GATEUP int8 x -> SwiGLU -> aq [ntok][ff] / ad [ntok][ff/32] (weights: gate rows [0, ff) then up rows);
 *      NORM  h = h_in (+ parts) -> xq_out / xd_out [ntok][K] (+ h_out, xn_out);  NORM_GEMV: the same prologue -> f32 rows out[out_off + t*out_stride + r];
 *      NORM_ARGMAX: the prologue -> keys[t*key_stride] (atomic first-max over rows [0, nrows_valid));  NORM_GATEUP: the prologue -> aq / ad;
 *      F_GEMV f32 x -> f32 rows (out_off / out_stride as NORM_GEMV);  F_GATEUP f32 x -> SwiGLU -> f32 act out[out_off + t*out_stride + j], j < ff.
 * Forced-form preconditions (refused before any allocation or launch; all forms: K % 256 == 0, 0 <= row0, row0 + nrows <= rows of the matrix):
 *   GEMV_Q8 (k_gemv_q8<LPR,MT>)        Q8_0 weights; lpr in {2,4,8}, mt in {1,2,4,8}
 *   GEMM_Q8_TOK (k_gemm_q8_tok)        Q8_0 weights
 *   GEMM_Q8_MFMA (k_gemm_q8_mfma)      Q8_0 weights; 1 <= ztiles <= ceil(ntok/32)
 *   GEMM_Q8_TILE1 (k_gemm_q8_tile1)    Q8_0; K <= 1024; nrows % 4 == 0; out_stride % 4 == 0; out + out_off 16-byte aligned; ztiles == ceil(ntok/32)
 *   GEMV_KQ (k_gemv_kq<LPR,MT,TS>)     K-quant-file weights (any mix of Q5_K / Q6_K / Q8_0 tensors); lpr in {2,4,8}, mt in {1,2,4,8}
 *   GEMM_KQ_MFMA (k_gemm_kq_mfma)      K-quant-file weights; 1 <= ztiles <= ceil(ntok/32)
 *   GU_Q8_TILE1 / GU_Q8_MFMA           Q8_0; K in {1024, 2048}; ff % 32 == 0; ceil(ntiles/4) <= ztiles <= ntiles (TILE1: ztiles == ntiles)
 *   GU_KQ_MFMA                         K-quant-file weights of ONE tensor type; the same K / ff / ztiles rules
 *   GU_UNFUSED                         the GEMV the engine would run (any weights) + k_swiglu_quant; ff % 32 == 0; K <= 2048 (one slab)
 *   NORM (k_rmsnorm_quant)             K <= 2048; parts_slab == ntok * parts_stride; takes idx (int32 rows) or idx_keys
 *   NORM_WG (k_rmsnorm_quant_wg)       K <= 2048; no int32 idx
 *   GEMV_NORM (k_gemv_q8_norm<LPR,MT,0>), GEMV_NORM_ARGMAX (<2,MT,1>), GU_SWIGLU_NORM (k_gateup_swiglu<MT,NSEG,TS>)
 *                                      K <= 2048; no int32 idx; GEMV_NORM lpr in {2,4,8}; ARGMAX lpr 2; mt in {1,2,4,8} (GU: {1,2,4});
 *                                      GU_SWIGLU_NORM: gate and up rows of one tensor type, ff % 32 == 0
 *   F_GEMV (k_gemv_float<T,MT,1>)      float weights; mt in {1,2,4,8}
 *   F_MFMA16 / F_MFMA                  float weights; row0 % 64 == 0; x 16-byte aligned; x_stride % 4 == 0
 *   F_GU_MFMA16                        the same, nrows == 2 * ff, ff % 16 == 0 (the engine's 2..95-token window is a dispatch choice only)
 *   F_GU_UNFUSED                       the float GEMV the engine would run + k_swiglu_f32
 *   GEMM_Q8_WIDE (k_gemm_q8_wide<0>)   Q8_0 weights; ztiles == ceil(ntok/32).  AUTO above 256 tokens.  It stores single floats: any out / out_stride
 *                                      the op accepts is accepted
 *   GU_Q8_WIDE (k_gemm_q8_wide<1>)     Q8_0; K in {1024, 2048}; ff % 32 == 0; ztiles == ceil(ntok/32).  AUTO above 256 tokens
 * Every buffer is uploaded whole and written back whole, so bytes outside the logical outputs show any stray write. */
enum { Q3TTS_LOP_GEMV = 0, Q3TTS_LOP_GATEUP = 1, Q3TTS_LOP_NORM = 2, Q3TTS_LOP_NORM_GEMV = 3, Q3TTS_LOP_NORM_ARGMAX = 4, Q3TTS_LOP_NORM_GATEUP = 5,
       Q3TTS_LOP_F_GEMV = 6, Q3TTS_LOP_F_GATEUP = 7 };
enum { Q3TTS_LIN_AUTO = 0, Q3TTS_LIN_GEMV_Q8 = 1, Q3TTS_LIN_GEMM_Q8_TOK = 2, Q3TTS_LIN_GEMM_Q8_MFMA = 3, Q3TTS_LIN_GEMM_Q8_TILE1 = 4,
       Q3TTS_LIN_GEMV_KQ = 5, Q3TTS_LIN_GEMM_KQ_MFMA = 6, Q3TTS_LIN_GU_Q8_TILE1 = 7, Q3TTS_LIN_GU_Q8_MFMA = 8, Q3TTS_LIN_GU_KQ_MFMA = 9,
       Q3TTS_LIN_GU_UNFUSED = 10, Q3TTS_LIN_NORM = 11, Q3TTS_LIN_NORM_WG = 12, Q3TTS_LIN_GEMV_NORM = 13, Q3TTS_LIN_GEMV_NORM_ARGMAX = 14,
       Q3TTS_LIN_GU_SWIGLU_NORM = 15, Q3TTS_LIN_F_GEMV = 16, Q3TTS_LIN_F_MFMA16 = 17, Q3TTS_LIN_F_MFMA = 18, Q3TTS_LIN_F_GU_MFMA16 = 19,
       Q3TTS_LIN_F_GU_UNFUSED = 20, Q3TTS_LIN_GEMM_Q8_WIDE = 21, Q3TTS_LIN_GU_Q8_WIDE = 22 };
typedef struct q3tts_linear_desc {
    int32_t op, form;
    /* weights: quantised = up to 3 raw GGUF tensors [rows[i]][K] of type[i] (8 Q8_0, 13 Q5_K, 14 Q6_K; all-Q8_0 = the Q8_0 file layout unless
     * kq_layout != 0); float = raw[0] [rows[0]][K] of type[0] (0 f32, 1 f16, 30 bf16) */
    int32_t nw; const void* raw[3]; int32_t type[3]; int32_t rows[3]; int32_t kq_layout;
    int32_t K, row0, nrows, nrows_valid, ntok, ff;
    int32_t lpr, mt, ztiles;       /* forced parameters, 0 = the plan's */
    int32_t fused;                 /* GATEUP AUTO: the Transformer's fused switch */
    const int8_t* xq; const uint16_t* xd; int32_t a_rows;                 /* int8 inputs [a_rows][K], [a_rows][K/32], a_rows >= ntok */
    const float* x; int64_t x_floats; int32_t x_off, x_stride;             /* float inputs: row t at x + x_off + t*x_stride */
    const float* h_in; int64_t h_floats; int32_t h_stride;                 /* norm prologue (NormPro) */
    const uint64_t* idx_keys; const int32_t* idx; int32_t idx_stride;      /* row select: argmax key (low word ~index) or int32 (NORM only) */
    const float* parts; int64_t parts_floats; int32_t nparts, parts_stride; int64_t parts_slab;
    const float* g; float eps;
    float* h_out; float* xn_out;                                           /* [ntok][K] each, or NULL */
    int8_t* xq_out; uint16_t* xd_out;                                      /* NORM / NORM_WG: [ntok][K], [ntok][K/32] */
    uint64_t* keys; int64_t n_keys; int32_t key_stride; const int32_t* mask_per_tok; int32_t idx_add;  /* argmax epilogue */
    float* out; int64_t out_floats, out_off; int32_t out_stride;
    int8_t* aq; uint16_t* ad;                                              /* gate/up: [ntok][ff], [ntok][ff/32] */
    int32_t form_ran, lpr_ran, mt_ran, z_ran;                              /* out: what ran */
} q3tts_linear_desc;
int q3tts_op_linear(q3tts_linear_desc* d);
/* host only (no device needed): the engine's dispatch for d's op and shape -> form_ran / lpr_ran / mt_ran / z_ran.  Buffers are not read; their
 * addresses count only for alignment (NULL = aligned; out_off and x_off still apply). */
int q3tts_linear_plan(q3tts_linear_desc* d);
/* host only: the argmax key the device packs for logit v at index idx (kdev.h pack_key: order-preserving value bits, ~idx, -0 as +0) */
uint64_t q3tts_argmax_key(float v, int32_t idx);

/* [EXT] test surface of the four token-selection kernels, host buffers: k_sample, k_sample_pred, k_argmax, k_argmax_keys over B rows
 * logits [B][n], with everything SampleArgs / launch_argmax / launch_argmax_keys take.  On the device row b starts row_off + b*stride floats
 * into its buffer; the floats before row 0 and columns [n, stride) of every row hold 3e38f (a kernel that reads one changes its pick).
 * Launch i of n_draws (the argmax kernels run once) writes slot b*out_stride of its own B*out_stride output slots; every slot is pre-set to
 * Q3TTS_SELECT_SENTINEL (k_argmax: its low 32 bits, the slots are int32 there) and the whole array comes back in out_raw.
 * Shapes a launcher refuses (SAMPLE: n > 4096; SAMPLE_PRED: n > 2048, a penalty or a mask) fail through that launcher's own check and leave
 * tokens / out_raw / draws_out unwritten. */
enum { Q3TTS_SEL_SAMPLE = 0, Q3TTS_SEL_SAMPLE_PRED = 1, Q3TTS_SEL_ARGMAX = 2, Q3TTS_SEL_ARGMAX_KEYS = 3 };
#define Q3TTS_SELECT_SENTINEL 0xA5C3F00D5A3C0FF1ull
typedef struct q3tts_select_desc {
    int32_t kernel;                  /* Q3TTS_SEL_* */
    int32_t B, n, stride, row_off;   /* stride >= n, row_off >= 0 */
    const float* logits;             /* [B][n] */
    const float* temperature; const int32_t* top_k; const float* top_p;   /* [B] each (samplers) */
    const int32_t* mask_idx;         /* optional [B]; < 0 = none */
    const uint64_t* seed;            /* [B] (samplers): row b's stream is seed_from_u64(seed[b]) ... */
    const uint32_t* draw0;           /* optional [B]: ... read from word draw0[b] on (NULL = 0) */
    int32_t n_draws;                 /* samplers: consecutive launches over the same rows */
    /* penalty block (NULL penalty = none): hist [B][hist_cap] holds row b's codes as given, out-of-range values included, hist_len [B]
     * <= hist_cap; cur_code NULL = the launch's cur_key is null, else [B] codes packed into keys (cur_stride 16) */
    const float* penalty; const int32_t* hist; const int32_t* hist_len; int32_t hist_cap; const int32_t* cur_code;
    int32_t out_stride;              /* 1 or 16 */
    int32_t start, end, add;         /* ARGMAX: 0 <= start <= end <= n */
    int32_t* tokens;                 /* out [n_draws][B] */
    uint64_t* out_raw;               /* out [n_draws][B*out_stride] (ARGMAX: the int32 slots zero-extended) */
    uint32_t* draws_out;             /* out [B]: the draw counters after the last launch (samplers) */
} q3tts_select_desc;
int q3tts_op_select_rows(q3tts_select_desc* d);

/* [EXT] test surface of the glue kernels between the GEMMs of a decode frame, host buffers: one call uploads what the caller gives, makes
 * exactly one launch through the launcher the engine calls, and downloads everything.  Inputs are synthetic: tables of any row count, a
 * row-major weight [n_out][n_in] (Wt / Wblk are built by the engine's own layout helpers), keys as raw 64-bit words.
 * A q3tts_guarded buffer is in/out and arrives WHOLE: Q3TTS_GLUE_GUARD guard elements, the core, Q3TTS_GLUE_GUARD guard elements.  The
 * device works at element Q3TTS_GLUE_GUARD; the caller pre-sets guards, stride padding and the state of one slot past ntok to a sentinel of
 * its choice and finds every stray write in what comes back.  `n` counts the whole buffer; the core may be larger than the minimum below.
 * Only what keeps the launch inside its buffers is checked here; what a launcher refuses (PROJECT_MT: n_in % 512, n_out % 16, x_stride % 4,
 * a row address off 16 bytes) fails through that launcher and leaves every buffer unwritten.
 *   PROJECT_MT         out[t*out_stride + o] = project(x row t), t < ntok; x holds the rows as the device sees them (row t at t*x_stride,
 *                      gaps included) and lands x_off floats past a 256-byte aligned address, 16 rows of 3e38 behind it.  out core >= ntok*out_stride
 *   PROJECT_TABLE      x = table [ntok][n_in], out core >= ntok*n_out (dense rows)
 *   (every table of the two kernels below sits between two rows of 3e38 on the device)
 *   FEEDBACK_KEYS      16 tables [table_rows[q]][2048], keys core >= ntok*key_stride (key_stride >= 16), tts_pad [2048], out core >= ntok*2048.
 *                      trail != 0: the TextTrail form over n_frames (guarded, core >= ntok), n_trail [ntok] <= ids_stride,
 *                      trail_ids [ntok][ids_stride], text_table [text_rows][2048]
 *   GATHER_ROWS_KEYS   tables[0] = [table_rows[0]][row_len], keys core >= ntok*key_stride, out core >= ntok*row_len
 *   ADVANCE_KEYS       AdvanceKeysArgs over ntok slots: keys core >= ntok*16, next_key0 / finished / n_frames / t_slot >= ntok, t_pos >= 4*ntok,
 *                      hist >= ntok*hist_stride, max_frames [ntok] with max_frames*16 <= hist_stride
 *   STALL_SAVE, ADVANCE_KEYS_GATED   the same plus StallArgs: open / n_trail [ntok], hidden / save_hidden >= ntok*2048, draws / pdraws >= ntok,
 *                      save_draws >= 2*ntok */
enum { Q3TTS_GLUE_PROJECT_MT = 0, Q3TTS_GLUE_PROJECT_TABLE = 1, Q3TTS_GLUE_FEEDBACK_KEYS = 2, Q3TTS_GLUE_GATHER_ROWS_KEYS = 3,
       Q3TTS_GLUE_ADVANCE_KEYS = 4, Q3TTS_GLUE_STALL_SAVE = 5, Q3TTS_GLUE_ADVANCE_KEYS_GATED = 6 };
#define Q3TTS_GLUE_GUARD 64
typedef struct q3tts_guarded { void* p; int64_t n; } q3tts_guarded;
typedef struct q3tts_frame_glue_desc {
    int32_t kernel;                  /* Q3TTS_GLUE_* */
    int32_t ntok;                    /* token rows, table rows (PROJECT_TABLE) or slots B */
    int32_t n_in, n_out, x_stride, x_off, out_stride;
    const float* x; int64_t x_floats;
    const float* w; const float* b;  /* [n_out][n_in], [n_out] */
    const float* const* tables; const int64_t* table_rows;
    int32_t row_len, key_stride;
    const float* tts_pad;
    int32_t trail; const int32_t* trail_ids; int32_t ids_stride; const float* text_table; int64_t text_rows;
    const int32_t* n_trail; const int32_t* open; const int32_t* max_frames;
    int32_t hist_stride;
    q3tts_guarded out;               /* float */
    q3tts_guarded keys, next_key0;   /* uint64 */
    q3tts_guarded finished, n_frames, t_slot, t_pos, hist;   /* int32 */
    q3tts_guarded hidden, save_hidden;                       /* float */
    q3tts_guarded draws, pdraws, save_draws;                 /* uint32 */
} q3tts_frame_glue_desc;
int q3tts_op_frame_glue(q3tts_frame_glue_desc* d);

/* [EXT] test surface of the ggml-mode kernels (csrc/ggml_mode.hip; Q3_SPEC=ggml), host buffers, no model: one call uploads what the caller
 * gives, runs ONE launcher of ggml_mode.h on it (LINEAR: gg_quant then gg_matvec, as Transformer::gg_linear chains them) and downloads every
 * guarded buffer whole.  Guarded buffers follow q3tts_op_frame_glue: Q3TTS_GLUE_GUARD guard elements, the core, as many guard elements; the
 * device works at element Q3TTS_GLUE_GUARD, the core may be larger than the minimum, and whatever the caller pre-set outside the logical
 * output shows a stray write.
 *   LOAD_ROWS  out[t*k + i] = x[row(t)*x_stride + i], i < k: row(t) = t, idx[t*idx_stride] or the code of idx_keys[t*idx_stride] (an argmax
 *              key); x holds x_rows rows (x_floats >= (x_rows-1)*x_stride + k, x_stride >= k), every selected row is checked against x_rows,
 *              idx / idx_keys hold idx_n >= (ntok-1)*idx_stride + 1 entries.  out core >= ntok*k
 *   ADD        out[i] = out[i] + x[i], i < n.  x_floats >= n, out core >= n
 *   RMSNORM    out [ntok][k] = ggml's RMSNorm of x [ntok][k] with weight u [k] and eps
 *   QUANT      x [ntok][k] f32 (k % 256 == 0) -> q8 [ntok][k], d8 [ntok][k/32] (f16 bits), qk [ntok][k], dk [ntok][k/256], bs [ntok][k/16]
 *   MATVEC     out[t*out_stride + r] = W[row0 + r] . activation row t, r < nrows, from the five quantised arrays as given (all five are
 *              required; the kernel reads q8 / d8 for type 8 and qk / dk / bs for types 13 / 14).  W = `rows` raw GGUF rows of k weights of
 *              `type`.  out_stride >= nrows, out core >= (ntok-1)*out_stride + nrows
 *   LINEAR     QUANT of x, then MATVEC: the five arrays come back as QUANT left them
 *   SWIGLU     out[i] = silu(x[i]) * u[i], i < n
 * Refusals happen before anything is uploaded and leave every buffer unwritten: what gg_matvec refuses (a type other than 8 / 13 / 14, a row
 * range outside [0, rows]), a buffer too small for its shape, ntok > 65535.  MATVEC / LINEAR with nrows == 0 or ntok == 0 (after those
 * checks), and every other op with ntok == 0 (ADD / SWIGLU: n == 0), are no-ops that write nothing. */
enum { Q3TTS_GG_LOAD_ROWS = 0, Q3TTS_GG_ADD = 1, Q3TTS_GG_RMSNORM = 2, Q3TTS_GG_QUANT = 3, Q3TTS_GG_MATVEC = 4, Q3TTS_GG_LINEAR = 5,
       Q3TTS_GG_SWIGLU = 6 };
typedef struct q3tts_ggml_desc {
    int32_t op;                      /* Q3TTS_GG_* */
    int32_t ntok, k;                 /* token rows and their width (LOAD_ROWS / RMSNORM: the row length d) */
    int64_t n;                       /* ADD / SWIGLU: elements */
    const float* x; int64_t x_floats; int32_t x_stride; int32_t x_rows;   /* x_stride / x_rows: LOAD_ROWS only */
    const float* u; float eps;       /* RMSNORM: weight [k]; SWIGLU: up [n] */
    const int32_t* idx; const uint64_t* idx_keys; int32_t idx_stride; int64_t idx_n;
    const void* w; int32_t type, rows, row0, nrows, out_stride;
    q3tts_guarded out;               /* float */
    q3tts_guarded q8, d8, qk, dk, bs;   /* int8, uint16, int8, float, int16 */
} q3tts_ggml_desc;
int q3tts_op_ggml(q3tts_ggml_desc* d);

/* [EXT] output formats (q3tts_spec.h "output formats"): sample-rate conversion and int16 PCM on the device, behind the codec.
 * Host only, no device needed:
 *   q3tts_pcm_out_plan     L, M, the prototype's tap count N and the most taps one output sample sums (24000: 1, 1, 0, 0); < 0 for a
 *                          rate that is not one of the eight.  Any out pointer may be NULL
 *   q3tts_pcm_out_filter   the f32 prototype h32[0..N) the converter uploads, into h32[cap]; returns N, < 0 for an unknown rate or cap < N
 *   q3tts_pcm_out_samples  output samples of n_native native samples from a stream's reset, floor(n_native L / M); < 0 for an unknown rate
 *   q3tts_pcm_format_check 0 for a format the converter delivers, < 0 (and q3tts_last_error) for an unknown rate or encoding or f32 above 24000
 * q3tts_op_pcm_convert is the test surface of the convert kernel, host buffers in the style of q3tts_op_frame_glue: G streams run through
 * n_chunks launches of the engine's own launcher, one per chunk, on a fresh converter (every history entry is read from half 0 of the
 * store first; a slot's live half flips with each chunk it converts).
 *   in            the chunks one after the other, chunk c = [G][chunk_samples[c]] native f32 samples (position g of every chunk is stream g)
 *   chunk_samples native samples per stream of each chunk; the launcher refuses what is no positive multiple of 1920
 *   streams       [n_chunks][G]: the history slot of position g in chunk c, out of n_streams
 *   fmt           [G]; a native stream's samples are copied through as the engine's copy does
 *   reset_before  [n_chunks][G] or NULL: nonzero = that position's slot is reset ahead of the chunk
 *   out           [G] WHOLE buffers of out_bytes[g] bytes: Q3TTS_GLUE_GUARD guard elements of the stream's encoding, the core, as many guard
 *                 elements.  Stream g's output is appended from the core's first element on, chunk after chunk; n_out[g] = its sample count
 *   hist_store    in/out, WHOLE: Q3TTS_GLUE_GUARD floats, [n_streams][2][96], Q3TTS_GLUE_GUARD floats
 * Everything is checked before anything is launched; a refused call leaves every buffer unwritten. */
int q3tts_pcm_out_plan(int32_t rate, int32_t* L, int32_t* M, int32_t* n_taps, int32_t* taps_per_phase);
int64_t q3tts_pcm_out_filter(int32_t rate, float* h32, int64_t cap);
int64_t q3tts_pcm_out_samples(int32_t rate, int64_t n_native);
int q3tts_pcm_format_check(const q3tts_pcm_format* f);
int q3tts_op_pcm_convert(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                         const q3tts_pcm_format* fmt, const int32_t* reset_before, void* const* out, const int64_t* out_bytes, int64_t* n_out,
                         float* hist_store);

/* [EXT] speaking rate (q3tts_spec.h "speaking rate"): the WSOLA stretcher on the device, behind the codec.
 * Host only, no device needed:
 *   q3tts_tsm_samples  samples delivered for n_native native samples from a stream's reset: 480 * #{k : a_k + 1200 <= n_native} while
 *                      streaming (final = 0), 480 * ceil(100 n_native / (480 rate_pct)) once flushed (final != 0); < 0 for a rate outside [50, 200]
 *   q3tts_tsm_windows  the two normative 480-entry f32 tables w and w2
 * q3tts_op_tsm is the test surface of the stretch kernel, host buffers in the style of q3tts_op_pcm_convert: G streams run through n_chunks
 * launches of the engine's own launcher, one per chunk, and one more (no input, flush) when `flush` is nonzero, on a fresh stretcher.
 *   in            the chunks one after the other, chunk c = [G][chunk_samples[c]] native f32 samples (position g of every chunk is stream g)
 *   chunk_samples native samples per stream of each chunk; the launcher refuses what is no positive multiple of 1920
 *   streams       [n_chunks][G]: the state slot of position g in chunk c, out of n_streams; the flush takes the last chunk's
 *   rate_pct      [G]; a stream at 100 is copied through as native f32, as the engine's copy does
 *   encoding      [G]: 0 = f32, 1 = s16
 *   reset_before  [n_chunks][G] or NULL: nonzero = that position's slot is reset ahead of the chunk
 *   out           [G] WHOLE buffers of out_bytes[g] bytes: Q3TTS_GLUE_GUARD guard elements of the stream's encoding, the core, as many guard
 *                 elements.  Stream g's hops are appended from the core's first element on; n_out[g] = its sample count
 *   delta_trace   [G] WHOLE int32 buffers of trace_len[g] entries: Q3TTS_GLUE_GUARD guards, one d_k per synthesis frame, as many guards
 *   hist_store    in/out, WHOLE: Q3TTS_GLUE_GUARD floats, [n_streams][1920], Q3TTS_GLUE_GUARD floats
 * Everything is checked before anything is launched; a refused call leaves every buffer unwritten. */
int64_t q3tts_tsm_samples(int32_t rate_pct, int64_t n_native, int32_t final);
int q3tts_tsm_windows(float* w, float* w2);
int q3tts_op_tsm(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                 const int32_t* rate_pct, const int32_t* encoding, const int32_t* reset_before, int32_t flush, void* const* out,
                 const int64_t* out_bytes, int64_t* n_out, int32_t* const* delta_trace, const int64_t* trace_len, float* hist_store);

/* [EXT] pitch (q3tts_spec.h "pitch"): the pitch shifter on the device, behind the codec.
 * Host only, no device needed:
 *   q3tts_pitch_samples  samples delivered for n_native native samples from a stream's reset at the pair (rate_pct, pitch_pct): ceil(480 f L / M)
 *                        with f the stage-1 frames, #{k : a_k + 1200 <= n_native} while streaming (final = 0), ceil(pitch n_native / (480 rate))
 *                        once flushed; < 0 for a value or the pair out of range
 *   q3tts_pitch_plan     L / M = 100 / pitch_pct in lowest terms, the taps of the prototype and the most terms one sample sums (outputs may
 *                        be NULL); < 0 for a pitch out of range
 *   q3tts_pitch_filter   the normative f32 prototype h32 of pitch_pct into h32[cap]; returns its length, < 0 when cap is too small
 * q3tts_op_pitch is the test surface of the pitch kernel: q3tts_op_tsm plus pitch_pct[G] and a second whole, guarded state store.  G streams
 * run through n_chunks launches of the engine's launcher, one per chunk, and one more (no input, flush) when `flush` is nonzero, on a fresh
 * shifter.  A stream with pitch 100 and a rate goes through the stretcher's launcher beside it, as in a decode pass; one with neither is
 * copied through as native f32.
 *   in, chunk_samples, streams, rate_pct, encoding, reset_before, out, delta_trace, hist_store   as q3tts_op_tsm's
 *   pitch_pct     [G]
 *   n_out[g]      the delivered samples of stream g
 *   zhist_store   in/out, WHOLE: Q3TTS_GLUE_GUARD floats, [n_streams][64], Q3TTS_GLUE_GUARD floats
 * Everything is checked before anything is launched; a refused call leaves every buffer unwritten. */
int64_t q3tts_pitch_samples(int32_t rate_pct, int32_t pitch_pct, int64_t n_native, int32_t final);
int q3tts_pitch_plan(int32_t pitch_pct, int32_t* L, int32_t* M, int32_t* n_taps, int32_t* taps_per_output);
int64_t q3tts_pitch_filter(int32_t pitch_pct, float* h32, int64_t cap);
int q3tts_op_pitch(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                   const int32_t* rate_pct, const int32_t* pitch_pct, const int32_t* encoding, const int32_t* reset_before, int32_t flush,
                   void* const* out, const int64_t* out_bytes, int64_t* n_out, int32_t* const* delta_trace, const int64_t* trace_len,
                   float* hist_store, float* zhist_store);

/* [EXT] volume (q3tts_spec.h "volume"): the gain and limiter stage on the device, behind the output conv.
 * Host only, no device needed:
 *   q3tts_volume_gain    G = (float) pow(10.0, db10 / 200.0) of a volume in tenths of a dB; NaN for one outside [Q3_VOL_MIN, Q3_VOL_MAX]
 * q3tts_op_volume is the test surface of the volume kernel.  G streams run through n_chunks launches of the engine's launcher, one per chunk,
 * on a fresh stage; each launch rewrites a copy of the chunk in place, as a decode pass rewrites the output conv's buffer, and every
 * stream's T samples are then appended to its output.  A stream with volume 0 is not touched and comes out as it went in.
 *   in            [n_chunks] chunks one after the other, each [G][chunk_samples[c]] native f32 samples
 *   chunk_samples [n_chunks], each a positive multiple of 1920
 *   streams       [n_chunks][G] state slots in [0, n_streams); reset_before [n_chunks][G] (optional): nonzero = the slot is reset first
 *   vol_db10      [G]
 *   out[g]        in/out, WHOLE: Q3TTS_GLUE_GUARD floats, the stream's samples, Q3TTS_GLUE_GUARD floats; out_bytes[g] = its size in bytes
 *   n_out[g]      the samples of stream g (the sum of the chunks)
 *   gain_trace    optional (NULL: none).  gain_trace[g]: in/out, WHOLE, guarded like out[g]: g[n] of every sample, trace_len[g] floats in all;
 *                 a stream with volume 0 leaves its core unwritten
 *   hist_store    in/out, WHOLE: Q3TTS_GLUE_GUARD floats, [n_streams][Q3_VOL_HIST], Q3TTS_GLUE_GUARD floats
 * Everything is checked before anything is launched; a refused call leaves every buffer unwritten. */
float q3tts_volume_gain(int32_t db10);
int q3tts_op_volume(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                    const int32_t* vol_db10, const int32_t* reset_before, float* const* out, const int64_t* out_bytes, int64_t* n_out,
                    float* const* gain_trace, const int64_t* trace_len, float* hist_store);

/* [EXT] loudness (q3tts_spec.h "loudness"): the BS.1770 meter, its host half and its kernel.
 * Host only, no device needed:
 *   q3tts_loudness_tables     coef[10] = the shelf stage's b0 b1 b2 a1 a2, then the high-pass stage's (b = 1, -2, 1), at 24000 Hz; m[16] = A^96,
 *                             row-major: column i is the filter state after 96 zero-input steps from the unit state e_i
 *   q3tts_loudness_gate       the gate over rows [n][2] = {energy, peak} of n 100 ms blocks: gated integrated loudness, the largest momentary
 *                             (400 ms) loudness and the sample peak in dBFS, -INFINITY where no block qualifies; n_blocks = n, n_gated = the
 *                             400 ms blocks past both gates.  < 0: a null argument or n < 0
 *   q3tts_loudness_gain_db10  the volume, in tenths of a dB, that takes measured_lufs to target_lufs: rounded to nearest, clamped to
 *                             [Q3_VOL_MIN, Q3_VOL_MAX]; 0 for a non-finite input
 * q3tts_op_loudness is the test surface of the loudness kernel.  G streams run through n_chunks launches of the engine's launcher, one per
 * chunk, on a fresh stage; the call keeps each slot's position as the engine keeps a request's: it grows by the chunk and a reset sets it
 * to 0.  A stream that is not metered is neither read nor written.
 *   in            [n_chunks] chunks one after the other, each [G][chunk_samples[c]] native f32 samples
 *   chunk_samples [n_chunks], each a positive multiple of 1920
 *   streams       [n_chunks][G] state slots in [0, n_streams); reset_before [n_chunks][G] (optional): nonzero = the slot is reset first
 *   metered       [G], nonzero = the stream is metered
 *   rows[g]       in/out, WHOLE: Q3TTS_GLUE_GUARD rows, the stream's rows [n_rows[g]][2] doubles, Q3TTS_GLUE_GUARD rows; rows_bytes[g] = its
 *                 size in bytes (16 per row); an unmetered stream leaves its core unwritten
 *   n_rows[g]     the blocks stream g completed
 *   state_store   in/out, WHOLE: Q3TTS_GLUE_GUARD doubles, [n_streams][Q3_LOUD_STATE], Q3TTS_GLUE_GUARD doubles
 * Everything is checked before anything is launched; a refused call leaves every buffer unwritten. */
int q3tts_loudness_tables(double* coef /* [10] */, double* m /* [16] */);
int q3tts_loudness_gate(const double* rows, int32_t n, q3tts_loudness* out);
int32_t q3tts_loudness_gain_db10(double measured_lufs, double target_lufs);
int q3tts_op_loudness(const float* in, int32_t G, const int32_t* chunk_samples, int32_t n_chunks, const int32_t* streams, int32_t n_streams,
                      const int32_t* metered, const int32_t* reset_before, double* const* rows, const int64_t* rows_bytes, int64_t* n_rows,
                      double* state_store);

/* [EXT] reference audio intake (q3tts_spec.h "reference audio intake"): reference audio in the caller's rate, sample format and channel
 * count, decoded, downmixed and resampled to the encoders' mono f32 at 24000 Hz on the device.  Host only (no device needed):
 *   q3tts_intake_plan      24000 / rate = L / M, the prototype's tap count N and the most taps one output sample sums (24000: 1, 1, 0, 0);
 *                          < 0 for a rate the intake does not take.  Any output pointer may be NULL
 *   q3tts_intake_filter    the f32 prototype h32[0..N) into h32[cap]; returns N, < 0 for such a rate or cap < N
 *   q3tts_intake_samples   ceil(n_frames L / M); < 0 for such a rate or n_frames < 0
 *   q3tts_intake_tile      output samples one block of the kernel computes at this rate (a multiple of 4 in [64, 1024]); < 0 for such a rate
 *   q3tts_intake_check     0 if the clip may run, else < 0 and q3tts_last_error says why: the rate, channels outside [1, 8], the sample
 *                          format, the downmix, n_frames < 1, more than 120 s of output, NULL data
 *   q3tts_wav_probe        reads a RIFF/WAVE header from bytes[0..n): PCM (tag 1) at 8, 16, 24, 32 bits, IEEE float (tag 3) at 32 bits, and
 *                          WAVE_FORMAT_EXTENSIBLE of either; chunks in any order with fmt before data, odd chunks padded; a data chunk
 *                          longer than the file is cut to the file.  Anything else is < 0 with a reason; no byte at or past n is read
 * q3tts_intake: n_clips in [1, 64] clips in one launch.  out[i] receives exactly n_out[i] = q3tts_intake_samples(rate_i, n_frames_i) floats
 * and must hold out_cap[i] >= that many.  Everything is checked before anything is launched, and a refused or failed call writes neither
 * out nor n_out; a clip with a non-finite sample fails the call, and the error names the clip.  Safe beside running engines.
 * q3tts_wav_intake: a WAV file through q3tts_wav_probe and q3tts_intake; info (optional) receives the header.  cap < the sample count is
 * refused; with out == NULL and cap == 0 only *n_out and *info are written (a size query, no device needed). */
int q3tts_intake_plan(int32_t rate, int32_t* L, int32_t* M, int32_t* n_taps, int32_t* taps_per_output);
int64_t q3tts_intake_filter(int32_t rate, float* h32, int64_t cap);
int64_t q3tts_intake_samples(int32_t rate, int64_t n_frames);
int32_t q3tts_intake_tile(int32_t rate);
int q3tts_intake_check(const q3tts_intake_clip* c);
int q3tts_wav_probe(const void* bytes, int64_t n, q3tts_wav_info* out);
int q3tts_intake(int32_t device, const q3tts_intake_clip* clips, int32_t n_clips, float* const* out, const int64_t* out_cap, int64_t* n_out);
int q3tts_wav_intake(const char* path, int32_t downmix, int32_t device, float* out, int64_t cap, int64_t* n_out, q3tts_wav_info* info);

#ifdef __cplusplus
}
#endif
#endif
