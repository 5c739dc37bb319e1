// capi.cpp -- extern "C" Boundary B (include/q3tts.h).  Every entry point catches, records last_error, returns a code.
#include "../../include/q3tts.h"
#include "engine.h"
#include "tfctx.h"
#include <algorithm>

using namespace q3;

struct q3tts_assets { std::unique_ptr<HostAssets> owned; const HostAssets* a = nullptr; };
struct q3tts_engine { std::unique_ptr<Engine> e; q3tts_assets assets_view; }; // the view lives exactly as long as the engine
struct q3tts_sampler { Sampler s; };
struct q3tts_chunker { std::unique_ptr<Chunker> c; };
struct q3tts_decoder { std::unique_ptr<CodecDecoder> d; hipStream_t st = nullptr; float* pinned = nullptr; size_t pinned_cap = 0; };
struct q3tts_tf { std::unique_ptr<TfContext> c; };

#define Q3_API_BEGIN try {
#define Q3_API_END(failval) } catch (const std::exception& ex) { set_last_error(ex.what()); return failval; } catch (...) { set_last_error("unknown error"); return failval; }

static void require_gpu() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) throw Error("no HIP device available: the HIP path is the only compute path (no CPU fallback)");
}

extern "C" {

const char* q3tts_last_error(void) { return last_error(); }
int q3tts_version(void) { return 100; }
int q3tts_device_count(void) { int n = 0; if (hipGetDeviceCount(&n) != hipSuccess) return 0; return n; }

void q3tts_sampler_config_default(q3tts_sampler_config* c) { c->temperature = 0.7f; c->top_k = 40; c->top_p = 0.9f; c->has_seed = 0; c->seed = 0; }
void q3tts_gen_options_default(q3tts_gen_options* o) { o->repetition_penalty = 1.0f; o->predictor_temperature = 0.0f; o->predictor_top_k = 0; o->predictor_top_p = 1.0f; }
void q3tts_engine_params_default(q3tts_engine_params* p) {
    p->model_dir = nullptr; p->quant = "q8_0"; p->device = 0; p->max_batch = 1; p->max_prompt = 1024;
    p->max_steps = Q3_DEFAULT_MAX_STEPS; p->load_codec = 1; p->use_graph = 1;
}

int q3tts_engine_create(const q3tts_engine_params* p, q3tts_engine** out) {
    Q3_API_BEGIN
    Q3_CHECK(p && out && p->model_dir, "null argument");
    require_gpu();
    Q3_HIP(hipSetDevice(p->device));
    EngineParams ep;
    ep.model_dir = p->model_dir; ep.quant = p->quant ? p->quant : "q8_0"; ep.max_batch = p->max_batch; ep.max_prompt = p->max_prompt;
    ep.max_steps = p->max_steps; ep.load_codec = p->load_codec != 0; ep.use_graph = p->use_graph != 0;
    auto* h = new q3tts_engine();
    try { h->e.reset(new Engine(ep)); } catch (...) { delete h; throw; }
    h->assets_view.a = &h->e->assets();
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_engine_destroy(q3tts_engine* e) { delete e; }
int32_t q3tts_engine_device(q3tts_engine* e) { return e ? e->e->device() : -1; }
int32_t q3tts_engine_prefill_width(q3tts_engine* e) { return e ? e->e->talker().max_tok() : -1; }

static GenRequest to_gen(const q3tts_request& q);
static GenOptions to_opts(const q3tts_gen_options* o) {
    GenOptions g;
    if (o) { g.repetition_penalty = o->repetition_penalty; g.predictor_temperature = o->predictor_temperature; g.predictor_top_k = o->predictor_top_k; g.predictor_top_p = o->predictor_top_p; }
    return g;
}
int q3tts_generate_batch(q3tts_engine* e, q3tts_request* reqs, int32_t n, int32_t want_pcm) { return q3tts_generate_batch_ex(e, reqs, n, want_pcm, nullptr); }
int q3tts_generate_batch_ex(q3tts_engine* e, q3tts_request* reqs, int32_t n, int32_t want_pcm, const q3tts_gen_options* opts) {
    return q3tts_generate_batch_trailing(e, reqs, n, want_pcm, opts, nullptr, nullptr);
}
int q3tts_generate_batch_trailing(q3tts_engine* e, q3tts_request* reqs, int32_t n, int32_t want_pcm, const q3tts_gen_options* opts,
                                  const int32_t* const* trail_ids, const int32_t* n_trail) {
    Q3_API_BEGIN
    Q3_CHECK(e && reqs && n >= 1, "bad arguments");
    std::vector<GenRequest> rq(n);
    for (int i = 0; i < n; i++) {
        rq[i] = to_gen(reqs[i]); rq[i].opts = to_opts(opts ? &opts[i] : nullptr);
        if (n_trail) { rq[i].n_trail = n_trail[i]; rq[i].trail = trail_ids ? trail_ids[i] : nullptr; } // validated with the rest, before queueing
    }
    std::vector<GenResult> res;
    e->e->generate_batch(rq, res, want_pcm != 0);
    for (int i = 0; i < n; i++) {
        reqs[i].n_frames = res[i].n_frames;
        if (reqs[i].codes_out) std::copy(res[i].codes.begin(), res[i].codes.end(), reqs[i].codes_out);
        const int64_t np = std::min<int64_t>((int64_t)res[i].pcm.size(), reqs[i].pcm_out ? reqs[i].pcm_capacity : 0);
        if (np > 0) std::copy(res[i].pcm.begin(), res[i].pcm.begin() + np, reqs[i].pcm_out);
        reqs[i].n_pcm = np;
        reqs[i].prefill_ms = res[i].prefill_ms; reqs[i].first_chunk_ms = res[i].first_chunk_ms; reqs[i].total_ms = res[i].total_ms;
    }
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

static GenRequest to_gen(const q3tts_request& q) {
    GenRequest g;
    g.prompt = q.prompt; g.n_prompt = q.n_prompt; g.max_steps = q.max_steps; g.mask_eos = q.mask_eos != 0;
    g.sampler.temperature = q.sampler.temperature; g.sampler.top_k = q.sampler.top_k; g.sampler.top_p = q.sampler.top_p;
    g.sampler.has_seed = q.sampler.has_seed != 0; g.sampler.seed = q.sampler.seed;
    return g;
}
int q3tts_submit(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, int64_t* req_id) { return q3tts_submit_ex(e, r, want_pcm, nullptr, req_id); }
int q3tts_submit_ex(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && r && req_id, "null argument");
    GenRequest g = to_gen(*r);
    g.opts = to_opts(opts);
    *req_id = e->e->submit(g, want_pcm != 0, true);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_submit_trailing(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts, const int32_t* trail_ids,
                          int32_t n_trail, int64_t* req_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && r && req_id, "null argument");
    GenRequest g = to_gen(*r);
    g.opts = to_opts(opts);
    g.trail = trail_ids; g.n_trail = n_trail;
    *req_id = e->e->submit(g, want_pcm != 0, true);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_submit_trailing_open(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts,
                               const int32_t* trail_ids, int32_t n_trail, int64_t* req_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && r && req_id, "null argument");
    GenRequest g = to_gen(*r);
    g.opts = to_opts(opts);
    g.trail = trail_ids; g.n_trail = n_trail; g.open = true;
    *req_id = e->e->submit(g, want_pcm != 0, true);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_submit_resume(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts, const int32_t* trail_ids,
                        int32_t n_trail, int32_t open, const int32_t* prefix_codes, int32_t n_prefix, int64_t* req_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && r && req_id, "null argument");
    GenRequest g = to_gen(*r);
    g.opts = to_opts(opts);
    g.trail = trail_ids; g.n_trail = n_trail; g.open = open != 0;
    g.prefix = prefix_codes; g.n_prefix = n_prefix;
    *req_id = e->e->submit(g, want_pcm != 0, true);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_submit_score(q3tts_engine* e, const float* prompt, int32_t n_prompt, const int32_t* trail_ids, int32_t n_trail, const int32_t* codes,
                       int32_t n, int64_t* req_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && req_id, "null argument");
    *req_id = e->e->submit_score(prompt, n_prompt, trail_ids, n_trail, codes, n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int32_t q3tts_engine_score_width(q3tts_engine* e) { return e ? e->e->score_width() : -1; }
int q3tts_submit_decode(q3tts_engine* e, const int32_t* codes, int32_t n, int64_t* req_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && codes && req_id, "null argument");
    *req_id = e->e->submit_decode(codes, n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int32_t q3tts_engine_decode_width(q3tts_engine* e) { return e ? e->e->decode_width() : -1; }
int q3tts_engine_decode_stats(q3tts_engine* e, int64_t* requests, int64_t* chunks, int64_t* chunks_shared) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int64_t r = 0, c = 0, s = 0;
    e->e->decode_stats(&r, &c, &s);
    if (requests) *requests = r;
    if (chunks) *chunks = c;
    if (chunks_shared) *chunks_shared = s;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_submit_candidates(q3tts_engine* e, const q3tts_request* r, int32_t want_pcm, const q3tts_gen_options* opts, const int32_t* trail_ids,
                            int32_t n_trail, const uint64_t* seeds, int32_t n, int64_t* req_ids) {
    Q3_API_BEGIN
    Q3_CHECK(e && r, "null argument");
    GenRequest g = to_gen(*r);
    g.opts = to_opts(opts);
    g.trail = trail_ids; g.n_trail = n_trail;
    std::vector<int64_t> ids((size_t)std::max(n, 1)); // the caller's array is written only when the whole set is queued
    e->e->submit_candidates(g, want_pcm != 0, seeds, n, req_ids ? ids.data() : nullptr);
    std::copy(ids.begin(), ids.begin() + n, req_ids);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_candidate_stats(q3tts_engine* e, int64_t* sets, int64_t* prefill_rows_saved, int64_t* pages_copied) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int64_t s = 0, r = 0, p = 0;
    e->e->candidate_stats(&s, &r, &p);
    if (sets) *sets = s;
    if (prefill_rows_saved) *prefill_rows_saved = r;
    if (pages_copied) *pages_copied = p;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_trail_append(q3tts_engine* e, int64_t req_id, const int32_t* ids, int32_t n, int32_t close) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    return e->e->append_trail(req_id, ids, n, close != 0);
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_trail_progress(q3tts_engine* e, int64_t req_id, int32_t* n_appended, int32_t* n_consumed, int32_t* closed) {
    Q3_API_BEGIN
    Q3_CHECK(e && n_appended && n_consumed && closed, "null argument");
    int na = 0, nc = 0; bool cl = false;
    e->e->trail_progress(req_id, &na, &nc, &cl);
    *n_appended = na; *n_consumed = nc; *closed = cl ? 1 : 0;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_text_append(q3tts_engine* e, int64_t req_id, const int32_t* text_ids, int32_t n, int32_t is_last) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    Q3_CHECK(n >= 0 && (n == 0 || text_ids), "bad arguments");
    std::vector<int32_t> ids(text_ids, text_ids + n);
    if (is_last) ids.push_back(Q3_TEXT_EOS); // the streaming layout's trail ends with TEXT_EOS (q3tts_spec.h)
    return e->e->append_trail(req_id, ids.data(), (int)ids.size(), is_last != 0);
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_poll(q3tts_engine* e, int64_t id, q3tts_req_status* o) {
    Q3_API_BEGIN
    Q3_CHECK(e && o, "null argument");
    const ReqStatus s = e->e->poll(id);
    o->state = s.state; o->n_frames = s.n_frames; o->n_pcm = s.n_pcm; o->queue_ms = s.queue_ms; o->prefill_ms = s.prefill_ms;
    o->first_chunk_ms = s.first_chunk_ms; o->total_ms = s.total_ms;
    if (s.state == REQ_FAILED) set_last_error(s.error.empty() ? "request failed" : s.error); // state says it failed; q3tts_last_error() says why
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_fetch(q3tts_engine* e, int64_t id, int32_t* codes, int32_t frame_off, int32_t max_frames, float* pcm, int64_t pcm_off,
                int64_t pcm_cap, int32_t* got_frames, int64_t* got_pcm) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int gf = 0; int64_t gp = 0;
    e->e->fetch(id, codes, frame_off, max_frames, pcm, pcm_off, pcm_cap, &gf, &gp);
    if (got_frames) *got_frames = gf;
    if (got_pcm) *got_pcm = gp;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_wait(q3tts_engine* e, int64_t id, double timeout_ms) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    return e->e->wait(id, timeout_ms) ? 0 : 1;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_release(q3tts_engine* e, int64_t id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->release(id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_cancel(q3tts_engine* e, int64_t id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); return e->e->cancel(id); Q3_API_END(Q3TTS_ERR) }
int q3tts_engine_set_logprobs(q3tts_engine* e, int32_t on) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_logprobs(on != 0); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_fetch_logprobs(q3tts_engine* e, int64_t id, float* out, int32_t frame_off, int32_t max_frames, int32_t* got_frames) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int gf = 0;
    e->e->fetch_logprobs(id, out, frame_off, max_frames, &gf);
    if (got_frames) *got_frames = gf;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] output formats */
int q3tts_engine_set_output_format(q3tts_engine* e, const q3tts_pcm_format* f) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_output_format(f); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_format(q3tts_engine* e, int64_t id, q3tts_pcm_format* out) {
    Q3_API_BEGIN
    Q3_CHECK(e && out, "null argument");
    *out = e->e->request_format(id);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_fetch_pcm16(q3tts_engine* e, int64_t id, int16_t* out, int64_t off, int64_t cap, int64_t* got) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int64_t n = 0;
    e->e->fetch_pcm16(id, out, off, cap, &n);
    if (got) *got = n;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_pcm_out_stats(q3tts_engine* e, int64_t* chunks_converted, int64_t* samples_out) {
    Q3_API_BEGIN
    Q3_CHECK(e && chunks_converted && samples_out, "null argument");
    const OutputStageStats s = e->e->output_stats();
    *chunks_converted = s.conv_chunks; *samples_out = s.conv_samples;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] codec preambles */
int q3tts_preamble_create(q3tts_engine* e, const int32_t* codes, int32_t n, int32_t* preamble_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && preamble_id, "null argument");
    *preamble_id = e->e->preamble_create(codes, n);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_preamble_poll(q3tts_engine* e, int32_t preamble_id, int32_t* state, int32_t* n_frames) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int st = 0, n = 0;
    e->e->preamble_poll(preamble_id, &st, &n);
    if (state) *state = st;
    if (n_frames) *n_frames = n;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_preamble_wait(q3tts_engine* e, int32_t preamble_id, double timeout_ms) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    return e->e->preamble_wait(preamble_id, timeout_ms) ? 0 : 1;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_preamble_release(q3tts_engine* e, int32_t preamble_id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->preamble_release(preamble_id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_voice_set_preamble(q3tts_engine* e, int32_t voice_id, int32_t preamble_id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_voice_preamble(voice_id, preamble_id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_engine_set_preamble(q3tts_engine* e, int32_t preamble_id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_preamble(preamble_id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_preamble(q3tts_engine* e, int64_t req_id, int32_t* preamble_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && preamble_id, "null argument");
    *preamble_id = e->e->request_preamble(req_id);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_preamble_stats(q3tts_engine* e, int64_t* built, int64_t* restores, int64_t* bytes_per_snapshot) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int64_t b = 0, r = 0, n = 0;
    e->e->preamble_stats(&b, &r, &n);
    if (built) *built = b;
    if (restores) *restores = r;
    if (bytes_per_snapshot) *bytes_per_snapshot = n;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] prompt stems */
int q3tts_stem_create(q3tts_engine* e, const float* rows, int32_t n_rows, int32_t* stem_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && stem_id, "null argument");
    *stem_id = e->e->stem_create(rows, n_rows);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
// The rows the text forms build in front of the task text for this voice, language and instruction: the builder's output for an empty text is
// head ++ [text EOS row] ++ [codec BOS row], and its last two rows are cut.  The head ends with the text BOS row, which both layouts share.
int q3tts_voice_stem_create(q3tts_engine* e, int32_t voice_id, int32_t lang_id, const int32_t* instr_ids, int32_t n_instr, int32_t* stem_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && stem_id, "null argument");
    Q3_CHECK(n_instr >= 0 && (n_instr == 0 || instr_ids), "bad arguments");
    const Voice& v = e->e->voice(voice_id);
    std::vector<int32_t> none, ins;
    if (instr_ids) ins.assign(instr_ids, instr_ids + n_instr);
    int lang = lang_id;
    const PromptData pd = !v.ref_codes.empty()
        ? PromptBuilder::build_clone_prompt(e->e->assets(), none, v.ref_codes, v.ref_text_ids, v.spk_emb.data(), lang_id, instr_ids ? &ins : nullptr, nullptr)
        : PromptBuilder::build_core(e->e->assets(), none, lang_id >= 0 ? &lang : nullptr, nullptr, v.spk_emb.data(), instr_ids ? &ins : nullptr, nullptr, nullptr);
    *stem_id = e->e->stem_create(pd.embd.data(), pd.n_rows - 2);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_stem_poll(q3tts_engine* e, int32_t stem_id, int32_t* state, int32_t* n_rows) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    int st = 0, n = 0;
    e->e->stem_poll(stem_id, &st, &n);
    if (state) *state = st;
    if (n_rows) *n_rows = n;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_stem_wait(q3tts_engine* e, int32_t stem_id, double timeout_ms) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    return e->e->stem_wait(stem_id, timeout_ms) ? 0 : 1;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_stem_release(q3tts_engine* e, int32_t stem_id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->stem_release(stem_id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_voice_set_stem(q3tts_engine* e, int32_t voice_id, int32_t stem_id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_voice_stem(voice_id, stem_id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_engine_set_stem(q3tts_engine* e, int32_t stem_id) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_stem(stem_id); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_stem(q3tts_engine* e, int64_t req_id, int32_t* stem_id, int32_t* rows_reused) {
    Q3_API_BEGIN
    Q3_CHECK(e && stem_id && rows_reused, "null argument");
    int sid = -1, n = 0;
    e->e->request_stem(req_id, &sid, &n);
    *stem_id = sid; *rows_reused = n;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_stem_stats(q3tts_engine* e, q3tts_stem_stats* out) {
    Q3_API_BEGIN
    Q3_CHECK(e && out, "null argument");
    const Engine::StemStats s = e->e->stem_stats();
    out->built = s.built; out->restores = s.restores; out->rows_not_prefilled = s.rows_skipped; out->pages_copied = s.pages_copied;
    out->mismatches = s.mismatches; out->device_bytes = s.bytes_held;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] speaking rate */
int q3tts_engine_set_speech_rate(q3tts_engine* e, int32_t rate_pct) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_speech_rate(rate_pct); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_speech_rate(q3tts_engine* e, int64_t id, int32_t* rate_pct) {
    Q3_API_BEGIN
    Q3_CHECK(e && rate_pct, "null argument");
    *rate_pct = e->e->request_speech_rate(id);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_tsm_stats(q3tts_engine* e, int64_t* chunks, int64_t* frames_out, int64_t* flushes) {
    Q3_API_BEGIN
    Q3_CHECK(e && chunks && frames_out && flushes, "null argument");
    const OutputStageStats s = e->e->output_stats();
    *chunks = s.tsm_chunks; *frames_out = s.tsm_frames; *flushes = s.tsm_flushes;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] pitch */
int q3tts_engine_set_pitch(q3tts_engine* e, int32_t pitch_pct) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_pitch(pitch_pct); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_pitch(q3tts_engine* e, int64_t id, int32_t* pitch_pct) {
    Q3_API_BEGIN
    Q3_CHECK(e && pitch_pct, "null argument");
    *pitch_pct = e->e->request_pitch(id);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_pitch_stats(q3tts_engine* e, int64_t* chunks, int64_t* samples_out, int64_t* flushes, int64_t* table_bytes) {
    Q3_API_BEGIN
    Q3_CHECK(e && chunks && samples_out && flushes && table_bytes, "null argument");
    const OutputStageStats s = e->e->output_stats();
    *chunks = s.pitch_chunks; *samples_out = s.pitch_samples; *flushes = s.pitch_flushes; *table_bytes = s.pitch_table_bytes;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] volume */
int q3tts_engine_set_volume(q3tts_engine* e, int32_t db10) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_volume(db10); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_volume(q3tts_engine* e, int64_t id, int32_t* db10) {
    Q3_API_BEGIN
    Q3_CHECK(e && db10, "null argument");
    *db10 = e->e->request_volume(id);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_volume_stats(q3tts_engine* e, int64_t* chunks, int64_t* samples) {
    Q3_API_BEGIN
    Q3_CHECK(e && chunks && samples, "null argument");
    const OutputStageStats s = e->e->output_stats();
    *chunks = s.vol_chunks; *samples = s.vol_samples;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
/* [EXT] loudness */
int q3tts_engine_set_loudness(q3tts_engine* e, int32_t on) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->set_loudness(on != 0); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_request_metered(q3tts_engine* e, int64_t id, int32_t* on) {
    Q3_API_BEGIN
    Q3_CHECK(e && on, "null argument");
    *on = e->e->request_metered(id) ? 1 : 0;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_fetch_loudness(q3tts_engine* e, int64_t id, double* out, int64_t block_off, int64_t max_blocks, int64_t* got) {
    Q3_API_BEGIN
    Q3_CHECK(e && out && got, "null argument");
    int64_t n = 0;
    e->e->fetch_loudness(id, out, block_off, max_blocks, &n);
    *got = n;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_request_loudness(q3tts_engine* e, int64_t id, q3tts_loudness* out) {
    Q3_API_BEGIN
    Q3_CHECK(e && out, "null argument");
    std::vector<double> rows;
    int64_t n = 0;
    for (;;) {   // the rows so far: fetched in pieces, since they may grow between two calls
        const size_t at = rows.size();
        rows.resize(at + 2 * 256);
        e->e->fetch_loudness(id, rows.data() + at, (int64_t)(at / 2), 256, &n);
        rows.resize(at + 2 * (size_t)n);
        if (n < 256) break;
    }
    LoudResult r;
    loud_gate(rows.data(), (int32_t)(rows.size() / 2), &r);
    out->integrated_lufs = r.integrated_lufs; out->momentary_max_lufs = r.momentary_max_lufs; out->peak_dbfs = r.peak_dbfs;
    out->n_blocks = r.n_blocks; out->n_gated = r.n_gated;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_engine_loudness_stats(q3tts_engine* e, int64_t* chunks, int64_t* blocks) {
    Q3_API_BEGIN
    Q3_CHECK(e && chunks && blocks, "null argument");
    const OutputStageStats s = e->e->output_stats();
    *chunks = s.loud_chunks; *blocks = s.loud_blocks;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_sched_start(q3tts_engine* e) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->start_driver(); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_sched_stop(q3tts_engine* e) { Q3_API_BEGIN Q3_CHECK(e, "null argument"); e->e->stop_driver(); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_sched_step(q3tts_engine* e, int32_t* busy) {
    Q3_API_BEGIN
    Q3_CHECK(e, "null argument");
    const bool b = e->e->step();
    if (busy) *busy = b ? 1 : 0;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_voice_register(q3tts_engine* e, const float* spk, const int32_t* ref_codes, int32_t n_ref_codes, const int32_t* ref_text,
                         int32_t n_ref_text, int32_t* voice_id) {
    Q3_API_BEGIN
    Q3_CHECK(e && spk && voice_id, "null argument");
    Voice v;
    v.spk_emb.assign(spk, spk + 2048);
    if (ref_codes && n_ref_codes > 0) v.ref_codes.assign(ref_codes, ref_codes + n_ref_codes);
    if (ref_text && n_ref_text > 0) v.ref_text_ids.assign(ref_text, ref_text + n_ref_text);
    *voice_id = e->e->register_voice(v);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_submit_text(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id, const int32_t* instr_ids,
                      int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps, int32_t mask_eos, int32_t want_pcm,
                      int64_t* req_id) {
    return q3tts_submit_text_ex(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, nullptr, req_id);
}
static int submit_text(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id, const int32_t* instr_ids,
                       int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps, int32_t mask_eos, int32_t want_pcm,
                       const q3tts_gen_options* opts, bool streaming, int64_t* req_id, bool open = false);
int q3tts_submit_text_ex(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id, const int32_t* instr_ids,
                         int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps, int32_t mask_eos, int32_t want_pcm,
                         const q3tts_gen_options* opts, int64_t* req_id) {
    return submit_text(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, opts, false, req_id);
}
int q3tts_submit_text_streaming(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                                int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id) {
    return submit_text(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, opts, true, req_id);
}
int q3tts_submit_text_streaming_open(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id,
                                     const int32_t* instr_ids, int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps,
                                     int32_t mask_eos, int32_t want_pcm, const q3tts_gen_options* opts, int64_t* req_id) {
    return submit_text(e, voice_id, text_ids, n_text, lang_id, instr_ids, n_instr, sampler, max_steps, mask_eos, want_pcm, opts, true, req_id,
                       true);
}
static int submit_text(q3tts_engine* e, int32_t voice_id, const int32_t* text_ids, int32_t n_text, int32_t lang_id, const int32_t* instr_ids,
                       int32_t n_instr, const q3tts_sampler_config* sampler, int32_t max_steps, int32_t mask_eos, int32_t want_pcm,
                       const q3tts_gen_options* opts, bool streaming, int64_t* req_id, bool open) {
    Q3_API_BEGIN
    Q3_CHECK(e && text_ids && n_text >= 0 && req_id, "bad arguments");
    Q3_CHECK(!streaming || n_text >= 1, "the streaming-text layout needs n_text >= 1");
    const Voice& v = e->e->voice(voice_id);
    std::vector<int32_t> t(text_ids, text_ids + n_text), ins;
    if (instr_ids) ins.assign(instr_ids, instr_ids + n_instr);
    int lang = lang_id;
    // engine.rs:398-428: clone voices (codes + ref text) take build_clone_prompt, presets build_core with marker + spk_emb
    std::vector<int32_t> trail;
    std::vector<int32_t>* tr = streaming ? &trail : nullptr;
    PromptData pd = !v.ref_codes.empty()
        ? PromptBuilder::build_clone_prompt(e->e->assets(), t, v.ref_codes, v.ref_text_ids, v.spk_emb.data(), lang_id, instr_ids ? &ins : nullptr, tr)
        : PromptBuilder::build_core(e->e->assets(), t, lang_id >= 0 ? &lang : nullptr, nullptr, v.spk_emb.data(), instr_ids ? &ins : nullptr, nullptr, tr);
    GenRequest g;
    g.prompt = pd.embd.data(); g.n_prompt = pd.n_rows; g.max_steps = max_steps; g.mask_eos = mask_eos != 0;
    if (sampler) {
        g.sampler.temperature = sampler->temperature; g.sampler.top_k = sampler->top_k; g.sampler.top_p = sampler->top_p;
        g.sampler.has_seed = sampler->has_seed != 0; g.sampler.seed = sampler->seed;
    }
    g.opts = to_opts(opts);
    if (open) trail.pop_back(); // the TEXT_EOS that ends the trail comes with q3tts_text_append(is_last = 1)
    g.trail = trail.data(); g.n_trail = (int)trail.size(); g.open = open;
    g.preamble = e->e->voice_preamble(voice_id); // [EXT] codec preambles: a text form takes its voice's, never the engine-level setting
    g.stem = e->e->voice_stem(voice_id);         // [EXT] prompt stems: likewise
    *req_id = e->e->submit(g, want_pcm != 0, true);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

int q3tts_engine_stats(q3tts_engine* e, q3tts_stats* o) {
    Q3_API_BEGIN
    const EngineStats& s = e->e->read_stats();
    o->frame_loop_ms = s.frame_loop_ms; o->frames = s.frames; o->prefill_ms = s.prefill_ms; o->gemv_ms = s.gemv_ms;
    o->gemv_launches = s.gemv_launches; o->gemv_bytes = s.gemv_bytes; o->codec_ms = s.codec_ms; o->codec_calls = s.codec_calls;
    o->gu_ms = s.gu_ms; o->gu_launches = s.gu_launches; o->gu_bytes = s.gu_bytes;
    o->sched_steps = s.steps; o->slot_frames = s.slot_frames; o->graph_frames = s.graph_frames;
    o->talker_weight_bytes = (double)e->e->talker().weight_bytes(); o->predictor_weight_bytes = (double)e->e->predictor().weight_bytes();
    const auto& hp = e->e->talker().hp();
    o->kv_bytes_per_token = (double)hp.n_layer * 2 * hp.n_kv * 128 * 2;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_engine_reset_stats(q3tts_engine* e) { if (e) e->e->reset_stats(); }
void q3tts_engine_set_instrument(q3tts_engine* e, int32_t on) { if (e) e->e->set_instrument(on != 0); }
double q3tts_engine_bytes_per_step(q3tts_engine* e, int32_t batch, double mean_ctx) { return e ? (double)e->e->bytes_per_frame_step(batch, mean_ctx) : 0.0; }
int64_t q3tts_pred_table_bytes(q3tts_engine* e) { return e ? (int64_t)e->e->pred_table_bytes() : 0; }

// ---------------- assets / prompt ----------------
int q3tts_assets_open(const char* path, q3tts_assets** out) {
    Q3_API_BEGIN
    Q3_CHECK(path && out, "null argument");
    auto* h = new q3tts_assets();
    try { h->owned.reset(new HostAssets(path)); } catch (...) { delete h; throw; }
    h->a = h->owned.get();
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_assets_close(q3tts_assets* a) { delete a; }
const q3tts_assets* q3tts_engine_assets(q3tts_engine* e) { return e ? &e->assets_view : nullptr; }
int q3tts_assets_codec_embedding(const q3tts_assets* a, int32_t q, int32_t code, float* out) { Q3_API_BEGIN a->a->codec_embedding(q, code, out); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_assets_text_embedding(const q3tts_assets* a, int64_t tok, float* out) { Q3_API_BEGIN a->a->text_embedding(tok, out); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_assets_tts_pad(const q3tts_assets* a, float* out) { Q3_API_BEGIN std::copy(a->a->tts_pad(), a->a->tts_pad() + 2048, out); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }

// [EXT] resume: k_feedback_codes against an assets file's tables, host buffers in and out
int q3tts_op_feedback_rows(const q3tts_assets* a, const int32_t* codes, int32_t n, const int32_t* trail_ids, int32_t n_trail, float* rows) {
    Q3_API_BEGIN
    Q3_CHECK(a && a->a && codes && rows && n >= 1, "bad arguments");
    Q3_CHECK(n_trail >= 0 && (n_trail == 0 || trail_ids), "trailing ids missing");
    require_gpu();
    const HostAssets& h = *a->a;
    Q3_CHECK(h.n_codec == 16, "need 16 codec embedding tables");
    std::vector<DevBuf<float>> tab(16);
    std::vector<const float*> ptrs(16); std::vector<int64_t> nrows(16);
    for (int q = 0; q < 16; q++) {
        const size_t sz = (size_t)h.codec_rows[q] * Q3_EMBD;
        tab[q].alloc(sz); tab[q].upload(h.codec[q], sz);
        ptrs[q] = tab[q].p; nrows[q] = h.codec_rows[q];
    }
    DevBuf<const float*> d_ptrs(16); DevBuf<int64_t> d_nrows(16); DevBuf<float> d_pad(Q3_EMBD), d_text, d_rows((size_t)(n + 2) * Q3_EMBD);
    DevBuf<int32_t> d_codes((size_t)n * 16), d_ids;
    d_ptrs.upload(ptrs.data(), 16); d_nrows.upload(nrows.data(), 16); d_pad.upload(h.tts_pad(), Q3_EMBD); d_codes.upload(codes, (size_t)n * 16);
    FeedbackIds fi;
    const int nt = std::min(n_trail, n);
    if (nt > 0) {
        const int64_t tr = h.text_table ? h.text_rows : 0;
        d_text.alloc((size_t)std::max<int64_t>(tr, 1) * Q3_EMBD);
        if (tr > 0) d_text.upload(h.text_table, (size_t)tr * Q3_EMBD);
        d_ids.alloc(nt); d_ids.upload(trail_ids, nt);
        fi.ids = d_ids.p; fi.n_ids = nt; fi.table = d_text.p; fi.rows = tr;
    }
    // one guard row on either side of the device rows: a write outside [0, n) rows is an error here, not silent damage
    std::vector<float> all((size_t)(n + 2) * Q3_EMBD, -12345.0f);
    d_rows.upload(all.data(), all.size());
    launch_feedback_codes(0, d_ptrs.p, d_nrows.p, d_codes.p, d_pad.p, d_rows.p + Q3_EMBD, n, &fi);
    Q3_HIP(hipDeviceSynchronize());
    d_rows.download(all.data(), all.size());
    for (int i = 0; i < Q3_EMBD; i++)
        Q3_CHECK(all[i] == -12345.0f && all[(size_t)(n + 1) * Q3_EMBD + i] == -12345.0f, "k_feedback_codes wrote outside its rows");
    std::copy(all.begin() + Q3_EMBD, all.begin() + (size_t)(n + 1) * Q3_EMBD, rows);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

// host-side projection with the reference's exact loop (assets_manager.rs:383-399); used by the Boundary-A replay harness
extern "C" int q3tts_assets_proj_out(const q3tts_assets* a) { return (int)a->a->proj_out; }
extern "C" int q3tts_assets_project_host(const q3tts_assets* a, const float* x, float* out) {
    const HostAssets& h = *a->a;
    for (int64_t o = 0; o < h.proj_out; o++) {
        float sum = h.proj_b[o];
        const float* w = h.proj_w + (size_t)o * (size_t)h.proj_in;
        for (int64_t i = 0; i < h.proj_in; i++) { const float t = x[i] * w[i]; sum = sum + t; }
        out[o] = sum;
    }
    return Q3TTS_OK;
}
static int emit_rows(const PromptData& d, float* out, int32_t max_rows) {
    if (d.n_rows > max_rows) { set_last_error("prompt does not fit max_rows"); return -1; }
    std::copy(d.embd.begin(), d.embd.end(), out);
    return d.n_rows;
}
int q3tts_prompt_build_core(const q3tts_assets* a, const int32_t* text_ids, int32_t n_text, int32_t lang_id, int32_t spk_id,
                            const float* spk_emb, const int32_t* instr_ids, int32_t n_instr, const float* mid_rows, int32_t n_mid,
                            float* out, int32_t max_rows) {
    Q3_API_BEGIN
    std::vector<int32_t> t(text_ids, text_ids + n_text), ins;
    if (instr_ids) ins.assign(instr_ids, instr_ids + n_instr);
    std::vector<float> mid;
    if (mid_rows) mid.assign(mid_rows, mid_rows + (size_t)n_mid * 2048);
    int lang = lang_id, spk = spk_id;
    return emit_rows(PromptBuilder::build_core(*a->a, t, lang_id >= 0 ? &lang : nullptr, spk_id >= 0 ? &spk : nullptr, spk_emb,
                                               instr_ids ? &ins : nullptr, mid_rows ? &mid : nullptr), out, max_rows);
    Q3_API_END(-1)
}
int q3tts_prompt_build_clone(const q3tts_assets* a, const int32_t* text_ids, int32_t n_text, const int32_t* ref_codes, int32_t n_ref_codes,
                             const int32_t* ref_text_ids, int32_t n_ref_text, const float* spk_emb, int32_t lang_id,
                             const int32_t* instr_ids, int32_t n_instr, float* out, int32_t max_rows) {
    Q3_API_BEGIN
    std::vector<int32_t> t(text_ids, text_ids + n_text), rc(ref_codes, ref_codes + n_ref_codes), rt(ref_text_ids, ref_text_ids + n_ref_text), ins;
    if (instr_ids) ins.assign(instr_ids, instr_ids + n_instr);
    return emit_rows(PromptBuilder::build_clone_prompt(*a->a, t, rc, rt, spk_emb, lang_id, instr_ids ? &ins : nullptr), out, max_rows);
    Q3_API_END(-1)
}
int q3tts_prompt_build_streaming(const q3tts_assets* a, const int32_t* text_ids, int32_t n_text, int32_t lang_id, int32_t spk_id,
                                 const float* spk_emb, const int32_t* instr_ids, int32_t n_instr, const int32_t* ref_codes,
                                 int32_t n_ref_codes, const int32_t* ref_text_ids, int32_t n_ref_text, float* out, int32_t max_rows,
                                 int32_t* trail_ids, int32_t trail_cap, int32_t* n_trail) {
    Q3_API_BEGIN
    Q3_CHECK(a && text_ids && n_text >= 1 && trail_ids && n_trail, "bad arguments (the streaming-text layout needs n_text >= 1)");
    Q3_CHECK(trail_cap >= n_text, "trail_cap < n_text");
    std::vector<int32_t> t(text_ids, text_ids + n_text), ins, trail;
    if (instr_ids) ins.assign(instr_ids, instr_ids + n_instr);
    PromptData d;
    if (ref_codes && n_ref_codes > 0) {
        Q3_CHECK(spk_emb && lang_id >= 0, "a clone prompt needs spk_emb and lang_id");
        std::vector<int32_t> rc(ref_codes, ref_codes + n_ref_codes), rt;
        if (ref_text_ids) rt.assign(ref_text_ids, ref_text_ids + n_ref_text);
        d = PromptBuilder::build_clone_prompt(*a->a, t, rc, rt, spk_emb, lang_id, instr_ids ? &ins : nullptr, &trail);
    } else {
        int lang = lang_id, spk = spk_id;
        d = PromptBuilder::build_core(*a->a, t, lang_id >= 0 ? &lang : nullptr, spk_id >= 0 ? &spk : nullptr, spk_emb, instr_ids ? &ins : nullptr,
                                      nullptr, &trail);
    }
    const int rows = emit_rows(d, out, max_rows);
    if (rows < 0) return rows;
    std::copy(trail.begin(), trail.end(), trail_ids);
    *n_trail = (int32_t)trail.size();
    return rows;
    Q3_API_END(-1)
}

// ---------------- sampler / chunker ----------------
q3tts_sampler* q3tts_sampler_new(float temperature, int32_t top_k, float top_p, uint64_t seed) { return new q3tts_sampler{Sampler(temperature, top_k, top_p, seed)}; }
void q3tts_sampler_free(q3tts_sampler* s) { delete s; }
int32_t q3tts_sampler_sample(q3tts_sampler* s, const float* logits, int32_t n_vocab, int32_t start, int32_t end) { return s->s.sample(logits, n_vocab, start, end); }
q3tts_chunker* q3tts_chunker_new(q3tts_decode_cb cb, void* user) {
    auto* h = new q3tts_chunker();
    h->c.reset(new Chunker([cb, user](const int64_t* codes, int n, bool fin) { if (cb) cb(user, codes, n, fin ? 1 : 0); }));
    return h;
}
void q3tts_chunker_free(q3tts_chunker* c) { delete c; }
int q3tts_chunker_push(q3tts_chunker* c, const int64_t* codes, int32_t n, int32_t is_final) { Q3_API_BEGIN c->c->push(codes, n, is_final != 0); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }

// ---------------- codec decoder ----------------
int q3tts_decoder_create(const char* path, int32_t n_streams, q3tts_decoder** out) {
    Q3_API_BEGIN
    require_gpu();
    auto* h = new q3tts_decoder();
    try { h->d.reset(new CodecDecoder(path, n_streams, 64)); Q3_HIP(hipStreamCreate(&h->st)); } catch (...) { delete h; throw; }
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_decoder_create_ex(const char* path, int32_t n_streams, int32_t max_frames, int32_t max_group, q3tts_decoder** out) {
    Q3_API_BEGIN
    require_gpu();
    Q3_CHECK(path && out && n_streams >= 1 && max_frames >= 1 && max_group >= 1, "bad arguments");
    auto* h = new q3tts_decoder();
    try { h->d.reset(new CodecDecoder(path, n_streams, max_frames, 1, max_group)); Q3_HIP(hipStreamCreate(&h->st)); } catch (...) { delete h; throw; }
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_decoder_decode_group(q3tts_decoder* d, int32_t G, const int32_t* streams, const int64_t* codes, int32_t n_frames, float* wav) {
    Q3_API_BEGIN
    Q3_CHECK(d && streams && codes && wav && G >= 1 && n_frames >= 1, "bad arguments");
    const size_t per = (size_t)n_frames * d->d->samples_per_frame();
    if (d->pinned_cap < per * G) { // pinned staging for the async D2H copies of the pass
        if (d->pinned) (void)hipHostFree(d->pinned);
        Q3_HIP(hipHostMalloc((void**)&d->pinned, per * G * sizeof(float)));
        d->pinned_cap = per * G;
    }
    std::vector<float*> dst(G);
    for (int g = 0; g < G; g++) dst[g] = d->pinned + (size_t)g * per;
    std::vector<int> st(streams, streams + G);
    const int got = d->d->decode_group_async(d->st, G, st.data(), codes, n_frames, dst.data(), 0);
    Q3_HIP(hipStreamSynchronize(d->st));
    if (got < 0) throw Error("decode failed");
    std::copy(d->pinned, d->pinned + per * G, wav);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_decoder_destroy(q3tts_decoder* d) { if (d && d->st) (void)hipStreamDestroy(d->st); if (d && d->pinned) (void)hipHostFree(d->pinned); delete d; }
int q3tts_decoder_samples_per_frame(q3tts_decoder* d) { return d->d->samples_per_frame(); }
int q3tts_decoder_reset(q3tts_decoder* d, int32_t stream) { Q3_API_BEGIN d->d->reset(stream); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_decoder_decode(q3tts_decoder* d, int32_t stream, const int64_t* codes, int32_t n_frames, int32_t is_last, float* wav, int64_t* valid) {
    Q3_API_BEGIN
    const int got = d->d->decode(d->st, stream, codes, n_frames, is_last != 0, wav);
    if (got < 0) throw Error("decode failed");
    if (valid) *valid = got;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

// DecoderState export / import (onnx.rs:461-496)
int64_t q3tts_decoder_state_floats(q3tts_decoder* d) { return d ? (int64_t)d->d->state_floats() : -1; }
int q3tts_decoder_state_export(q3tts_decoder* d, int32_t stream, float* out, int64_t n_floats) { Q3_API_BEGIN Q3_CHECK(d && out && n_floats >= 0, "null argument"); d->d->state_export(stream, out, (size_t)n_floats); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_decoder_state_import(q3tts_decoder* d, int32_t stream, const float* in, int64_t n_floats) { Q3_API_BEGIN Q3_CHECK(d && in && n_floats >= 0, "null argument"); d->d->state_import(stream, in, (size_t)n_floats); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
// [EXT] codec preambles: device-side snapshots on the decoder's own HIP stream (ordered with its decodes, no synchronisation)
int q3tts_decoder_snapshot_create(q3tts_decoder* d, int32_t stream, int32_t* snapshot) {
    Q3_API_BEGIN
    Q3_CHECK(d && snapshot, "null argument");
    *snapshot = d->d->snapshot_async(d->st, stream);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
int q3tts_decoder_snapshot_restore(q3tts_decoder* d, int32_t snapshot, int32_t stream) { Q3_API_BEGIN Q3_CHECK(d, "null argument"); d->d->restore_async(d->st, snapshot, stream); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int q3tts_decoder_snapshot_free(q3tts_decoder* d, int32_t snapshot) { Q3_API_BEGIN Q3_CHECK(d, "null argument"); d->d->snapshot_free(snapshot); return Q3TTS_OK; Q3_API_END(Q3TTS_ERR) }
int64_t q3tts_decoder_snapshot_bytes(q3tts_decoder* d) { return d ? (int64_t)d->d->snapshot_bytes() : -1; }
/* entry i of the layout: name (valid until the decoder is destroyed), offset in floats, rows x cols; returns the number of entries */
int32_t q3tts_decoder_state_entry(q3tts_decoder* d, int32_t i, const char** name, int64_t* offset, int32_t* rows, int32_t* cols) {
    if (!d) return -1;
    static thread_local std::vector<CodecStateEntry> lay;
    lay = d->d->state_layout();
    if (i >= 0 && i < (int)lay.size()) { if (name) *name = lay[i].name.c_str(); if (offset) *offset = lay[i].offset; if (rows) *rows = lay[i].rows; if (cols) *cols = lay[i].cols; }
    return (int32_t)lay.size();
}

// ---------------- transformer contexts ----------------
int q3tts_tf_open(const char* path, int32_t n_ctx, int32_t max_tok, q3tts_tf** out) {
    Q3_API_BEGIN
    require_gpu();
    auto model = std::make_shared<Transformer>(path, n_ctx, max_tok);
    auto* h = new q3tts_tf();
    h->c.reset(new TfContext(model, n_ctx));
    *out = h;
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}
void q3tts_tf_close(q3tts_tf* t) { delete t; }
int q3tts_tf_dims(q3tts_tf* t, int32_t* n_embd, int32_t* n_layer, int32_t* n_head, int32_t* n_vocab) {
    const auto& hp = t->c->model().hp();
    if (n_embd) *n_embd = hp.n_embd; if (n_layer) *n_layer = hp.n_layer; if (n_head) *n_head = hp.n_head; if (n_vocab) *n_vocab = hp.n_vocab;
    return Q3TTS_OK;
}
void q3tts_tf_clear(q3tts_tf* t) { t->c->clear(); }
int q3tts_tf_eval(q3tts_tf* t, const float* x, const int32_t* pos4, int32_t ntok, float* hidden_out, float* logits_out, int32_t row0, int32_t row1) {
    Q3_API_BEGIN
    t->c->eval(x, pos4, ntok, hidden_out, logits_out, row0, row1);
    return Q3TTS_OK;
    Q3_API_END(Q3TTS_ERR)
}

} // extern "C"
