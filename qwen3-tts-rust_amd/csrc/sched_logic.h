// sched_logic.h -- the scheduler's pure bookkeeping (no HIP, no threads; engine.cpp keeps what touches either): the request structs,
// the frame variant, the per-slot state table, the request states with what a cancel does in each, the staging cursor, the prefill chunk packer, the checks of a resumed prefix, of a score request, of a candidate set, of a decode-only request, of a codec preamble and of a prompt stem (with its take rule), the table of held objects both live in, what an admission wave takes from the queue, the chunk rows a score request needs the head for, how the decoder thread seats chunks in a codec pass and the queues they wait in, the rules of the output formats, the counts and the submit rule of the speaking rate, and the pair rule, the plan, the counts and the submit rule of the pitch, and the range, the gain and the submit rule of the volume, and the one record of a stream's output settings with what follows from it: the counts, the submit rule, the checks every output stage's launch shares and the routing of a pass's streams behind the output conv.
// tests/test_sched_logic_cpu.py builds it with plain g++.
#pragma once
#include "../../include/q3tts_spec.h"
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <deque>
#include <map>
#include <optional>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace q3 {

struct SamplerConfig { // engine.rs:13-45
    float temperature = 0.7f; int top_k = 40; float top_p = 0.9f; bool has_seed = false; uint64_t seed = 0;
};

// [EXT] generation controls beyond the reference (q3tts_spec.h "Repetition penalty" / "Sampled code predictor"); defaults = reference
struct GenOptions {
    float repetition_penalty = 1.0f;    // talker code_0; 1 = off
    float predictor_temperature = 0.0f; // <= 0: greedy predictor
    int predictor_top_k = 0;            // 0 = disabled
    float predictor_top_p = 1.0f;       // 1 = disabled
    bool penalised() const { return repetition_penalty != 1.0f; }
    bool pred_sampled() const { return predictor_temperature > 0.0f; }
};

struct GenRequest {
    const float* prompt = nullptr; int n_prompt = 0; // [n_prompt][2048] host
    SamplerConfig sampler;
    int max_steps = Q3_DEFAULT_MAX_STEPS;
    bool mask_eos = false;      // bench/test knob: exclude EOS so runs have a fixed length
    GenOptions opts;
    // [EXT] streaming-text talker input (q3tts_spec.h): trailing text ids, one per frame in the feedback; copied at submit
    const int32_t* trail = nullptr; int n_trail = 0;
    // [EXT] live text append (q3tts_spec.h): the trail stays open; frames past the appended ids wait until append_trail() brings more
    bool open = false;
    // [EXT] resume (q3tts_spec.h): frames 0 .. n_prefix-1 of the request, [n_prefix][16] codes; copied at submit
    const int32_t* prefix = nullptr; int n_prefix = 0;
    // [EXT] token log-probabilities (q3tts_spec.h): the request records 17 floats per frame; set by Engine::submit from the engine's flag
    bool logprobs = false;
    // [EXT] codec preambles (q3tts_spec.h): -2 the engine-level setting (the raw-prompt forms), -1 none, else that preamble (a text form
    // passes its voice's); resolved by Engine::submit, which never primes a request without PCM
    int preamble = -2;
    // [EXT] prompt stems (q3tts_spec.h): -2 the engine-level setting (the raw-prompt forms), -1 none, else that stem (a text form passes its
    // voice's); Engine::submit applies the take rule
    int stem = -2;
};

// Which launches one frame step issues: some live slot samples the talker / has a repetition penalty / samples the predictor / has trailing text
// ids (trail: the feedback kernel's streaming-text variant) / has an open trail (gate, implies trail: k_stall_save first, the gated k_advance_keys last)
// / records log-probabilities (lp: every head writes its logits, as sampled / pen / pred make it, and k_logprob_rows follows the talker's sampler)
struct FrameVariant {
    bool sampled = false, pen = false, pred = false, trail = false, gate = false, lp = false;
    // of the frame-graph cache; widths stay below 2^15, so the lp bit sits above every key without it and those keep their values
    int key(int width) const { return lp * (1 << 20) + width * 32 + gate * 16 + trail * 8 + pred * 4 + pen * 2 + sampled; }
};

// Every per-slot scalar the host mirrors, as one host block and one device block laid out [field][B] in 4-byte words (int32 or float), each
// row padded to 64 bytes.  The talker routing rows (t_seq, t_slot, t_pos[B][4]) are derived by route(); the device advances them itself.
enum SlotField { SF_TSEQ, SF_TSLOT, SF_TPOS, SF_FINISHED, SF_MAXFRAMES, SF_NFRAMES, SF_NPROMPT, SF_MASKEOS, SF_TEMP, SF_TOPK, SF_TOPP,
                 SF_PEN, SF_PTEMP, SF_PTOPK, SF_PTOPP, SF_NTRAIL, SF_OPEN, SF_COUNT };
struct SlotTable {
    int B = 0, off[SF_COUNT + 1] = {0}; // off: first word of each row
    std::vector<uint32_t> host; uint32_t* dev = nullptr; // dev: host.size() words the owner allocates once (captured graphs hold its addresses)
    std::vector<char> live; std::vector<const GenRequest*> req; // live: the slot steps inside the frame graph, for the request load() saw
    explicit SlotTable(int n = 0) : B(n), live(n, 0), req(n, nullptr) {
        for (int f = 0; f < SF_COUNT; f++) off[f + 1] = off[f] + (((f == SF_TPOS ? 4 : 1) * B + 15) & ~15);
        host.assign(off[SF_COUNT], 0); // padding stays zero
        for (int b = 0; b < B; b++) reset(b);
        route();
    }
    int32_t* hi(SlotField f) { return (int32_t*)(host.data() + off[f]); }
    float* hf(SlotField f) { return (float*)(host.data() + off[f]); }
    const int32_t* hi(SlotField f) const { return (const int32_t*)(host.data() + off[f]); }
    int32_t* di(SlotField f) const { return (int32_t*)(dev + off[f]); }
    float* df(SlotField f) const { return (float*)(dev + off[f]); }
    void reset(int b) { // the idle slot: finished, nothing to step, neutral sampler parameters, no text
        req[b] = nullptr;
        hi(SF_FINISHED)[b] = 1; hi(SF_MAXFRAMES)[b] = hi(SF_NFRAMES)[b] = hi(SF_NPROMPT)[b] = 0; hi(SF_MASKEOS)[b] = -1;
        hf(SF_TEMP)[b] = 0.0f; hi(SF_TOPK)[b] = 0; hf(SF_TOPP)[b] = 1.0f; hi(SF_NTRAIL)[b] = hi(SF_OPEN)[b] = 0;
        hf(SF_PEN)[b] = 1.0f; hf(SF_PTEMP)[b] = 0.0f; hi(SF_PTOPK)[b] = 0; hf(SF_PTOPP)[b] = 1.0f;
    }
    void load(int b, const GenRequest& r) { // a slot about to go live (an open trail's count and flag: Engine::go_live, under its lock)
        req[b] = &r;
        hi(SF_FINISHED)[b] = 0; hi(SF_MAXFRAMES)[b] = r.max_steps; hi(SF_NFRAMES)[b] = r.n_prefix; hi(SF_NPROMPT)[b] = r.n_prompt;
        hi(SF_MASKEOS)[b] = r.mask_eos ? Q3_CODEC_EOS : -1; hi(SF_NTRAIL)[b] = r.n_trail; hi(SF_OPEN)[b] = 0;
        hf(SF_TEMP)[b] = r.sampler.temperature; hi(SF_TOPK)[b] = r.sampler.top_k; hf(SF_TOPP)[b] = r.sampler.top_p;
        const GenOptions& o = r.opts;
        hf(SF_PEN)[b] = o.repetition_penalty; hf(SF_PTEMP)[b] = o.predictor_temperature; hi(SF_PTOPK)[b] = o.predictor_top_k; hf(SF_PTOPP)[b] = o.predictor_top_p;
    }
    void route() { // a live slot steps at position n_prompt + n_frames of its own sequence, an idle one on the scratch sequence (row B)
        for (int b = 0; b < B; b++) {
            const int t = live[b] ? hi(SF_NPROMPT)[b] + hi(SF_NFRAMES)[b] : 0;
            int32_t* pos = hi(SF_TPOS) + 4 * b;
            hi(SF_TSEQ)[b] = live[b] ? b : B; hi(SF_TSLOT)[b] = pos[0] = pos[1] = pos[2] = t; pos[3] = 0;
        }
    }
    // the host side of the device's stall predicate (the mirrors are exact between frame groups)
    bool stalled(int b) const { const int f = hi(SF_NFRAMES)[b]; return hi(SF_OPEN)[b] && !hi(SF_FINISHED)[b] && f < hi(SF_MAXFRAMES)[b] && f >= hi(SF_NTRAIL)[b]; }
    bool all_live_stalled() const {
        bool any = false;
        for (int b = 0; b < B; b++) if (live[b]) { if (!stalled(b)) return false; any = true; }
        return any;
    }
};

inline FrameVariant live_variant(const SlotTable& t) { // of the live batch
    FrameVariant v;
    for (int b = 0; b < t.B; b++) if (t.live[b]) {
        const GenRequest& r = *t.req[b];
        const bool open = t.hi(SF_OPEN)[b] != 0; // a closed trail leaves the gate, not the trail variant
        v.sampled |= r.sampler.temperature > 0.0f; v.pen |= r.opts.penalised(); v.pred |= r.opts.pred_sampled();
        v.trail |= r.n_trail > 0 || r.open || open; v.gate |= open; v.lp |= r.logprobs;
    }
    return v;
}

enum ReqState { REQ_QUEUED = 0, REQ_RUNNING = 1, REQ_DRAINING = 2, REQ_DONE = 3, REQ_CANCELLED = 4, REQ_FAILED = -1 };
inline bool req_ended(int state) { return state == REQ_DONE || state == REQ_CANCELLED || state == REQ_FAILED; }

// [EXT] request cancellation: what a cancel does to a request in `state`.  in_wave: RUNNING with a slot reserved but still inside an
// asynchronous prefill wave; live: RUNNING and stepping inside the frame graph; want_pcm: the request holds a codec stream.
enum CancelAction {
    CANCEL_NOTHING,     // already ended: the call returns 1
    CANCEL_AT_ONCE,     // QUEUED: leaves the queue and is CANCELLED in the caller's thread
    CANCEL_AT_ACTIVATE, // in a prefill wave: the wave is not disturbed, the request does not go live (then as RETIRE / RETIRE_FENCE)
    CANCEL_RETIRE,      // live, codes only: the slot is retired between two frame groups, CANCELLED right there
    CANCEL_RETIRE_FENCE,// live with PCM: retired without the tail flush, unstarted chunks dropped, a fence ends it once the codec is quiet
    CANCEL_PURGE        // DRAINING: unstarted chunks dropped, the fence already queued ends it
};
inline CancelAction cancel_action(int state, bool in_wave, bool live, bool want_pcm) {
    if (state == REQ_QUEUED) return CANCEL_AT_ONCE;
    if (state == REQ_DRAINING) return CANCEL_PURGE;
    if (state != REQ_RUNNING) return CANCEL_NOTHING;
    if (!live) return in_wave ? CANCEL_AT_ACTIVATE : CANCEL_NOTHING; // RUNNING without a slot does not exist
    return want_pcm ? CANCEL_RETIRE_FENCE : CANCEL_RETIRE;
}
// the state a request takes when its slot is retired (EOS, max_steps or a cancel) and when its fence completes
inline int retired_state(bool want_pcm, bool cancelled) { return want_pcm ? REQ_DRAINING : cancelled ? REQ_CANCELLED : REQ_DONE; }
inline int fenced_state(bool cancelled) { return cancelled ? REQ_CANCELLED : REQ_DONE; }

// The bump cursor of a pinned staging arena of `cap` bytes.  take() hands out the offset of the next 64-byte-aligned piece, or NONE when the
// piece does not fit behind what is in use; the cursor then stays as it is, and the owner decides: the AR arena waits for its stream and
// starts over (reset), the asynchronous prefill arena must never wait and treats NONE as an error.
struct StageCursor {
    static constexpr size_t NONE = ~(size_t)0;
    size_t cap = 0, used = 0;
    size_t take(size_t bytes) {
        if (bytes > cap) return NONE; // not even an empty arena serves it (and rounding up cannot wrap below)
        bytes = (bytes + 63) & ~(size_t)63;
        if (bytes > cap - used) return NONE;
        const size_t at = used;
        used += bytes;
        return at;
    }
    void reset() { used = 0; }
};

// Prefill: the prompts of one admission wave form one token stream.  Fills one chunk of at most n_max tokens from the cursor on -- prompt rows,
// per-token seq / slot / pos routing (engine.rs:306-314) -- and returns its token count; lasts = (request, index inside the chunk) of final prompt tokens.
// [EXT] resume: a request's n_fb feedback rows follow its prompt at positions n .. n + n_fb - 1.  They are not staged: the device writes them
// (k_feedback_codes), and fb lists each run of them inside the chunk.
// [EXT] prompt stems: a request's first n_skip rows are not prefilled (their K/V is restored from the stem's store); its cursor starts there, and
// positions and slots stay the row index, so every other row lands where it always did.
struct PromptRef { const float* rows; int n, slot; int n_fb = 0; int n_skip = 0; }; struct PrefillCursor { size_t req = 0; int tok = 0; };
struct FbRun { int req, row, frame, n; }; // request index, first row inside the chunk, first frame, number of rows
inline int pack_prefill_chunk(const std::vector<PromptRef>& batch, PrefillCursor& c, int n_max, float* stage, int32_t* seq, int32_t* slot,
                              int32_t* pos, std::vector<std::pair<int, int>>& lasts, std::vector<FbRun>* fb = nullptr) {
    int n = 0;
    if (fb) fb->clear();
    for (lasts.clear(); n < n_max && c.req < batch.size(); n++) {
        const PromptRef& r = batch[c.req];
        if (c.tok < r.n_skip) c.tok = r.n_skip;
        if (c.tok < r.n) std::copy(r.rows + (size_t)c.tok * Q3_EMBD, r.rows + (size_t)(c.tok + 1) * Q3_EMBD, stage + (size_t)n * Q3_EMBD);
        else if (fb) {
            if (!fb->empty() && fb->back().req == (int)c.req && fb->back().row + fb->back().n == n) fb->back().n++;
            else fb->push_back({(int)c.req, n, c.tok - r.n, 1});
        }
        seq[n] = r.slot; slot[n] = c.tok; pos[4 * n] = pos[4 * n + 1] = pos[4 * n + 2] = c.tok; pos[4 * n + 3] = 0;
        if (c.tok == r.n + r.n_fb - 1) { lasts.emplace_back((int)c.req, n); c.req++; c.tok = 0; } else c.tok++;
    }
    return n;
}
// the runs of staged (host) rows of a chunk of n rows: what fb leaves out, as (first row, count)
inline std::vector<std::pair<int, int>> staged_runs(int n, const std::vector<FbRun>& fb) {
    std::vector<std::pair<int, int>> out;
    int at = 0;
    for (const FbRun& f : fb) { if (f.row > at) out.emplace_back(at, f.row - at); at = f.row + f.n; }
    if (n > at) out.emplace_back(at, n - at);
    return out;
}

// [EXT] resume (q3tts_spec.h): why a prefix cannot be resumed, or null.  Pure: the submitting thread runs it before anything is queued.
// kv_rows = positions the slot's KV pages hold; codes [n_prefix][16].
inline const char* resume_refusal(int n_prompt, int max_steps, const int32_t* codes, int n_prefix, bool open, int n_trail, int64_t kv_rows) {
    if (n_prefix < 0) return "n_prefix must be >= 0";
    if (n_prefix == 0) return nullptr;
    if (n_prefix >= max_steps) return "n_prefix must be below max_steps: a resumed request generates at least one frame";
    if (!codes) return "prefix codes missing";
    for (int f = 0; f < n_prefix; f++) {
        const int32_t* c = codes + (size_t)f * 16;
        if (c[0] < 0 || c[0] >= Q3_SAMPLE_END) return "a prefix code_0 lies outside [0, Q3_SAMPLE_END)";
        if (c[0] == Q3_CODEC_EOS) return "a prefix frame is EOS: the request had ended there";
        for (int q = 1; q < 16; q++) if (c[q] < 0 || c[q] >= Q3_CODEBOOK_SIZE) return "a prefix residual code lies outside [0, 2048)";
    }
    if (open && n_trail < n_prefix) return "an open trail must hold at least n_prefix ids: the prefix frames ran, so their ids were known";
    if ((int64_t)n_prompt + n_prefix + 1 > kv_rows) return "n_prompt + n_prefix exceeds the slot's KV capacity";
    return nullptr;
}

// [EXT] scoring given frames (q3tts_spec.h "scoring"): why a score request is refused, or null.  Pure, like resume_refusal, whose code range
// checks it reuses (a score request has no frame to generate, so n = max_steps of the engine is allowed).  ggml: the engine runs Q3_SPEC=ggml.
inline const char* score_refusal(const float* prompt, int n_prompt, int max_prompt, const int32_t* trail, int n_trail, const int32_t* codes, int n,
                                 int max_steps, int64_t kv_rows, bool ggml) {
    if (ggml) return "scoring is not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)";
    if (n <= 0) return "n must be >= 1: there is no frame to score";
    if (n > max_steps) return "n exceeds the engine's max_steps";
    if (!codes) return "codes missing";
    if (!prompt) return "prompt missing";
    if (n_prompt < 1 || n_prompt > max_prompt) return "prompt length out of range";
    if (n_trail < 0 || n_trail > max_prompt) return "n_trail must be in [0, max_prompt]";
    if (n_trail > 0 && !trail) return "trailing ids missing";
    if ((int64_t)n_prompt + n > kv_rows) return "n_prompt + n exceeds the slot's KV capacity";
    // the code ranges: resume_refusal's, with its own limits out of the way (n + 1 steps, a closed trail, the capacity checked above)
    return resume_refusal(n_prompt, n + 1, codes, n, false, n_trail, (int64_t)n_prompt + n + 1);
}

// [EXT] candidate sets (q3tts_spec.h "candidate sets"): why a set of n seeded candidates of one prompt is refused, or null.  Pure, like the two
// above; the prompt, max_steps and the options are checked by the rule every submission goes through.  A set takes no resumed prefix and no
// open trail, so neither appears here.
inline const char* candidates_refusal(int n, int max_batch, const uint64_t* seeds, const int64_t* req_ids, const int32_t* trail, int n_trail,
                                      int max_prompt, bool ggml) {
    if (ggml) return "candidate sets are not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)";
    if (n < 1) return "n must be >= 1: a set has at least one candidate";
    if (n > max_batch) return "n exceeds max_batch: a set is admitted whole, one slot per candidate";
    if (!seeds) return "seeds missing";
    if (!req_ids) return "req_ids missing";
    if (n_trail < 0 || n_trail > max_prompt) return "n_trail must be in [0, max_prompt]";
    if (n_trail > 0 && !trail) return "trailing ids missing";
    return nullptr;
}

// [EXT] decoding given frames (q3tts_spec.h "decoding given frames"): why a decode-only request is refused, or null.  Pure, like the three above.
// The code ranges are resume_refusal's: no request emits a frame outside them, so there is no PCM "of a request that emitted it" to deliver.
inline const char* decode_refusal(const int32_t* codes, int n, int max_steps, bool have_codec) {
    if (!have_codec) return "the engine was created with load_codec = 0: there is no codec to decode with";
    if (n < 1) return "n must be >= 1: there is no frame to decode";
    if (n > max_steps) return "n exceeds the engine's max_steps (a codec stream's staging region holds max_steps frames)";
    if (!codes) return "codes missing";
    return resume_refusal(1, n + 1, codes, n, false, 0, (int64_t)n + 2); // the ranges alone: its own limits are out of the way
}

// [EXT] held objects: what codec preambles and prompt stems have in common.  Both are numbered things built once, asynchronously, by a hidden
// request.  Who holds one: its creator until the release call, and `holders` = the voices it is set on, the engine-level setting, and the
// requests submitted with it that have not ended (a request with PCM ends behind its fence, so every restore it enqueued has completed).
enum { HELD_BUILDING = 0, HELD_READY = 1, HELD_FAILED = -1 };
static_assert(Q3TTS_PREAMBLE_BUILDING == HELD_BUILDING && Q3TTS_PREAMBLE_READY == HELD_READY && Q3TTS_PREAMBLE_FAILED == HELD_FAILED &&
              Q3TTS_STEM_BUILDING == HELD_BUILDING && Q3TTS_STEM_READY == HELD_READY && Q3TTS_STEM_FAILED == HELD_FAILED, "one table serves both kinds");
struct HeldRefs {
    bool creator = true; int holders = 0; int state = HELD_BUILDING;
    // what the object owns on the device goes back only when nobody holds it and its build has ended (a building one is still being written)
    bool recyclable() const { return !creator && holders == 0 && state != HELD_BUILDING; }
};
struct HeldWords { // the messages of one kind, noun = "preamble" / "stem"
    const std::string unknown, released, building, failed, bad_id;
    explicit HeldWords(const std::string& noun)
        : unknown("unknown " + noun + " id"), released("the " + noun + " has already been released"),
          building("the " + noun + " is still building: wait for it (q3tts_" + noun + "_wait)"), failed("the " + noun + " failed to build"),
          bad_id(noun + " id must be -1 (none) or a " + noun + "'s id") {}
    // what a setter (voice or engine level) refuses, or null: it takes a READY object only, so "primed or not" / "taken or not" never depends on timing
    const char* set_refusal(bool known, int state) const {
        return !known ? unknown.c_str() : state == HELD_BUILDING ? building.c_str() : state != HELD_READY ? failed.c_str() : nullptr;
    }
};
// the same two answers asked per kind, as the rule drivers of tests/host ask them: both kinds count alike and word their refusals alike
typedef HeldRefs PreambleRefs;
inline bool preamble_recyclable(const HeldRefs& p) { return p.recyclable(); }
inline const char* preamble_set_refusal(bool known, int state) { static const HeldWords w("preamble"); return w.set_refusal(known, state); }
inline const char* stem_set_refusal(bool known, int state) { static const HeldWords w("stem"); return w.set_refusal(known, state); }
// The live objects of one kind by id, the next id (never reused) and the engine-level setting (-1: none).  No lock: the engine calls it under
// its own.  Whatever ends the last hold -- unhold, release_creator, finish, swap_setting -- removes the entry and hands its payload back, and the
// caller disposes of what the payload owns; nothing else removes an entry.
template <class Payload> class HeldTable {
public:
    struct Entry { HeldRefs refs; int n = 0; Payload payload{}; }; // n: frames of a preamble, rows of a stem
    using Recycled = std::optional<Payload>;
    const HeldWords words; int setting = -1;
    explicit HeldTable(const char* noun) : words(noun) {}
    const std::map<int, Entry>& entries() const { return map_; }
    int live() const { return (int)map_.size(); }
    int add(int n) { const int id = next_++; map_[id].n = n; return id; } // its creator holds it, nobody else, building
    Entry* find(int id) { auto it = map_.find(id); return it == map_.end() ? nullptr : &it->second; }
    Entry& at(int id) { if (Entry* e = find(id)) return *e; throw std::runtime_error(words.unknown); }
    void hold(int id) { at(id).refs.holders++; }
    Recycled unhold(int id) { // one holder less; an unknown id is nobody's
        auto it = map_.find(id);
        if (it == map_.end()) return std::nullopt;
        it->second.refs.holders--;
        if (!it->second.refs.recyclable()) return std::nullopt;
        Recycled out(std::move(it->second.payload));
        map_.erase(it);
        return out;
    }
    Recycled release_creator(int id) { // the creator's reference becomes a holder's, which is dropped: recycles when nobody else holds it
        Entry& e = at(id);
        if (!e.refs.creator) throw std::runtime_error(words.released);
        e.refs.creator = false; e.refs.holders++;
        return unhold(id);
    }
    Recycled finish(int id, bool ok) { // the build has ended; recycles at once when it was released while it built
        Entry* e = find(id);
        if (!e) return std::nullopt;
        e->refs.state = ok ? HELD_READY : HELD_FAILED; e->refs.holders++;
        return unhold(id);
    }
    void fail_building() { for (auto& kv : map_) if (kv.second.refs.state == HELD_BUILDING) kv.second.refs.state = HELD_FAILED; } // nothing builds them any more
    const char* set_refusal(int id) const { auto it = map_.find(id); return words.set_refusal(it != map_.end(), it != map_.end() ? it->second.refs.state : 0); }
    // a setter: `which` (a voice's setting or this table's own) becomes id.  The new object is held before the old one is dropped, so setting the
    // same id twice never recycles it; a refusal leaves everything as it was
    Recycled swap_setting(int& which, int id) {
        if (id >= 0) { if (const char* why = set_refusal(id)) throw std::runtime_error(why); hold(id); }
        else if (id != -1) throw std::runtime_error(words.bad_id);
        const int old = which;
        which = id;
        return old >= 0 ? unhold(old) : std::nullopt;
    }
private:
    std::map<int, Entry> map_; int next_ = 0;
};

// [EXT] codec preambles (q3tts_spec.h "codec preambles"): why a preamble of n frames is refused, or null.  Pure, like the four above.  A preamble
// is built like a decode-only request, so decode_refusal's reasons come first; live = preambles the engine holds now (building ones included).
// Frame f of a primed request sits at RoPE position n + f, so n + max_steps must stay within the codec's positions.
inline const char* preamble_refusal(const int32_t* codes, int n, int max_steps, bool have_codec, int live, int64_t max_positions) {
    if (const char* why = decode_refusal(codes, n, max_steps, have_codec)) return why;
    if (live >= Q3TTS_MAX_PREAMBLES) return "Q3TTS_MAX_PREAMBLES preambles are live: release one first";
    if ((int64_t)n + max_steps > max_positions) return "n + max_steps exceeds the codec's frame positions";
    return nullptr;
}
// the preamble a request is primed with: never without PCM; a text form takes its voice's, a raw-prompt form the engine-level setting
enum { PREAMBLE_NONE = -1, PREAMBLE_ENGINE = -2 };
inline int preamble_of_request(bool want_pcm, int asked, int engine_level) {
    if (!want_pcm) return PREAMBLE_NONE;
    return asked == PREAMBLE_ENGINE ? engine_level : asked;
}

// [EXT] prompt stems (q3tts_spec.h "prompt stems").  The states and the holder rule are HeldTable's: the store goes back when nobody holds the
// stem and its build has ended; a request that took it holds it from submit to its end, so every restore enqueued from it has completed by then.
// why a stem of n rows is refused, or null.  Pure; live = stems the engine holds now (building ones included)
inline const char* stem_refusal(const float* rows, int n, int max_prompt, int live, bool ggml) {
    if (ggml) return "prompt stems are not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)";
    if (!rows) return "stem rows missing";
    if (n < 1) return "n_rows must be >= 1";
    if (n >= max_prompt) return "n_rows must be below max_prompt: a request that takes a stem has at least one row of its own";
    if (live >= Q3TTS_MAX_STEMS) return "Q3TTS_MAX_STEMS stems are live: release one first";
    return nullptr;
}
// the stem that applies to a request: a text form passes its voice's, a raw-prompt form takes the engine-level setting
enum { STEM_NONE = -1, STEM_ENGINE = -2 };
inline int stem_of_request(int asked, int engine_level) { return asked == STEM_ENGINE ? engine_level : asked; }
// the take rule, given that a stem of n rows in `state` applies: READY, n_prompt > n, the first n rows bytewise equal; never a score request
inline bool stem_takes(int state, int n, const float* stem_rows, const float* prompt, int n_prompt, bool score) {
    if (score || state != Q3TTS_STEM_READY || n < 1 || n_prompt <= n || !stem_rows || !prompt) return false;
    return std::memcmp(stem_rows, prompt, (size_t)n * Q3_EMBD * sizeof(float)) == 0; // bytes: -0 differs from +0 and a NaN equals itself
}
inline int stem_pages(int n) { return (n + 63) / 64; }
// device bytes of a stem's store: K and V planes of whole pages, f16
inline int64_t stem_store_bytes(int n, int n_layer, int n_kv) { return (int64_t)2 * stem_pages(n) * n_layer * n_kv * 8192 * 2; }
// the rows of a request that an admission wave stages and prefills
inline int admission_rows(int n_prompt, int n_skip, int n_prefix) { return n_prompt - n_skip + n_prefix; }

// Decode-only requests that may hold a codec stream at once: half of the streams the engine keeps beyond one per slot (those serve
// requests whose slot is already reused while their last chunks drain), and how many of the queued ones a scheduler step admits after
// the generating wave has taken its streams.
inline int decode_width(int n_cs, int max_batch) { return std::max(1, (n_cs - max_batch) / 2); }
inline int decode_admit(int queued, int free_cs, int holding, int width) { return std::max(0, std::min(queued, std::min(free_cs, width - holding))); }

// The decoder thread's next step.  It has two queues: `live` (tasks of generating requests) and `low` (tasks of decode-only requests), each in
// arrival order; a request's tasks are reset, chunks, fence, in that order, and all sit in one queue.  A step is one task alone (a reset or a
// fence) or one codec pass: chunks of equal frame count, one per request, at most gmax.  Only a request's first pending task can be chosen.
//   control  a reset or fence that heads a decode-only request's tasks runs at once, alone (no codec work; it keeps a stream's turnover short)
//   lead     the head of the live queue -- a reset or fence runs alone, a chunk leads the pass; with the live queue empty, the oldest
//            decode-only chunk leads
//   seats    the first pending chunks of the other generating requests with the lead's frame count, in queue order, then those of
//            decode-only requests, in queue order
//   epoch    the generating chunks of one pass come from one hand-over (TaskHead::epoch: the scheduler numbers its hand-overs and gives a
//            hand-over's tasks to the thread in one piece).  A pass then holds the same chunks whether the thread forms it before or after
//            the next hand-over arrives, so what a request's samples are computed with -- the rows of its pass pick the GEMM forms --
//            depends on the schedule and not on how fast the thread runs.  Decode-only chunks carry no epoch: they take the seats left
//   turn     after SEAT_DRY_MAX consecutive passes that seated no decode-only chunk while one was waiting, the oldest decode-only chunk
//            leads the next pass; generating chunks of its frame count still take the other seats first
// With the low queue empty this is the grouping the thread always did.  dry = the count of such passes so far; the result carries the next.
enum TaskKind { TASK_CHUNK = 0, TASK_RESET = 1, TASK_FENCE = 2 };
enum { SEAT_DRY_MAX = 4 };
struct TaskHead { int64_t req; int frames; int kind; int64_t epoch = 0; }; // frames: of a chunk, else 0; epoch: of a generating request's task
struct Seat { bool low; int index; };                   // index into its queue
struct Seating { std::vector<Seat> seats; int dry = 0; };
inline Seating seat_chunks(const std::vector<TaskHead>& live, const std::vector<TaskHead>& low, int gmax, int dry) {
    Seating out;
    out.dry = dry;
    // the first pending task of every decode-only request, in queue order
    std::vector<int> heads; std::vector<int64_t> seen;
    for (int i = 0; i < (int)low.size(); i++)
        if (std::find(seen.begin(), seen.end(), low[i].req) == seen.end()) { seen.push_back(low[i].req); heads.push_back(i); }
    for (int i : heads) if (low[i].kind != TASK_CHUNK) { out.seats.push_back({true, i}); return out; }
    if (live.empty() && heads.empty()) return out;
    const bool turn = !heads.empty() && (live.empty() || dry >= SEAT_DRY_MAX);
    if (!turn && live[0].kind != TASK_CHUNK) { out.seats.push_back({false, 0}); return out; }
    const TaskHead& lead = turn ? low[heads[0]] : live[0];
    out.seats.push_back({turn, turn ? heads[0] : 0});
    seen.assign(1, lead.req); // request ids are the engine's: no two requests share one, whichever queue they wait in
    bool bound = !turn; int64_t epoch = lead.epoch; // a decode-only lead binds the pass to the epoch of the first generating chunk it seats
    for (int i = 0; i < (int)live.size() && (int)out.seats.size() < gmax; i++) {
        const bool dup = std::find(seen.begin(), seen.end(), live[i].req) != seen.end();
        if (!dup) seen.push_back(live[i].req);
        if (dup || live[i].kind != TASK_CHUNK || live[i].frames != lead.frames || (bound && live[i].epoch != epoch)) continue;
        out.seats.push_back({false, i});
        bound = true; epoch = live[i].epoch;
    }
    bool seated_low = turn;
    for (int i : heads) {
        if ((int)out.seats.size() >= gmax) break;
        if (turn && i == heads[0]) continue;
        if (low[i].frames == lead.frames) { out.seats.push_back({true, i}); seated_low = true; }
    }
    out.dry = seated_low ? 0 : heads.empty() ? 0 : dry + 1;
    return out;
}

// The decoder thread's two queues and every count that goes with them; the thread's owner locks around it.  Job is what the thread sees of a
// request: `id` (TaskHead::req) and `decode` (which queue).
//   pending  chunk and fence tasks queued, or taken and their completion not yet popped (a reset completes nothing).  Assigned here only
//   hold     hand-overs open: the scheduler queues a frame group's chunks, fences and decode-only tasks and no step is taken meanwhile
//   epoch    hand-overs so far; a generating request's chunk carries the number of the one it came with, every other task none (seat_chunks)
template <class Job> struct CodecQueue {
    struct Task { Job* job; TaskKind kind; std::vector<int64_t> codes; bool is_final; int64_t epoch; };
    std::deque<Task> live, low;
    int pending = 0, hold = 0, dry = 0; int64_t epoch = 0; // dry: seat_chunks' count, carried from step to step
    void open() { if (hold++ == 0) epoch++; } // a hand-over inside another belongs to it
    void close() { hold--; }
    void push(Job* j, TaskKind kind, const int64_t* codes = nullptr, int n_codes = 0, bool is_final = false) {
        (j->decode ? low : live).push_back(Task{j, kind, std::vector<int64_t>(codes, codes + n_codes), is_final, kind == TASK_CHUNK && !j->decode ? epoch : 0});
        if (kind != TASK_RESET) pending++;
    }
    void purge(Job* j) { // the chunks of j nobody has taken yet; what has been taken runs to its end
        std::deque<Task>& q = j->decode ? low : live;
        for (auto it = q.begin(); it != q.end();) {
            if (it->job == j && it->kind == TASK_CHUNK) { it = q.erase(it); pending--; }
            else ++it;
        }
    }
    bool ready() const { return hold == 0 && !(live.empty() && low.empty()); }
    std::vector<Task> take(int gmax) { // the next step: what seat_chunks seats, in its order; nothing while a hand-over is open
        std::vector<Task> step;
        if (!ready()) return step;
        auto heads = [](const std::deque<Task>& q) {
            std::vector<TaskHead> h;
            for (const Task& t : q) h.push_back({t.job->id, (int)t.codes.size() / 16, t.kind, t.epoch});
            return h;
        };
        const Seating s = seat_chunks(heads(live), heads(low), gmax, dry);
        dry = s.dry;
        for (const Seat& c : s.seats) step.push_back(std::move((c.low ? low : live)[c.index]));
        for (int lo = 0; lo < 2; lo++) { // the seated tasks leave their queue, last first
            std::vector<int> idx;
            for (const Seat& c : s.seats) if ((int)c.low == lo) idx.push_back(c.index);
            std::sort(idx.rbegin(), idx.rend());
            for (int i : idx) (lo ? low : live).erase((lo ? low : live).begin() + i);
        }
        return step;
    }
    void popped() { pending--; } // a chunk's or a fence's completion has left the completion FIFO
};

// How many entries from the head of the queue the next admission wave takes.  A plain request (set = 0) needs a slot, a codec stream when it
// wants PCM, and -- limit_rows: an asynchronous wave, whose prompts sit in one staging arena -- room for its rows below max_rows unless it
// is the wave's first.  The members of a candidate set are the consecutive entries with its id (those cancelled in the queue have left it):
// they are taken all or none, need a slot and a codec stream each, and their rows count once, since one member alone is prefilled.
// Whatever does not fit ends the wave, so nothing overtakes it.  With no set in the queue this is the loop admit() always ran.
struct QueueEntry { int rows; bool want_pcm; int64_t set; }; // rows: n_prompt - n_skip + n_prefix ([EXT] prompt stems: admission_rows)
inline int admission_take(const std::vector<QueueEntry>& q, int free_slots, int free_codec, bool limit_rows, size_t max_rows = 4096) {
    size_t take = 0, rows = 0;
    while (take < q.size() && free_slots > 0) {
        const QueueEntry& e = q[take];
        size_t k = 1;
        if (e.set != 0) while (take + k < q.size() && q[take + k].set == e.set) k++;
        if ((size_t)free_slots < k) break;
        if (e.want_pcm && (size_t)free_codec < k) break; // every codec stream still drains: after the next harvest
        if (limit_rows && take > 0 && rows + (size_t)e.rows > max_rows) break;
        take += k; free_slots -= (int)k; rows += (size_t)e.rows;
        if (e.want_pcm) free_codec -= (int)k;
    }
    return (int)take;
}

// The rows of one prefill chunk that a score request needs the talker head for.  Frame f of a request with n prompt rows is scored from row
// n - 1 + f of its stream: the last prompt row and every feedback row (the packer is given n_fb = frames - 1 feedback rows, so the stream ends
// with the row of the last frame).  `before` is the cursor pack_prefill_chunk started the chunk from, n_chunk the token count it returned;
// a run is (request, first row inside the chunk, first frame, number of rows), in chunk order.  score[i] != 0: request i is a score request.
struct ScoreRun { int req, row, frame, n; };
inline std::vector<ScoreRun> score_head_runs(const std::vector<PromptRef>& batch, const std::vector<char>& score, PrefillCursor before, int n_chunk) {
    std::vector<ScoreRun> out;
    PrefillCursor c = before;
    for (int i = 0; i < n_chunk && c.req < batch.size(); i++) {
        const PromptRef& r = batch[c.req];
        if (c.tok < r.n_skip) c.tok = r.n_skip; // as the packer
        if (score[c.req] && c.tok >= r.n - 1) {
            if (!out.empty() && out.back().req == (int)c.req && out.back().row + out.back().n == i) out.back().n++;
            else out.push_back({(int)c.req, i, c.tok - (r.n - 1), 1});
        }
        if (c.tok == r.n + r.n_fb - 1) { c.req++; c.tok = 0; } else c.tok++;
    }
    return out;
}

// [EXT] output formats (q3tts_spec.h "output formats"): the eight rates and their ratios, which formats exist, what comes out of n frames.
constexpr int PCM_N_RATES = 8;
inline const int* pcm_rates() { static const int r[PCM_N_RATES] = {8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000}; return r; }
inline int pcm_rate_index(int rate) { // -1: not one of the eight
    for (int i = 0; i < PCM_N_RATES; i++) if (pcm_rates()[i] == rate) return i;
    return -1;
}

// rate = 24000 * L / M in lowest terms; n_taps = N of the prototype, taps_per_phase = the most terms one output sample sums.
// 24000 itself has no filter: L = M = 1 and no taps.
struct PcmPlan { int L = 1, M = 1, n_taps = 0, taps_per_phase = 0; };
inline bool pcm_plan(int rate, PcmPlan* out) {
    if (pcm_rate_index(rate) < 0) return false;
    int a = rate, b = Q3_PCM_NATIVE_RATE;
    while (b) { const int t = a % b; a = b; b = t; }
    PcmPlan p;
    p.L = rate / a; p.M = Q3_PCM_NATIVE_RATE / a;
    if (rate != Q3_PCM_NATIVE_RATE) {
        const int F = p.L > p.M ? p.L : p.M;
        p.n_taps = 2 * Q3_PCM_FILTER_Z * F + 1;
        p.taps_per_phase = (p.n_taps + p.L - 1) / p.L;
    }
    *out = p;
    return true;
}
// output samples of n_native native samples from a stream's reset: floor(n_native * L / M); -1 for an unknown rate or a negative count
inline int64_t pcm_samples_of_native(int rate, int64_t n_native) {
    PcmPlan p;
    if (n_native < 0 || !pcm_plan(rate, &p)) return -1;
    return n_native * p.L / p.M;
}

// which formats exist: nullptr = allowed, else the reason.  f32 only up to the native rate, so that no format needs more bytes per native
// sample than the native one.
inline const char* pcm_format_why_not(int rate, int encoding) {
    if (pcm_rate_index(rate) < 0) return "unknown sample rate";
    if (encoding != Q3_PCM_F32 && encoding != Q3_PCM_S16) return "unknown encoding";
    if (encoding == Q3_PCM_F32 && rate > Q3_PCM_NATIVE_RATE) return "f32 is delivered up to 24000 Hz only";
    return nullptr;
}
inline bool pcm_format_native(const q3tts_pcm_format& f) { return f.sample_rate == Q3_PCM_NATIVE_RATE && f.encoding == Q3_PCM_F32; }

// what a request may ask for and what n frames of it come to.  f == NULL is the native format.  No format needs more bytes than the native one, so a staging region sized for native floats serves every format.
inline const char* pcm_format_refusal(const q3tts_pcm_format* f, bool have_codec) {
    if (!have_codec) return "the engine has no codec";
    return f ? pcm_format_why_not(f->sample_rate, f->encoding) : nullptr;
}
inline int64_t pcm_out_samples(const q3tts_pcm_format& f, int64_t n_frames) { return pcm_samples_of_native(f.sample_rate, n_frames * Q3_PCM_FRAME); }
inline int64_t pcm_out_bytes(const q3tts_pcm_format& f, int64_t n_frames) {
    const int64_t n = pcm_out_samples(f, n_frames);
    return n < 0 ? -1 : n * (f.encoding == Q3_PCM_S16 ? 2 : 4);
}

// [EXT] speaking rate (q3tts_spec.h "speaking rate"): which rates exist, how many frames and samples n_native samples come to, and what a
// request with a rate may ask for.  The counts depend on pct and n_native alone, never on the samples: the host computes every size and offset.
inline const char* tsm_rate_why_not(int pct) { return (pct < Q3_TSM_MIN || pct > Q3_TSM_MAX) ? "speech rate out of range [50, 200]" : nullptr; }
inline int64_t tsm_analysis_pos(int pct, int64_t k) { return k * Q3_TSM_HOP * pct / 100; }
// synthesis frames of a stream that has seen n_native samples: #{k : a_k + 1200 <= N} while streaming, #{k : a_k < N} once it is final
inline int64_t tsm_frames(int pct, int64_t n_native, bool final) {
    if (tsm_rate_why_not(pct) || n_native < 0) return -1;
    const int64_t step = (int64_t)Q3_TSM_HOP * pct;   // a_k = floor(k * step / 100)
    if (final) return (100 * n_native + step - 1) / step;
    if (n_native < Q3_TSM_LOOK) return 0;
    return (100 * (n_native - Q3_TSM_LOOK + 1) - 1) / step + 1;   // a_k <= N - 1200  <=>  k * step < 100 (N - 1199)
}
inline int64_t tsm_out_samples(int pct, int64_t n_native, bool final) {
    const int64_t f = tsm_frames(pct, n_native, final);
    return f < 0 ? -1 : f * Q3_TSM_HOP;
}
// the submit rule.  A request with pct != 100 delivers 24000 Hz, f32 or s16, and its flushed utterance of max_steps frames must fit the
// stream's staging region of cap_bytes bytes (slowing down makes more samples than native).  nullptr = it may be queued
inline const char* tsm_submit_refusal(int pct, const q3tts_pcm_format& f, int max_steps, int64_t cap_bytes, bool have_codec) {
    if (!have_codec) return "the engine has no codec";
    if (const char* why = tsm_rate_why_not(pct)) return why;
    if (pct == 100) return nullptr;
    if (f.sample_rate != Q3_PCM_NATIVE_RATE) return "a speech rate needs the 24000 Hz output format";
    if (f.encoding != Q3_PCM_F32 && f.encoding != Q3_PCM_S16) return "unknown encoding";
    if (tsm_out_samples(pct, (int64_t)max_steps * Q3_PCM_FRAME, true) * (f.encoding == Q3_PCM_S16 ? 2 : 4) > cap_bytes)
        return "max_steps at this speech rate makes more PCM than a request's staging holds";
    return nullptr;
}

// [EXT] pitch (q3tts_spec.h "pitch"): a shift by P percent is the stretcher at the rational tempo R / P followed by an L / M resample,
// L / M = 100 / P in lowest terms.  Which pitches and (rate, pitch) pairs exist, the plan of a pitch's resampler, how many stage-1 frames and
// delivered samples n_native samples come to, and what a request with a pitch may ask for.  Every count depends on R, P and n_native alone.
inline const char* pitch_why_not(int P) { return (P < Q3_PITCH_MIN || P > Q3_PITCH_MAX) ? "pitch out of range [50, 200]" : nullptr; }
// the pair rule: the tempo R / P lies in [1/2, 2], which keeps a frame's reach inside Q3_TSM_HIST (q3tts_spec.h "pitch", reach)
inline const char* prosody_pair_why_not(int R, int P) {
    if (const char* why = tsm_rate_why_not(R)) return why;
    if (const char* why = pitch_why_not(P)) return why;
    return (2 * R < P || R > 2 * P) ? "speech rate / pitch outside [1/2, 2]" : nullptr;
}
inline int64_t pitch_analysis_pos(int R, int P, int64_t k) { return k * Q3_TSM_HOP * R / P; }
// stage-1 frames of a stream that has seen n_native samples: #{k : a_k + 1200 <= N} while streaming, #{k : a_k < N} once it is final
inline int64_t pitch_frames(int R, int P, int64_t n_native, bool final) {
    if (prosody_pair_why_not(R, P) || n_native < 0) return -1;
    const int64_t step = (int64_t)Q3_TSM_HOP * R;   // a_k = floor(k * step / P)
    if (final) return (P * n_native + step - 1) / step;
    if (n_native < Q3_TSM_LOOK) return 0;
    return (P * (n_native - Q3_TSM_LOOK + 1) - 1) / step + 1;   // a_k <= N - 1200  <=>  k * step < P (N - 1199)
}
// the resampler of a pitch: L / M = 100 / P in lowest terms, n_taps = N of the prototype, taps_per_output = the most terms one sample sums
struct PitchPlan { int L = 1, M = 1, n_taps = 0, taps_per_output = 0; };
inline bool pitch_plan(int P, PitchPlan* out) {
    if (pitch_why_not(P)) return false;
    int a = 100, b = P;
    while (b) { const int t = a % b; a = b; b = t; }
    PitchPlan p;
    p.L = 100 / a; p.M = P / a;
    const int F = p.L > p.M ? p.L : p.M;
    p.n_taps = 2 * Q3_PCM_FILTER_Z * F + 1;
    p.taps_per_output = (p.n_taps + p.L - 1) / p.L;
    *out = p;
    return true;
}
// delivered samples of nz stage-1 samples from a stream's reset: ceil(nz * L / M), since y[n] needs z[n M div L] and nothing later
inline int64_t pitch_samples_of_z(const PitchPlan& p, int64_t nz) { return (nz * p.L + p.M - 1) / p.M; }
inline int64_t pitch_out_samples(int R, int P, int64_t n_native, bool final) {
    const int64_t f = pitch_frames(R, P, n_native, final);
    PitchPlan p;
    if (f < 0 || !pitch_plan(P, &p)) return -1;
    return pitch_samples_of_z(p, f * Q3_TSM_HOP);
}
// the submit rule of a request with pitch P != 100 at rate R: the pair, 24000 Hz, f32 or s16, and its flushed utterance of max_steps frames
// must fit the stream's staging region of cap_bytes bytes.  nullptr = it may be queued
inline const char* pitch_submit_refusal(int R, int P, const q3tts_pcm_format& f, int max_steps, int64_t cap_bytes, bool have_codec) {
    if (!have_codec) return "the engine has no codec";
    if (const char* why = prosody_pair_why_not(R, P)) return why;
    if (P == 100) return tsm_submit_refusal(R, f, max_steps, cap_bytes, have_codec);
    if (f.sample_rate != Q3_PCM_NATIVE_RATE) return "a pitch needs the 24000 Hz output format";
    if (f.encoding != Q3_PCM_F32 && f.encoding != Q3_PCM_S16) return "unknown encoding";
    if (pitch_out_samples(R, P, (int64_t)max_steps * Q3_PCM_FRAME, true) * (f.encoding == Q3_PCM_S16 ? 2 : 4) > cap_bytes)
        return "max_steps at this speech rate and pitch makes more PCM than a request's staging holds";
    return nullptr;
}

// [EXT] volume (q3tts_spec.h "volume"): which volumes exist, the f32 gain of one, and what a request with a volume may ask for.  The stage
// changes no count: n native samples in, n out.
inline const char* volume_why_not(int db10) { return (db10 < Q3_VOL_MIN || db10 > Q3_VOL_MAX) ? "volume out of range [-400, 200]" : nullptr; }
// G = (float) pow(10.0, db10 / 200.0); NaN for a volume out of range
inline float volume_gain(int db10) { return volume_why_not(db10) ? std::nanf("") : (float)std::pow(10.0, (double)db10 / 200.0); }
// the submit rule of a request with volume db10 (0: off, always allowed where there is a codec).  nullptr = it may be queued
inline const char* volume_submit_refusal(int db10, bool have_codec) {
    if (!have_codec) return "the engine has no codec";
    return volume_why_not(db10);
}

// [EXT] the output settings of one stream (q3tts_spec.h "output formats" / "speaking rate" / "pitch" / "volume") as one record: what the
// engine's setters write, what a request reads once at submit and what the codec's pass tail is given per stream.  The default is the plain
// stream: native format, no rate, no pitch, no volume.  A setting more is a field here and a branch where the pass tail delivers.
// loud: [EXT] loudness (q3tts_spec.h "loudness"): nonzero = the stream is metered; it changes no sample and no count
struct OutSpec { q3tts_pcm_format fmt{Q3_PCM_NATIVE_RATE, Q3_PCM_F32}; int32_t rate_pct = 100, pitch_pct = 100, vol_db10 = 0; int32_t loud = 0; };
// whose stream it is behind the output conv: nobody's, the converter's, the stretcher's, the shifter's (a pitch wins over a rate, a rate over a
// format).  The volume is no kind: it rewrites the native chunk in front of any of them; nor is the meter, which reads it in front of the volume
enum OutKind : uint8_t { OUT_NATIVE, OUT_CONVERTED, OUT_RATED, OUT_PITCHED };
inline OutKind out_kind(const OutSpec& o) {
    return o.pitch_pct != 100 ? OUT_PITCHED : o.rate_pct != 100 ? OUT_RATED : !pcm_format_native(o.fmt) ? OUT_CONVERTED : OUT_NATIVE;
}
inline size_t out_sample_bytes(const OutSpec& o) { return o.fmt.encoding == Q3_PCM_S16 ? 2 : 4; }
// samples delivered once the stream has been given n_native native samples since its reset (final: and has been flushed).  Additive over
// whole-frame chunks for every kind -- of the converter because a frame of 1920 native samples is a whole number of samples at all eight rates
inline int64_t out_delivered(const OutSpec& o, int64_t n_native, bool final) {
    switch (out_kind(o)) {
    case OUT_PITCHED: return pitch_out_samples(o.rate_pct, o.pitch_pct, n_native, final);
    case OUT_RATED: return tsm_out_samples(o.rate_pct, n_native, final);
    case OUT_CONVERTED: return pcm_samples_of_native(o.fmt.sample_rate, n_native);
    default: return n_native;
    }
}
// the submit rule of a request with these settings: the volume's, then the pitch's (which judges the pair and the format), else the rate's.
// nullptr = it may be queued
inline const char* out_submit_refusal(const OutSpec& o, int max_steps, int64_t cap_bytes, bool have_codec) {
    if (o.loud != 0 && !have_codec) return "the engine has no codec";   // loudness_submit_refusal (loudness.h)
    if (o.vol_db10 != 0) if (const char* why = volume_submit_refusal(o.vol_db10, have_codec)) return why;
    if (o.pitch_pct != 100) return pitch_submit_refusal(o.rate_pct, o.pitch_pct, o.fmt, max_steps, cap_bytes, have_codec);
    if (o.rate_pct != 100) return tsm_submit_refusal(o.rate_pct, o.fmt, max_steps, cap_bytes, have_codec);
    return nullptr;
}
// [EXT] loudness: where a metered stream of a pass stands and where its rows go.  pos = native samples the stream was given before this
// chunk, since its reset; rows = pinned host memory for the rows {energy, peak} the chunk completes (loud_blocks(pos, T), loudness.h)
struct LoudDst { int64_t pos = 0; double* rows = nullptr; };

// what every output stage's launch refuses, in the order all of them state it (pcm_out.h, tsm.h, volume.h, loudness.h): the group size;
// chunk_why = what the stage has against the chunk length or a missing array (nullptr: nothing), worked out by the caller from values alone;
// then stream by stream its slot, that it appears once, and why_not(g) = what the stage has against stream g's own arguments
template <class WhyNot>
inline const char* stage_launch_refusal(int G, int max_group, const char* chunk_why, const int32_t* streams, int n_streams, WhyNot why_not) {
    if (G < 1 || G > max_group) return "group size out of range";
    if (chunk_why) return chunk_why;
    for (int g = 0; g < G; g++) {
        if (streams[g] < 0 || streams[g] >= n_streams) return "stream out of range";
        for (int h = 0; h < g; h++) if (streams[h] == streams[g]) return "a stream may appear once per launch";
        if (const char* why = why_not(g)) return why;
    }
    return nullptr;
}

// [EXT] what follows the output conv for the G streams of a pass, as arithmetic on their records: which stages run, what each is handed
// per stream, and where each stream's copy comes from.  A stream is of one of four kinds (out_kind) and each stage sees the streams of the
// other stages as ones it leaves alone -- the native format, 100 percent, volume 0, unmetered; a stage nobody needs is not launched, and a
// pass of native streams is G copies of the native chunk.  A stretched or shifted stream delivers 24000 Hz.  The arrays hold max_group
// entries each and are sized once: out_route writes the first G.
struct OutRoute {
    explicit OutRoute(int max_group)
        : cf((size_t)max_group), pct((size_t)max_group), pr((size_t)max_group), pp((size_t)max_group), enc((size_t)max_group),
          vol((size_t)max_group), metered((size_t)max_group), toff((size_t)max_group), loff((size_t)max_group), src((size_t)max_group),
          src_off((size_t)max_group), bytes((size_t)max_group) {}
    bool run[4] = {false, false, false, false};   // by OutKind: run[OUT_CONVERTED], run[OUT_RATED], run[OUT_PITCHED]; run[OUT_NATIVE] = some stream is native
    bool any_volume = false, any_metered = false;
    bool all_native() const { return !run[OUT_CONVERTED] && !run[OUT_RATED] && !run[OUT_PITCHED]; }
    std::vector<q3tts_pcm_format> cf;             // the converter's formats
    std::vector<int32_t> pct, pr, pp, enc;        // the stretcher's percents; the shifter's rates and pitches; the encodings both write
    std::vector<int32_t> vol, metered;            // the volume stage's tenths of a dB; the meter's flags
    std::vector<int64_t> toff, loff;              // first byte of the stream's region in the stretcher's / shifter's lane buffer; in the meter's
    std::vector<OutKind> src;                     // whose lane buffer the stream's copy reads (OUT_NATIVE: the native chunk)
    std::vector<size_t> src_off, bytes;           // its first float there; bytes per delivered sample
};
// out == NULL is a pass of plain streams.  T = native samples per stream; region = floats per stream of the stretcher's and the shifter's
// lane buffers, loud_rows = rows per stream of the meter's.  Returns what the pass is refused for (nullptr: it may run; r is then whole)
inline const char* out_route(const OutSpec* out, int G, int64_t T, size_t region, size_t loud_rows, OutRoute* r) {
    for (bool& b : r->run) b = false;
    r->any_volume = r->any_metered = false;
    for (int g = 0; out && g < G; g++) r->run[out_kind(out[g])] = true;
    const bool prosody = r->run[OUT_RATED] || r->run[OUT_PITCHED];
    for (int g = 0; g < G; g++) {
        const OutSpec o = out ? out[g] : OutSpec();
        const OutKind k = out_kind(o);
        r->cf[g] = OutSpec().fmt; r->pct[g] = r->pr[g] = r->pp[g] = 100; r->enc[g] = Q3_PCM_F32;
        r->vol[g] = o.vol_db10; r->metered[g] = o.loud != 0;
        r->any_volume = r->any_volume || r->vol[g] != 0; r->any_metered = r->any_metered || r->metered[g];
        r->toff[g] = prosody ? (int64_t)((size_t)g * region * sizeof(float)) : 0;
        r->loff[g] = (int64_t)((size_t)g * loud_rows * 2 * sizeof(double));
        r->src[g] = k; r->src_off[g] = (size_t)g * (k >= OUT_RATED ? region : (size_t)T); r->bytes[g] = out_sample_bytes(o);
        if (k == OUT_CONVERTED) r->cf[g] = o.fmt;
        if (k < OUT_RATED) continue;
        if (o.fmt.sample_rate != Q3_PCM_NATIVE_RATE) return "a speech rate or a pitch needs the 24000 Hz output format";
        r->enc[g] = o.fmt.encoding;
        if (k == OUT_PITCHED) { r->pr[g] = o.rate_pct; r->pp[g] = o.pitch_pct; }
        else r->pct[g] = o.rate_pct;
    }
    if (prosody && 2 * (size_t)T + 3 * Q3_TSM_HOP > region) return "chunk too long for the stretcher's buffers";
    return nullptr;
}

// [EXT] the counters of the codec's output stages, as one snapshot: stream chunks the converter took and samples it made; stream chunks the
// stretcher took, synthesis frames it made, its flushes; stream chunks shifted, samples delivered, flushes, bytes of tap tables on the device;
// stream chunks the volume stage took and samples it rewrote; stream chunks the loudness meter took and blocks it completed
struct OutputStageStats {
    int64_t conv_chunks = 0, conv_samples = 0, tsm_chunks = 0, tsm_frames = 0, tsm_flushes = 0;
    int64_t pitch_chunks = 0, pitch_samples = 0, pitch_flushes = 0, pitch_table_bytes = 0, vol_chunks = 0, vol_samples = 0;
    int64_t loud_chunks = 0, loud_blocks = 0;
};

} // namespace q3
