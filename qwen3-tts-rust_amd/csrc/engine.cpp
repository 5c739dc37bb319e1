// engine.cpp -- see engine.h.  Loop structure cites /root/reference/src/tts/engine.rs line numbers.
#include "engine.h"
#include "../../include/q3tts.h"
#include <algorithm>
#include <cmath>
#include <chrono>
#include "kdev.h"
#include <functional>

namespace q3 {

static std::string quant_dir(const std::string& q) { // engine.rs:91-95 (+ this engine's extra dirs)
    if (q == "q5_k_m") return "gguf_q5_k_m";
    if (q == "q8_0") return "gguf_q8_0";
    if (q == "bf16") return "gguf_bf16";
    if (q == "f16") return "gguf_f16";
    return "gguf";
}
static double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

Engine::Engine(const EngineParams& p) : p_(p) {
    Q3_CHECK(p.max_batch >= 1 && p.max_batch <= 512, "max_batch out of range");
    Q3_HIP(hipGetDevice(&dev_));
    Q3_HIP(hipStreamCreateWithFlags(&st_, hipStreamNonBlocking));
    const std::string dir = p.model_dir + "/" + quant_dir(p.quant);
    assets_.reset(new HostAssets(dir + "/qwen3_assets.gguf"));
    const int B = p.max_batch;
    B_ = B;
    talker_.reset(new Transformer(dir + "/qwen3_tts_talker.gguf", Q3_TALKER_NCTX, std::max(256, B)));
    // Prompt chunks: 512 rows for a Q8_0 talker, whose four GEMMs take the wide forms above 256 tokens (k_gemm_q8_wide: 118.8 us per
    // layer against 176.0 us for two 256-token rounds, profiles/prefill_wide_gemm_kernel_counts.md); 256 for K-quant and float files, and under Q3_PREFILL_WIDE=0.
    // A row's result does not depend on the chunk it travels in: every kernel of the walk computes each token on its own, with the same bits.
    if (talker_->q8_uniform() && prefill_wide()) { pf_chunk_ = 512; if (talker_->max_tok() < pf_chunk_) talker_->set_max_tok(pf_chunk_); }
    predictor_.reset(new Transformer(dir + "/qwen3_tts_predictor.gguf", Q3_PRED_NCTX, 2 * B));
    if (const char* e = std::getenv("Q3_PRED_FUSED_MAX")) predictor_->set_fused_max_tokens(atoi(e)); // experiment knob
    // The predictor never holds more than 17 positions per sequence: wide steps use the single-wave attention kernel (one wave per
    // token and kv head, no workgroup barrier).  At one sequence it loses to k_attention_fused (3.24 vs 3.06 ms/frame: the serial PV
    // of both heads costs more than the barriers it removes), hence the token threshold.
    {
        int min_tok = 8;
        if (const char* e = std::getenv("Q3_SHORT_ATTN_MIN")) min_tok = atoi(e); // 0 = never
        // (the engine drives the predictor through positions 0..16 only -- 2 prompt rows + 15 code passes -- i.e. one KV page)
        predictor_->set_short_attention(min_tok, 17);
    }
    Q3_CHECK(talker_->hp().n_embd == Q3_EMBD, "talker n_embd must be 2048 (reference hard-codes 2048-wide rows)");
    dP_ = predictor_->hp().n_embd;
    Q3_CHECK(assets_->proj_out == dP_ && assets_->proj_in == Q3_EMBD, "proj shape does not match predictor n_embd");
    Q3_CHECK(assets_->n_codec == 16, "need 16 codec embedding tables");
    Q3_CHECK(predictor_->hp().n_vocab >= 15 * Q3_CODEBOOK_SIZE, "predictor vocab < 15*2048");
    // ---- device assets ----
    Q3_CHECK(dP_ % 16 == 0, "projection width must be a multiple of 16");
    {   // Wt for the load-time table projection, the blocked copy [dP/16][2048][16] for the per-frame projection of m_hidden
        const std::vector<float> wt = project_wt(assets_->proj_w, Q3_EMBD, dP_), wb = project_wblk(assets_->proj_w, Q3_EMBD, dP_);
        d_proj_wt_.alloc(wt.size()); d_proj_wt_.upload(wt.data(), wt.size());
        d_proj_wblk_.alloc(wb.size()); d_proj_wblk_.upload(wb.data(), wb.size());
    }
    d_proj_b_.alloc(dP_); d_proj_b_.upload(assets_->proj_b, dP_);
    d_tts_pad_.alloc(Q3_EMBD); d_tts_pad_.upload(assets_->tts_pad(), Q3_EMBD);
    std::vector<const float*> ptrs(16);
    std::vector<int64_t> rows(16);
    for (int q = 0; q < 16; q++) {
        const size_t n = (size_t)assets_->codec_rows[q] * Q3_EMBD;
        d_codec_tab_[q].alloc(n); d_codec_tab_[q].upload(assets_->codec[q], n);
        // pre-projected table P_q[c] = project(E_q[c]) : same arithmetic as assets_manager.rs:401-417,439-442, done once
        d_proj_tab_[q].alloc((size_t)assets_->codec_rows[q] * dP_);
        launch_project_table(st_, d_codec_tab_[q].p, assets_->codec_rows[q], d_proj_wt_.p, d_proj_b_.p, Q3_EMBD, dP_, d_proj_tab_[q].p);
        ptrs[q] = d_codec_tab_[q].p; rows[q] = assets_->codec_rows[q];
    }
    d_tab_ptrs_.alloc(16); d_tab_ptrs_.upload(ptrs.data(), 16);
    d_tab_rows_.alloc(16); d_tab_rows_.upload(rows.data(), 16);
    // Predictor passes 1..14 start from P_q[code]: layer 0's attention norm and q/k/v projection of that row depend on (q, code) alone, so
    // Q_q[c] = qkv_0(P_q[c]) is built once here, by the predictor's own norm and matmul launches, and the frame reads rows of it instead
    // of recomputing them for every slot in every pass (f32, bit for bit the in-frame result).  Q3_PRED_L0_TABLE=0 turns it off.
    pred_l0_table_ = !predictor_->ggml_mode();
    if (const char* e = std::getenv("Q3_PRED_L0_TABLE")) if (e[0] == '0') pred_l0_table_ = false;
    if (pred_l0_table_) {
        const int qs = (predictor_->hp().n_head + 2 * predictor_->hp().n_kv) * 128;
        Transformer wide(*predictor_, 256); // the predictor's weights with a workspace of 256 rows per chunk (its own may be 2)
        for (int q = 1; q < 15; q++) {
            d_qkv0_tab_[q].alloc((size_t)assets_->codec_rows[q] * qs);
            wide.build_layer0_qkv(st_, d_proj_tab_[q].p, dP_, assets_->codec_rows[q], d_qkv0_tab_[q].p);
            pred_table_bytes_ += d_qkv0_tab_[q].n * sizeof(float);
        }
        Q3_HIP(hipStreamSynchronize(st_)); // `wide` frees its workspace here
    }
    // ---- KV pools ----
    const int pages_per_seq = (p.max_prompt + p.max_steps + 1 + 63) / 64;
    kv_rows_ = (int64_t)pages_per_seq * 64;
    // talker page-table row B is the scratch sequence: idle slots of the frame graph read and write its single page, so the pages of a
    // slot that is being prefilled (or was just recycled) are never touched by the graph
    kv_t_.reset(new KvPool(talker_->hp().n_layer, talker_->hp().n_kv, B * pages_per_seq + 1, B + 1, pages_per_seq));
    kv_p_.reset(new KvPool(predictor_->hp().n_layer, predictor_->hp().n_kv, B, B, 1));
    for (int b = 0; b < B; b++) kv_p_->ensure(b, 16);
    pred_identity_pages_ = true; // sequence b owns physical page b: the predictor's attention can skip the page-table lookup
    for (int b = 0; b < B; b++) if (kv_p_->page(b, 0) != b) pred_identity_pages_ = false;
    if (const char* e = std::getenv("Q3_UNIFORM_META")) if (e[0] == '0') pred_identity_pages_ = false;
    kv_t_->ensure(B, 1);
    {
        const char* e = std::getenv("Q3_ASYNC_PREFILL");
        async_pf_ = B > 1 && !(e && e[0] == '0');
    }
    if (async_pf_) {
        talker_pf_.reset(new Transformer(*talker_, pf_chunk_)); // shares the talker's device weights; own activation workspace
        Q3_HIP(hipStreamCreateWithFlags(&st_pf_, hipStreamNonBlocking));
        Q3_HIP(hipEventCreate(&pf_done_)); Q3_HIP(hipEventCreate(&pf_e0_));
        // prompts of one admission: at most 4096 rows + routing tables + [EXT] the codes and ids of resumed prefixes (68 B a row) and the
        // codes of score rows (64 B a row) + [EXT] the fork destinations of a wave.  Every piece starts on a 64-byte boundary: six pieces a
        // chunk lose at most 6 x 63 B, over the at most 17 chunks of a 4096-row wave 6426 B, the destinations 63 B more -- inside the 64 KiB slack
        lane_alloc(pf_, talker_pf_.get(), st_pf_, pf_chunk_, true,(size_t)4096 * (Q3_EMBD * 4 + 24 + 68 + 64) + ((size_t)1 << 16) + (size_t)B * 4 +
                   (size_t)B * 2 * (sizeof(StemJob) + 4) + 256); // [EXT] prompt stems: the job tables and slot lists of a wave, four pieces
    }
    // ---- per-slot state ----
    hist_stride_ = p.max_steps * 16;
    tl_stride_ = (Q3_SAMPLE_END + 31) & ~31;
    slots_ = SlotTable(B); d_slots_.alloc(slots_.host.size()); slots_.dev = d_slots_.p; // every slot idle; sent by upload_slot_state below
    d_keys_.alloc(16 * B); d_next_key0_.alloc(B); d_hist_.alloc((size_t)B * hist_stride_);
    d_rngkey_.alloc((size_t)8 * B); d_draws_.alloc(B); d_prngkey_.alloc((size_t)8 * B); d_pdraws_.alloc(B);
    d_rngkey_.zero(); d_draws_.zero(); d_prngkey_.zero(); d_pdraws_.zero(); d_plogits_.alloc((size_t)B * Q3_CODEBOOK_SIZE);
    d_tlogits_.alloc((size_t)B * tl_stride_); d_thidden_.alloc((size_t)B * Q3_EMBD); d_pin_.alloc((size_t)2 * B * dP_);
    d_fb_.alloc((size_t)B * Q3_EMBD);
    d_hist_.zero(); d_tlogits_.zero(); d_thidden_.zero();
    // predictor routing: pass i (i = 2..15) handles position i of every slot; tables are [16][B] so any graph width can use them
    std::vector<int32_t> seq(B), slot((size_t)16 * B), pos((size_t)16 * B * 4);
    for (int b = 0; b < B; b++) {
        seq[b] = b;
        for (int i = 0; i < 16; i++) { slot[(size_t)i * B + b] = i; for (int s = 0; s < 4; s++) pos[((size_t)i * B + b) * 4 + s] = i; } // engine.rs:316-318
    }
    d_pseq_.alloc(B); d_pseq_.upload(seq.data(), B);
    d_pslot_.alloc(slot.size()); d_pslot_.upload(slot.data(), slot.size());
    d_ppos_.alloc(pos.size()); d_ppos_.upload(pos.data(), pos.size());
    h_pend_.assign(B, std::vector<int32_t>()); h_pend_off_.assign(B, 0);
    slot_req_.assign(B, nullptr);
    if (const char* e = std::getenv("Q3_SCORE_WIDTH")) score_w_ = std::max(16, std::min(64, atoi(e))); // experiment knob (DESIGN.md "Scoring given frames")
    if (async_pf_) { d_pf_logits_.alloc((size_t)B * tl_stride_); d_pf_hidden_.alloc((size_t)B * Q3_EMBD); }
    {
        std::vector<q3_u64> k0((size_t)16 * B, pack_key(-INFINITY, 0)), n0(B, pack_key(-INFINITY, 0));
        d_keys_.upload(k0.data(), k0.size()); d_next_key0_.upload(n0.data(), n0.size());
    }
    lane_alloc(ar_, talker_.get(), st_, talker_->max_tok(), false, (size_t)talker_->max_tok() * Q3_EMBD * 4 + (size_t)B * 4096 + ((size_t)1 << 20));
    Q3_HIP(hipDeviceSynchronize()); // memsets / table kernels above ran on other streams than st_
    upload_slot_state();
    if (p.load_codec) {
        Q3_CHECK(p.max_steps <= Q3TTS_CODEC_MAX_FRAMES, "max_steps above Q3TTS_CODEC_MAX_FRAMES: a request's codec stream could not be decoded to its end");
        // codec streams outnumber the slots: a retired sequence's last chunks still drain while its slot is already reused
        // up to 16 streams share one decode pass; two lanes (HIP streams + scratch) let consecutive groups overlap
        // streams per decode pass, measured on MI355X: 64 slots 617 / 607 / 600 audio-s/s at 16 / 32 / 64, 256 slots 821 / 860 / 836
        static const int group_env = [] { const char* e = std::getenv("Q3_CODEC_GROUP"); return e ? atoi(e) : 0; }();
        const int group_cap = group_env > 0 ? group_env : (B >= 128 ? 32 : 16);
        const int n_cs = B + std::min(B, 16), gmax = std::max(1, std::min(B, group_cap));
        static const int lanes_env = [] { const char* e = std::getenv("Q3_CODEC_LANES"); return e ? atoi(e) : 0; }();
        const int n_lanes = B > 1 ? (lanes_env > 0 ? std::min(lanes_env, 8) : 2) : 1;
        codec_.reset(new CodecDecoder(p.model_dir + "/onnx/q3tts_codec.gguf", n_cs, 4, n_lanes, gmax));
        worker_.reset(new CodecWorker(codec_.get(), dev_, n_lanes, n_cs, (size_t)p.max_steps * codec_->samples_per_frame()));
        Q3_HIP(hipHostMalloc((void**)&pre_tails_, (size_t)Q3TTS_MAX_PREAMBLES * Q3_PCM_HIST * sizeof(float))); // [EXT] codec preambles: 24 KB
        for (int i = Q3TTS_MAX_PREAMBLES - 1; i >= 0; i--) pre_tail_free_.push_back(i);
        for (int c = n_cs - 1; c >= 0; c--) cs_free_.push_back(c);
        decode_w_ = q3::decode_width(n_cs, B); // [EXT] decoding given frames: half of the surplus streams
    }
    Q3_HIP(hipStreamSynchronize(st_));
    Q3_HIP(hipDeviceSynchronize());
    ar_.cur.reset();
}

void Engine::lane_alloc(PrefillLane& L, Transformer* talker, hipStream_t st, int chunk, bool async, size_t arena_bytes) {
    L.talker = talker; L.st = st; L.chunk = chunk; L.async = async;
    L.d_rows.alloc((size_t)chunk * Q3_EMBD); L.d_seq.alloc(chunk); L.d_slot.alloc(chunk); L.d_pos.alloc(4 * (size_t)chunk);
    L.d_codes.alloc((size_t)chunk * 16); L.d_ids.alloc(chunk); L.d_fork_dst.alloc(B_);
    L.d_stem_jobs.alloc((size_t)2 * B_); L.d_stem_slots.alloc((size_t)2 * B_); // [EXT] prompt stems: 40 B a slot for each of restore and save
    L.cur.cap = arena_bytes;
    Q3_HIP(hipHostMalloc((void**)&L.arena, arena_bytes));
}
// The next piece of a lane's staging.  A full AR arena waits for its stream -- everything staged so far has then been consumed -- and starts
// over; the asynchronous lane's holds a whole wave and never waits.
void* Engine::stage_take(PrefillLane& L, size_t bytes) {
    size_t at = L.cur.take(bytes);
    if (at == StageCursor::NONE) {
        Q3_CHECK(!L.async, "prefill staging arena overflow");
        Q3_HIP(hipStreamSynchronize(L.st));
        L.cur.reset();
        at = L.cur.take(bytes);
        Q3_CHECK(at != StageCursor::NONE, "staging request larger than the arena");
    }
    return L.arena + at;
}
void Engine::h2d(void* dst, const void* src, size_t bytes) {
    void* p = stage_alloc(bytes);
    std::memcpy(p, src, bytes);
    Q3_HIP(hipMemcpyAsync(dst, p, bytes, hipMemcpyHostToDevice, st_));
}
void* Engine::d2h_begin(const void* src, size_t bytes) {
    void* p = stage_alloc(bytes);
    Q3_HIP(hipMemcpyAsync(p, src, bytes, hipMemcpyDeviceToHost, st_));
    return p;
}

// ---------------------------------------------------------------------------------------------------------------
struct CandSet { std::vector<float> prompt; std::vector<int32_t> trail; }; // [EXT] candidate sets: what the members of a set share
struct Engine::Req {
    // What the decoder thread sees of the request (codec_worker.h); everything else here is the scheduler's, and the thread cannot name it.
    // A decode-only one (job.decode): codes / fed hold the caller's frames from submission on; never has a slot, job.cs from admit_decodes to its fence
    CodecJob job;
    int64_t set = 0; std::shared_ptr<const CandSet> shared; // [EXT] candidate sets: the set's id (0 = a plain request) and its one prompt / trail copy
    const std::vector<int32_t>& trail_ids() const { return shared ? shared->trail : trail_own; }
    GenRequest r; std::vector<float> prompt_own; std::vector<int32_t> trail_own; bool want_pcm = false;
    std::vector<int32_t> prefix_own; // [EXT] resume: the caller's frames [n_prefix][16]; codes starts as a copy of it and fed at n_prefix
    bool closed = false;  // [EXT] open trail (r.open): closed by append_trail; trail_own and closed change under mu_ only
    int state = REQ_QUEUED; int slot = -1; int fed = 0;
    std::vector<int32_t> codes; std::vector<float> pcm;
    int64_t pcm_n = 0; // pcm_ready / pcm_n count samples of job.out's format; pcm: their bytes as the stage left them, rounded up to whole floats
    bool score = false;   // [EXT] scoring: prefix_own holds all n frames, r.n_prefix = n - 1 feedback rows; never live; codes / lp / fed appear when it is done
    // [EXT] codec preambles: the preamble the request is primed with (-1: none; kept for request_preamble after the end), whether it still
    // holds it (what its `reset` task restores is job.pre_snap / pre_tail, fixed at submit: the preamble was READY); build_pre: this is the
    // hidden decode-only request that builds that preamble (job.snapshot), and job.snap the snapshot the decoder thread enqueued at its fence
    int pre = -1; bool pre_held = false; int build_pre = -1;
    // [EXT] prompt stems: the stem the request took (-1: none; kept for request_stem after the end), whether it still holds it, the rows its
    // prefill skips and the store its wave restores them from (fixed at submit: the stem was READY); build_stem: this is the hidden wave
    // member that builds that stem -- stem_rows keeps its rows alive, build_store is what the scheduler allocated for it
    int stem = -1; bool stem_held = false; int n_skip = 0; uint16_t* stem_store = nullptr;
    int build_stem = -1; std::shared_ptr<const std::vector<float>> stem_rows; uint16_t* build_store = nullptr;
    bool offline() const { return score || build_stem >= 0; } // takes a slot for one wave and never goes live
    std::vector<float> lp; // [EXT] log-probabilities [fed][17] of a recording request (r.logprobs); grows with codes under mu_
    size_t pcm_ready = 0; // samples whose decode has completed (harvested events)
    size_t loud_ready = 0; std::vector<double> loud; // [EXT] loudness: rows whose chunk has completed; the rows [loud_ready][2] once the request has ended
    std::unique_ptr<Chunker> chunker;
    uint64_t seed = 0;
    hipEvent_t ev_admit = nullptr; bool first_seen = false;
    double t_submit = 0, t_admit = 0, t_done = 0, prefill_ms = 0, first_chunk_ms = 0;
    std::string error;
};

static void push_frames(Chunker& c, const int32_t* codes, int n) { // n frames [n][16] of int32 codes, as the chunker takes them
    for (int f = 0; f < n; f++) {
        int64_t fc[16];
        for (int q = 0; q < 16; q++) fc[q] = codes[(size_t)f * 16 + q];
        c.push(fc, 16, false);
    }
}
Engine::~Engine() {
    (void)hipSetDevice(dev_);
    try { stop_driver(); } catch (...) {}
    worker_.reset(); // joins the decoder thread
    for (auto& kv : reqs_) if (kv.second->ev_admit) (void)hipEventDestroy(kv.second->ev_admit);
    for (auto& g : graphs_) {
        if (g.second->exec) (void)hipGraphExecDestroy(g.second->exec);
        if (g.second->graph) (void)hipGraphDestroy(g.second->graph);
    }
    for (auto& s : stems_.entries()) if (s.second.payload.store) (void)hipFree(s.second.payload.store); // [EXT] prompt stems
    for (auto& d : stem_garbage_) (void)hipFree(d.first);
    if (pre_tails_) (void)hipHostFree(pre_tails_);
    if (ar_.arena) (void)hipHostFree(ar_.arena);
    if (pf_.arena) (void)hipHostFree(pf_.arena);
    if (pf_done_) (void)hipEventDestroy(pf_done_);
    if (pf_e0_) (void)hipEventDestroy(pf_e0_);
    if (st_pf_) (void)hipStreamDestroy(st_pf_);
    if (st_) (void)hipStreamDestroy(st_);
}

size_t Engine::bytes_per_frame_step(int batch, double mean_ctx) const {
    // W_T + W_P (once) + B*ctx*KV bytes/token + B*(17 rows of 8 KB)
    const auto& t = talker_->hp();
    const size_t head_t = (size_t)tl_stride_ * talker_->head_bytes_per_row();
    const size_t head_p = (size_t)15 * Q3_CODEBOOK_SIZE * predictor_->head_bytes_per_row();
    const size_t kv_per_tok = (size_t)t.n_layer * 2 * t.n_kv * 128 * 2;
    // the predictor's weights count once per frame (they stay in cache across its 15 passes, and pass A still reads layer 0's q/k/v rows), so
    // the layer-0 table takes nothing off them; it adds one f32 q/k/v row per slot in each of passes 1..14
    const size_t tab_rows = pred_l0_table_ ? (size_t)batch * 14 * (size_t)(predictor_->hp().n_head + 2 * predictor_->hp().n_kv) * 128 * 4 : 0;
    return talker_->weight_bytes() + head_t + predictor_->weight_bytes() + head_p +
           (size_t)((double)batch * mean_ctx * (double)kv_per_tok) + (size_t)batch * 17 * 8192 + tab_rows;
}

// One frame for fg.width slots (engine.rs:545-641).  code_0 of the frame is already in keys[b][0]: it was produced at the end
// of the previous frame (or of the prefill) by the talker head's argmax epilogue or by the device sampler.
// [EXT] v.pen: the talker head writes logits and k_sample applies the penalty with the history the device already has (code_0 of frames
// [0, n_frames) in d_hist_ + the current frame's key, which k_advance_keys appends only after the head); v.pred: every predictor head writes
// its 2048 logits and k_sample_pred draws the code (greedy slots take its first-max branch); v.trail: the feedback kernel reads the slot
// table's n_frames / n_trail rows, d_trail_ and the text table; v.gate: a slot that waits runs through every launch between k_stall_save and
// the gated advance and its work is discarded (q3tts_spec.h "live text append").  [EXT] v.lp: every head writes its logits -- the predictor's
// into per-step slices of d_plp_ -- every slot draws through the samplers with its own parameters, and one k_logprob_rows launch between the
// talker's sampler and the advance covers all 16 heads.  A clear flag leaves the launches as they are without it.
void Engine::record_frame(FrameGraph& fg, FrameVariant v) {
    const int B = fg.width;
    const KvCache kvt = kv_t_->view(), kvp = kv_p_->view();
    AdvanceKeysArgs a{B, di(SF_FINISHED), di(SF_NFRAMES), di(SF_MAXFRAMES), d_keys_.p, d_next_key0_.p, d_hist_.p, hist_stride_, di(SF_TSLOT), di(SF_TPOS)};
    StallArgs sg;
    if (v.gate) {
        sg.open = di(SF_OPEN); sg.n_trail = di(SF_NTRAIL); sg.hidden = d_thidden_.p; sg.draws = d_draws_.p; sg.pdraws = d_pdraws_.p;
        sg.save_hidden = d_stall_hidden_.p; sg.save_draws = d_stall_draws_.p;
        launch_stall_save(st_, a, sg);
    }
    // :565-573 predictor input = [project(m_hidden) ; project(E_0[code_0])]
    launch_project_blk(st_, d_thidden_.p, Q3_EMBD, d_proj_wblk_.p, d_proj_b_.p, Q3_EMBD, dP_, d_pin_.p, dP_, B);
    launch_gather_rows_keys(st_, d_proj_tab_[0].p, assets_->codec_rows[0], d_keys_.p, 16, dP_, d_pin_.p + (size_t)B * dP_, B);
    {   // :575-582 clear KV (= positions restart at 0) + 2-token prefill; :588-596 only slice q-1 of the 30720 logits is needed
        TokMeta tm{fg.seqA.p, fg.slotA.p, fg.posA.p};
        Transformer::Input in; in.x = d_pin_.p; in.x_stride = dP_;
        predictor_->set_same_seq_tokens(true);
        predictor_->forward(st_, in, 2 * B, tm, kvp, nullptr);
        if (v.pred || v.lp) {
            float* pl = v.lp ? d_plp_.p : d_plogits_.p;
            predictor_->head(st_, B, B, 0, Q3_CODEBOOK_SIZE, pl, Q3_CODEBOOK_SIZE);
            SampleArgs sa{pl, Q3_CODEBOOK_SIZE, Q3_CODEBOOK_SIZE, df(SF_PTEMP), di(SF_PTOPK), df(SF_PTOPP), nullptr, d_prngkey_.p, d_pdraws_.p, d_keys_.p + 1, 16};
            launch_sample_pred(st_, sa, B);
        } else {
            ArgmaxEpi am{d_keys_.p + 1, 16, nullptr, 0};
            predictor_->head(st_, B, B, 0, Q3_CODEBOOK_SIZE, nullptr, 0, &am);
        }
    }
    predictor_->set_same_seq_tokens(false);
    for (int q = 1; q < 15; q++) { // :602-610 decode project(E_q[code_q]) at pos q+1
        TokMeta tm{d_pseq_.p, d_pslot_.p + (size_t)(q + 1) * B_, d_ppos_.p + (size_t)(q + 1) * B_ * 4};
        KvCache kvq = kvp;
        if (pred_identity_pages_) { tm.uniform_pos = q + 1; kvq.page_table = nullptr; } // token t = sequence t = page t, position q+1 everywhere
        Transformer::Input in; in.x = d_proj_tab_[q].p; in.x_stride = dP_; in.idx_keys = d_keys_.p + q; in.idx_stride = 16;
        if (pred_l0_table_) { in.qkv0 = d_qkv0_tab_[q].p; in.qkv0_stride = (predictor_->hp().n_head + 2 * predictor_->hp().n_kv) * 128; }
        predictor_->forward(st_, in, B, tm, kvq, nullptr);
        if (v.pred || v.lp) {
            float* pl = v.lp ? d_plp_.p + (size_t)q * B_ * Q3_CODEBOOK_SIZE : d_plogits_.p;
            predictor_->head(st_, 0, B, q * Q3_CODEBOOK_SIZE, Q3_CODEBOOK_SIZE, pl, Q3_CODEBOOK_SIZE);
            SampleArgs sa{pl, Q3_CODEBOOK_SIZE, Q3_CODEBOOK_SIZE, df(SF_PTEMP), di(SF_PTOPK), df(SF_PTOPP), nullptr, d_prngkey_.p, d_pdraws_.p, d_keys_.p + q + 1, 16};
            launch_sample_pred(st_, sa, B);
        } else {
            ArgmaxEpi am{d_keys_.p + q + 1, 16, nullptr, 0};
            predictor_->head(st_, 0, B, q * Q3_CODEBOOK_SIZE, Q3_CODEBOOK_SIZE, nullptr, 0, &am);
        }
    }
    // :622-631 feedback ; :633-639 talker step at pos = cur_pos ; :550-555 next frame's code_0
    if (v.trail) {
        TextTrail tt; tt.n_frames = di(SF_NFRAMES); tt.n_trail = di(SF_NTRAIL); tt.ids = d_trail_.p; tt.ids_stride = p_.max_prompt;
        tt.table = d_text_.p; tt.rows = text_rows_;
        launch_feedback_keys(st_, d_tab_ptrs_.p, d_tab_rows_.p, d_keys_.p, 16, d_tts_pad_.p, d_fb_.p, B, &tt);
    } else {
        launch_feedback_keys(st_, d_tab_ptrs_.p, d_tab_rows_.p, d_keys_.p, 16, d_tts_pad_.p, d_fb_.p, B);
    }
    {
        TokMeta tm{di(SF_TSEQ), di(SF_TSLOT), di(SF_TPOS)};
        Transformer::Input in; in.x = d_fb_.p; in.x_stride = Q3_EMBD;
        talker_->set_same_seq_tokens(false);
        talker_->forward(st_, in, B, tm, kvt, nullptr);
        if (v.sampled || v.pen || v.lp) { // llama/mod.rs:666-776 on device; greedy slots of a mixed batch take the kernel's T<=0 branch
            talker_->head(st_, 0, B, 0, tl_stride_, d_tlogits_.p, tl_stride_, nullptr, -1, d_thidden_.p);
            SampleArgs sa{d_tlogits_.p, tl_stride_, Q3_SAMPLE_END, df(SF_TEMP), di(SF_TOPK), df(SF_TOPP), di(SF_MASKEOS), d_rngkey_.p, d_draws_.p, d_next_key0_.p, 1};
            if (v.pen) { sa.penalty = df(SF_PEN); sa.hist = d_hist_.p; sa.hist_stride = hist_stride_; sa.hist_len = di(SF_NFRAMES); sa.cur_key = d_keys_.p; sa.cur_stride = 16; }
            launch_sample(st_, sa, B);
            if (v.lp) { // columns 1..15 of this frame's row, columns 0 and 16 of the next frame's: before k_advance_keys moves n_frames
                LogprobArgs la;
                la.p.logits = d_plp_.p; la.p.stride = Q3_CODEBOOK_SIZE; la.p.head_stride = (size_t)B_ * Q3_CODEBOOK_SIZE; la.p.n = Q3_CODEBOOK_SIZE;
                la.p.key = d_keys_.p + 1; la.p.key_stride = 16; la.p.col = 1; la.n_first = 15;
                la.t.logits = d_tlogits_.p; la.t.stride = tl_stride_; la.t.n = Q3_SAMPLE_END; la.t.key = d_next_key0_.p; la.t.key_stride = 1;
                la.t.extra_idx = Q3_CODEC_EOS; la.t.col = 0; la.t.col_extra = Q3_LOGPROB_COLS - 1; la.t.row_ahead = 1;
                la.out = d_lp_.p; la.out_stride = Q3_LOGPROB_COLS; la.out_rows = lp_rows_;
                la.n_frames = di(SF_NFRAMES); la.finished = di(SF_FINISHED); la.max_frames = di(SF_MAXFRAMES); la.open = di(SF_OPEN);
                la.n_trail = di(SF_NTRAIL); la.record = d_lp_rec_.p;
                launch_logprob_rows(st_, la, B);
            }
        } else {
            ArgmaxEpi am{d_next_key0_.p, 1, di(SF_MASKEOS), 0};
            talker_->head(st_, 0, B, 0, tl_stride_, nullptr, 0, &am, Q3_SAMPLE_END, d_thidden_.p);
        }
    }
    if (v.gate) launch_advance_keys_gated(st_, a, sg);
    else launch_advance_keys(st_, a);
    Q3_LAUNCH_CHECK();
}

std::mutex& capture_mutex() { static std::mutex mu; return mu; }

Engine::FrameGraph& Engine::frame_graph(int width, FrameVariant v, bool capture) {
    std::unique_ptr<FrameGraph>& slot = graphs_[v.key(width)];
    // one graph construction at a time per process: engines of a multi-device group (or several engines on one device) build their frame
    // graphs from different threads; the synchronous allocations / uploads below and concurrent thread-local captures were seen to
    // invalidate another thread's capture on ROCm 7.2 ("operation failed due to a previous error during capture")
    std::unique_lock<std::mutex> build_lock(capture_mutex(), std::defer_lock);
    if (!slot || (capture && !slot->exec)) build_lock.lock();
    if (!slot) {
        slot.reset(new FrameGraph());
        FrameGraph& fg = *slot;
        fg.width = width;
        const int B = width; // pass A = positions 0 and 1 of every slot: 2B tokens, slot b's pair stays in its own sequence
        std::vector<int32_t> seqA(2 * B), slotA(2 * B), posA((size_t)2 * B * 4);
        for (int b = 0; b < B; b++) {
            seqA[b] = b; seqA[B + b] = b; slotA[b] = 0; slotA[B + b] = 1;
            for (int s = 0; s < 4; s++) { posA[(size_t)b * 4 + s] = 0; posA[((size_t)B + b) * 4 + s] = 1; }
        }
        fg.seqA.alloc(2 * B); fg.seqA.upload(seqA.data(), 2 * B);
        fg.slotA.alloc(2 * B); fg.slotA.upload(slotA.data(), 2 * B);
        fg.posA.alloc(posA.size()); fg.posA.upload(posA.data(), posA.size());
    }
    FrameGraph& fg = *slot;
    if (capture && !fg.exec) {
        (void)hipGetLastError();
        Q3_HIP(hipStreamBeginCapture(st_, hipStreamCaptureModeThreadLocal));
        try { record_frame(fg, v); }
        catch (...) { hipGraph_t dead = nullptr; (void)hipStreamEndCapture(st_, &dead); if (dead) (void)hipGraphDestroy(dead); throw; }
        Q3_HIP(hipStreamEndCapture(st_, &fg.graph));
        Q3_HIP(hipGraphInstantiate(&fg.exec, fg.graph, nullptr, nullptr, 0));
    }
    return fg;
}

void Engine::upload_slot_state() {
    slots_.route();
    h2d(slots_.dev, slots_.host.data(), slots_.host.size() * 4);
    slot_dirty_ = false;
}

// Prefill (engine.rs:455-462) of one admission wave on lane L: all prompts as ONE token stream, chunked by the lane's width; tokens of
// different sequences share a launch (per-token seq/slot/pos routing); each sequence's last token gets the head -- code_0 of its first
// frame (:550-555) + the hidden row the predictor starts from (:565-566) -- as the lane takes it: head_live or head_staged.  Every chunk
// is enqueued on L.st; only the AR lane's staging can make the host wait (stage_take).
void Engine::prefill_wave(PrefillLane& L, const std::vector<Req*>& wave, bool sampled) {
    size_t total = 0;
    std::vector<PromptRef> refs;
    std::vector<Req*> batch; std::vector<std::vector<Req*>> rest; // [EXT] candidate sets: a set's later members add no rows
    split_sets(wave, batch, rest);
    for (Req* r : batch) { // [EXT] prompt stems: the rows a stem covers are restored below and neither staged nor prefilled
        total += (size_t)admission_rows(r->r.n_prompt, r->n_skip, r->r.n_prefix);
        refs.push_back({r->r.prompt, r->r.n_prompt, r->slot, r->r.n_prefix, r->n_skip});
    }
    PrefillCursor cur; std::vector<std::pair<int, int>> lasts; std::vector<FbRun> fb;
    std::vector<char> is_score; // [EXT] scoring: which requests of the wave only want their rows scored
    for (Req* r : batch) is_score.push_back(r->score);
    restore_stems(L, batch); // behind the page-table rows KvPool::ensure put on this stream, in front of the first chunk
    L.talker->set_same_seq_tokens(true);
    for (size_t done = 0; done < total;) {
        const size_t n_max = std::min<size_t>(total - done, (size_t)L.chunk);
        float* stage = (float*)stage_take(L, n_max * Q3_EMBD * 4);
        int32_t* hc = (int32_t*)stage_take(L, n_max * 68); // [EXT] resume: codes [rows][16] and ids [rows] of the chunk's feedback rows
        int32_t* hs = (int32_t*)stage_take(L, n_max * 64); // [EXT] scoring: codes [rows][16] of the chunk's score rows
        int32_t* seq = (int32_t*)stage_take(L, n_max * 4); int32_t* slot = (int32_t*)stage_take(L, n_max * 4); int32_t* pos = (int32_t*)stage_take(L, n_max * 16);
        const PrefillCursor before = cur;
        const int n = pack_prefill_chunk(refs, cur, (int)n_max, stage, seq, slot, pos, lasts, &fb);
        for (auto& run : staged_runs(n, fb))
            Q3_HIP(hipMemcpyAsync(L.d_rows.p + (size_t)run.first * Q3_EMBD, stage + (size_t)run.first * Q3_EMBD, (size_t)run.second * Q3_EMBD * 4, hipMemcpyHostToDevice, L.st));
        feedback_rows(L.st, batch, fb, hc, L.d_codes.p, L.d_ids.p, L.d_rows.p);
        Q3_HIP(hipMemcpyAsync(L.d_seq.p, seq, (size_t)n * 4, hipMemcpyHostToDevice, L.st));
        Q3_HIP(hipMemcpyAsync(L.d_slot.p, slot, (size_t)n * 4, hipMemcpyHostToDevice, L.st));
        Q3_HIP(hipMemcpyAsync(L.d_pos.p, pos, (size_t)n * 16, hipMemcpyHostToDevice, L.st));
        TokMeta tm{L.d_seq.p, L.d_slot.p, L.d_pos.p};
        Transformer::Input in; in.x = L.d_rows.p; in.x_stride = Q3_EMBD;
        L.talker->forward(L.st, in, n, tm, kv_t_->view(), nullptr);
        score_chunk(L.st, *L.talker, batch, score_head_runs(refs, is_score, before, n), hs);
        for (auto& lb : lasts) {
            if (batch[lb.first]->offline()) continue; // no first frame to draw
            if (L.async) head_staged(batch[lb.first], rest[lb.first], lb.second);
            else head_live(batch[lb.first], rest[lb.first], lb.second, sampled);
        }
        done += (size_t)n;
    }
    save_stems(L, batch); // [EXT] prompt stems: the pages of the wave's builds go into their stores, behind the last chunk
    if (batch.size() < wave.size()) fork_sets(L.st, batch, rest, (int32_t*)stage_take(L, (size_t)B_ * 4), L.d_fork_dst.p); // a wave without a set stages nothing more
}
SampleArgs Engine::first_head_args(const float* logits_row, int b) const {
    return SampleArgs{logits_row, tl_stride_, Q3_SAMPLE_END, df(SF_TEMP) + b, di(SF_TOPK) + b, df(SF_TOPP) + b,
                      di(SF_MASKEOS) + b, d_rngkey_.p + (size_t)b * 8, d_draws_.p + b, d_keys_.p + (size_t)b * 16, 16};
}
// In line: the head of a request's last prompt token `tok` draws code_0 straight into the live arrays, once per member of its set ([EXT]
// candidate sets: every member's slot draws from the set's last prompt token).  The argmax epilogue, unless something needs the logits.
void Engine::head_live(Req* lead, const std::vector<Req*>& rest, int tok, bool sampled) {
    const bool hist = resumed_penalised(lead->r); // [EXT] resume: the first head already sees a history, greedy slots included
    const bool rec = lead->r.logprobs;            // [EXT] log-probabilities: the first frame's talker columns need the logits
    for (size_t m = 0; m <= rest.size(); m++) {
        const int sb = m == 0 ? lead->slot : rest[m - 1]->slot;
        float* logits = d_tlogits_.p + (size_t)sb * tl_stride_; float* hidden = d_thidden_.p + (size_t)sb * Q3_EMBD;
        if (sampled || hist || rec) {
            talker_->head(st_, tok, 1, 0, tl_stride_, logits, tl_stride_, nullptr, -1, hidden);
            SampleArgs sa = first_head_args(logits, sb);
            if (hist) head_history(sa, sb);
            launch_sample(st_, sa, 1);
            if (rec) first_head_logprobs(st_, logits, sb, lead->r.n_prefix);
        } else {
            ArgmaxEpi am{d_keys_.p + (size_t)sb * 16, 16, di(SF_MASKEOS) + sb, 0};
            talker_->head(st_, tok, 1, 0, tl_stride_, nullptr, 0, &am, Q3_SAMPLE_END, hidden);
        }
    }
}
// Asynchronously: logits + hidden of the LAST prompt token (engine.rs:550-554,565-566) wait in the staging rows of the request's slot;
// code_0 is drawn at activation.  [EXT] candidate sets: the staged rows reach every member; activate() stays per slot.
void Engine::head_staged(Req* lead, const std::vector<Req*>& rest, int tok) {
    float* logits = d_pf_logits_.p + (size_t)lead->slot * tl_stride_; float* hidden = d_pf_hidden_.p + (size_t)lead->slot * Q3_EMBD;
    talker_pf_->head(st_pf_, tok, 1, 0, tl_stride_, logits, tl_stride_, nullptr, -1, hidden);
    for (Req* m : rest) {
        Q3_HIP(hipMemcpyAsync(d_pf_logits_.p + (size_t)m->slot * tl_stride_, logits, (size_t)tl_stride_ * 4, hipMemcpyDeviceToDevice, st_pf_));
        Q3_HIP(hipMemcpyAsync(d_pf_hidden_.p + (size_t)m->slot * Q3_EMBD, hidden, (size_t)Q3_EMBD * 4, hipMemcpyDeviceToDevice, st_pf_));
    }
}

// [EXT] candidate sets.  The members of a set stand together in a wave (they were queued together and admitted whole); the first is prefilled.
void Engine::split_sets(const std::vector<Req*>& batch, std::vector<Req*>& lead, std::vector<std::vector<Req*>>& rest) {
    for (Req* r : batch) {
        if (r->set != 0 && !lead.empty() && lead.back()->set == r->set) rest.back().push_back(r);
        else { lead.push_back(r); rest.emplace_back(); }
    }
}
// One k_kv_fork launch per set behind the wave's last chunk, on the chunks' stream: the pages that hold the prompt go from the prefilled
// member's slot into the others'.  The page-table rows of all of them were uploaded on this stream before the first chunk.
void Engine::fork_sets(hipStream_t st, const std::vector<Req*>& lead, const std::vector<std::vector<Req*>>& rest, int32_t* h_dst, int32_t* d_dst) {
    int at = 0;
    for (size_t i = 0; i < lead.size(); i++) {
        const int n_dst = (int)rest[i].size(), n_pages = (lead[i]->r.n_prompt + 63) / 64;
        if (n_dst == 0) continue;
        Q3_CHECK(at + n_dst <= B_, "fork destinations beyond the slots");
        for (int d = 0; d < n_dst; d++) h_dst[at + d] = rest[i][d]->slot;
        Q3_HIP(hipMemcpyAsync(d_dst + at, h_dst + at, (size_t)n_dst * 4, hipMemcpyHostToDevice, st));
        launch_kv_fork(st, kv_t_->view(), lead[i]->slot, d_dst + at, n_dst, n_pages);
        cand_rows_saved_ += (int64_t)n_dst * lead[i]->r.n_prompt; cand_pages_ += (int64_t)n_dst * n_pages;
        at += n_dst;
    }
    if (at > 0) Q3_LAUNCH_CHECK();
}

// [EXT] prompt stems.  One k_kv_stem launch restores every stem the wave's prefilled members took: a job per stem, its slots listed together
// (a candidate set's first member is restored; fork_sets copies its pages to the others behind the last chunk).  The job table and the slot
// list go up through the lane's staging.  A wave without a stem stages and launches nothing.
void Engine::restore_stems(PrefillLane& L, const std::vector<Req*>& lead) {
    std::vector<Req*> takers;
    for (Req* r : lead) if (r->n_skip > 0) takers.push_back(r);
    if (takers.empty()) return;
    std::stable_sort(takers.begin(), takers.end(), [](const Req* a, const Req* b) { return a->stem < b->stem; });
    Q3_CHECK((int)takers.size() <= B_, "stem restores beyond the slots");
    StemJob* jobs = (StemJob*)stage_take(L, takers.size() * sizeof(StemJob));
    int32_t* slots = (int32_t*)stage_take(L, takers.size() * 4);
    const size_t plane = kv_t_->view().page_stride();
    int n_jobs = 0, max_pages = 0;
    for (size_t i = 0; i < takers.size(); i++) {
        Req* r = takers[i];
        const int np = stem_pages(r->n_skip);
        slots[i] = r->slot;
        if (i == 0 || takers[i - 1]->stem != r->stem) {
            jobs[n_jobs++] = StemJob{r->stem_store, r->stem_store + (size_t)np * plane, np, (int32_t)i, 0, 0};
            max_pages = std::max(max_pages, np);
        }
        jobs[n_jobs - 1].n_dst++;
        stem_restores_++; stem_rows_ += r->n_skip; stem_pages_ += np;
    }
    Q3_HIP(hipMemcpyAsync(L.d_stem_jobs.p, jobs, (size_t)n_jobs * sizeof(StemJob), hipMemcpyHostToDevice, L.st));
    Q3_HIP(hipMemcpyAsync(L.d_stem_slots.p, slots, takers.size() * 4, hipMemcpyHostToDevice, L.st));
    launch_kv_stem(L.st, kv_t_->view(), L.d_stem_jobs.p, n_jobs, max_pages, L.d_stem_slots.p, false);
    Q3_LAUNCH_CHECK();
}
// One k_kv_stem launch saves the pages of every build of the wave into its store: a job per build, one slot each.  The save half of the
// lane's tables starts at entry B.
void Engine::save_stems(PrefillLane& L, const std::vector<Req*>& lead) {
    std::vector<Req*> builds;
    for (Req* r : lead) if (r->build_stem >= 0) builds.push_back(r);
    if (builds.empty()) return;
    StemJob* jobs = (StemJob*)stage_take(L, builds.size() * sizeof(StemJob));
    int32_t* slots = (int32_t*)stage_take(L, builds.size() * 4);
    const size_t plane = kv_t_->view().page_stride();
    int max_pages = 0;
    for (size_t i = 0; i < builds.size(); i++) {
        Req* r = builds[i];
        const int np = stem_pages(r->r.n_prompt);
        Q3_CHECK(r->build_store, "a stem build without a store");
        slots[i] = r->slot;
        jobs[i] = StemJob{r->build_store, r->build_store + (size_t)np * plane, np, (int32_t)i, 1, 0};
        max_pages = std::max(max_pages, np);
    }
    Q3_HIP(hipMemcpyAsync(L.d_stem_jobs.p + B_, jobs, builds.size() * sizeof(StemJob), hipMemcpyHostToDevice, L.st));
    Q3_HIP(hipMemcpyAsync(L.d_stem_slots.p + B_, slots, builds.size() * 4, hipMemcpyHostToDevice, L.st));
    launch_kv_stem(L.st, kv_t_->view(), L.d_stem_jobs.p + B_, (int)builds.size(), max_pages, L.d_stem_slots.p + B_, true);
    Q3_LAUNCH_CHECK();
}
// The stores of a wave's builds: one allocation per stem, K plane pages then V plane pages, made by the scheduler thread under
// capture_mutex() like every allocation after construction.  A failed allocation fails the wave as any scheduler error does.
void Engine::alloc_stem_stores(const std::vector<Req*>& wave) {
    bool any = false;
    for (Req* r : wave) any = any || r->build_stem >= 0;
    if (!any) return;
    std::lock_guard<std::mutex> cap(capture_mutex());
    for (Req* r : wave) {
        if (r->build_stem < 0) continue;
        const int64_t bytes = stem_store_bytes(r->r.n_prompt, talker_->hp().n_layer, talker_->hp().n_kv);
        Q3_HIP(hipMalloc((void**)&r->build_store, (size_t)bytes));
        stem_bytes_ += bytes;
        std::lock_guard<std::mutex> lk(mu_);
        if (auto* s = stems_.find(r->build_stem)) { s->payload.store = r->build_store; s->payload.bytes = bytes; }
        else stem_garbage_.emplace_back(r->build_store, bytes); // cannot happen: a building stem is never recycled
    }
}
// Scheduler thread, the wave's prefill and saves complete: the stems are READY, the slots and their KV pages free again, the hidden requests gone.
void Engine::finish_builds(const std::vector<Req*>& builds) {
    for (Req* r : builds) {
        const int b = r->slot;
        kv_t_->release(b);
        std::lock_guard<std::mutex> lk(mu_);
        slot_req_[b] = nullptr; r->slot = -1;
        if (stems_.find(r->build_stem)) stem_built_++;
        recycled(stems_.finish(r->build_stem, true)); // recycles at once when it was released while it built
        end_build(r);
    }
}
// Scheduler thread: the stores of stems nobody holds any more.  hipFree waits for the device, so every restore has long completed.
void Engine::free_stem_stores() {
    std::vector<std::pair<uint16_t*, int64_t>> dead;
    { std::lock_guard<std::mutex> lk(mu_); dead.swap(stem_garbage_); }
    if (dead.empty()) return;
    std::lock_guard<std::mutex> cap(capture_mutex());
    for (auto& d : dead) { (void)hipFree(d.first); stem_bytes_ -= d.second; }
}

// [EXT] resume: the feedback rows of one prefill chunk.  The codes (64 B a frame) and trailing ids of every run go up through hc (pinned, not
// reused before the stream has consumed it) and k_feedback_codes writes the rows into the chunk's input buffer, behind the staged rows' copies.
void Engine::feedback_rows(hipStream_t st, const std::vector<Req*>& batch, const std::vector<FbRun>& fb, int32_t* hc, int32_t* d_codes, int32_t* d_ids,
                           float* d_rows) {
    if (fb.empty()) return;
    int rows = 0;
    for (const FbRun& f : fb) rows += f.n;
    int32_t* hi = hc + (size_t)rows * 16;
    std::vector<int> n_ids(fb.size());
    int at = 0;
    for (size_t i = 0; i < fb.size(); i++) {
        const FbRun& f = fb[i]; Req* r = batch[f.req];
        std::copy(r->prefix_own.begin() + (size_t)f.frame * 16, r->prefix_own.begin() + (size_t)(f.frame + f.n) * 16, hc + (size_t)at * 16);
        std::lock_guard<std::mutex> lk(mu_); // an open trail grows under mu_; the ids of the prefix frames were there at submit
        n_ids[i] = std::max(0, std::min(f.n, (int)r->trail_own.size() - f.frame));
        std::copy(r->trail_own.begin() + std::min<size_t>(f.frame, r->trail_own.size()), r->trail_own.begin() + std::min<size_t>(f.frame, r->trail_own.size()) + n_ids[i], hi + at);
        at += f.n;
    }
    Q3_HIP(hipMemcpyAsync(d_codes, hc, (size_t)rows * 64, hipMemcpyHostToDevice, st));
    Q3_HIP(hipMemcpyAsync(d_ids, hi, (size_t)rows * 4, hipMemcpyHostToDevice, st));
    at = 0;
    for (size_t i = 0; i < fb.size(); i++) {
        const FbRun& f = fb[i];
        FeedbackIds fi; fi.ids = d_ids + at; fi.n_ids = n_ids[i]; fi.table = d_text_.p; fi.rows = text_rows_;
        launch_feedback_codes(st, d_tab_ptrs_.p, d_tab_rows_.p, d_codes + (size_t)at * 16, d_tts_pad_.p, d_rows + (size_t)f.row * Q3_EMBD, f.n, &fi);
        at += f.n;
    }
}
// the sampler arguments of a resumed slot's first head: the penalty with the history the prefix seeded (go_live), no current frame
void Engine::head_history(SampleArgs& sa, int b) const {
    sa.penalty = df(SF_PEN) + b; sa.hist = d_hist_.p + (size_t)b * hist_stride_; sa.hist_stride = hist_stride_; sa.hist_len = di(SF_NFRAMES) + b;
    sa.cur_key = nullptr; sa.cur_stride = 0;
}
void Engine::first_head_logprobs(hipStream_t st, const float* logits_row, int b, int row) {
    LogprobArgs la;
    la.t.logits = logits_row; la.t.stride = tl_stride_; la.t.n = Q3_SAMPLE_END; la.t.key = d_keys_.p + (size_t)b * 16; la.t.key_stride = 16;
    la.t.extra_idx = Q3_CODEC_EOS; la.t.col = 0; la.t.col_extra = Q3_LOGPROB_COLS - 1;
    la.out = d_lp_.p + ((size_t)b * lp_rows_ + row) * Q3_LOGPROB_COLS; la.out_stride = Q3_LOGPROB_COLS;
    launch_logprob_rows(st, la, 1);
}

// collects finished codec work: PCM watermark per request, first-chunk latency, request completion
void Engine::harvest(bool block) {
    for (;;) {
        CodecWorker::Completion c;
        if (!worker_ || !worker_->poll_completion(block, &c)) return;
        std::lock_guard<std::mutex> lk(mu_);
        Req* r = &req(c.job->id);
        r->pcm_ready = c.pcm_after; r->loud_ready = c.loud_after;
        if (!r->first_seen && c.pcm_after > 0) {
            float ms = 0;
            Q3_HIP(hipEventElapsedTime(&ms, r->ev_admit, c.ev));
            r->first_chunk_ms = (r->t_admit - r->t_submit) + ms;
            r->first_seen = true;
        }
        (void)hipEventDestroy(c.ev);
        if (c.fence) {
            r->pcm_n = (int64_t)c.pcm_after; // the bytes as they are: whole floats for f32, (n + 1) / 2 of them for s16
            r->pcm.assign(worker_->staging(r->job.cs), worker_->staging(r->job.cs) + (c.pcm_after * r->job.sample_bytes() + 3) / 4);
            if (c.loud_after > 0) r->loud.assign(worker_->loud_staging(r->job.cs), worker_->loud_staging(r->job.cs) + c.loud_after * 2); // [EXT] loudness
            cs_free_.push_back(r->job.cs);
            r->job.cs = -1;
            r->state = fenced_state(r->job.cancel); r->t_done = now_ms();
            n_draining_--;
            if (r->job.decode) n_decoding_--;
            drop_held(r); // [EXT] codec preambles, prompt stems: the restores this request and its wave enqueued have completed
            if (r->build_pre >= 0) { // the preamble is built: its snapshot is on the device, its last native samples become its tail
                bool ok = false;
                if (auto* e = pres_.find(r->build_pre)) {
                    PreHeld& p = e->payload;
                    p.snap = r->job.snap;
                    ok = p.snap >= 0 && r->pcm.size() >= (size_t)Q3_PCM_HIST;
                    if (ok) { std::copy(r->pcm.end() - Q3_PCM_HIST, r->pcm.end(), pre_tails_ + (size_t)p.tail * Q3_PCM_HIST); pre_built_++; }
                }
                recycled(pres_.finish(r->build_pre, ok)); // recycles at once when it was released while it built
                end_build(r);
            } else cv_.notify_all();
        }
        block = false; // after one blocking wait, drain whatever else is ready
    }
}

void Engine::validate(const GenRequest& g) const {
    Q3_CHECK(g.prompt && g.n_prompt >= 1 && g.n_prompt <= p_.max_prompt, "prompt length out of range");
    Q3_CHECK(g.max_steps >= 0 && g.max_steps <= p_.max_steps, "max_steps out of range");
    const GenOptions& o = g.opts;
    Q3_CHECK(std::isfinite(o.repetition_penalty) && o.repetition_penalty > 0.0f, "repetition_penalty must be finite and > 0");
    Q3_CHECK(o.predictor_top_k >= 0, "predictor_top_k must be >= 0");
    Q3_CHECK(o.predictor_top_p > 0.0f && o.predictor_top_p <= 1.0f, "predictor_top_p must be in (0, 1]");
    Q3_CHECK(!(talker_->ggml_mode() && (o.penalised() || o.pred_sampled())),
             "repetition_penalty / predictor sampling are not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)");
    Q3_CHECK(g.n_trail >= 0 && g.n_trail <= p_.max_prompt, "n_trail must be in [0, max_prompt]");
    Q3_CHECK(g.n_trail == 0 || g.trail, "trailing ids missing");
    Q3_CHECK(!(talker_->ggml_mode() && (g.n_trail > 0 || g.open)),
             "trailing text ids are not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)");
    // [EXT] resume: the pure rule of sched_logic.h, before anything is queued
    if (const char* why = resume_refusal(g.n_prompt, g.max_steps, g.prefix, g.n_prefix, g.open, g.n_trail, kv_rows_)) throw Error(why);
    Q3_CHECK(!g.logprobs || lp_ready_.load(), "the request records log-probabilities but recording was never enabled on this engine");
    Q3_CHECK(!(talker_->ggml_mode() && g.n_prefix > 0),
             "resuming from a prefix is not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)");
}

// The streaming-text state goes to the device on first use only: the real text table is 151936 x 2048 f32 (~1.24 GB).  Called from
// submitting threads; the synchronous allocations and uploads hold capture_mutex() so they never land inside another thread's capture.
void Engine::ensure_text_stream() {
    std::lock_guard<std::mutex> lk(text_mu_);
    if (text_ready_) return;
    std::lock_guard<std::mutex> cap(capture_mutex());
    int prev = 0;
    Q3_HIP(hipGetDevice(&prev));
    Q3_HIP(hipSetDevice(dev_));
    try {
        const HostAssets& a = *assets_;
        text_rows_ = a.text_table ? a.text_rows : 0;
        d_text_.alloc((size_t)std::max<int64_t>(text_rows_, 1) * Q3_EMBD);
        if (text_rows_ > 0) d_text_.upload(a.text_table, (size_t)text_rows_ * Q3_EMBD);
        d_trail_.alloc((size_t)B_ * p_.max_prompt); d_trail_.zero();
        d_stall_hidden_.alloc((size_t)B_ * Q3_EMBD); d_stall_draws_.alloc((size_t)2 * B_);
        Q3_HIP(hipStreamSynchronize(nullptr)); // the memsets ran on the null stream; the engine's streams do not wait for it
    } catch (...) { (void)hipSetDevice(prev); throw; }
    Q3_HIP(hipSetDevice(prev));
    text_ready_ = true;
}

// [EXT] token log-probabilities: like the streaming-text state, the buffers go to the device on first use only (the predictor logits
// slices are 15 x B x 8 KB); same locking, so the synchronous allocations never land inside another thread's capture.
void Engine::set_logprobs(bool on) {
    if (on) {
        Q3_CHECK(!talker_->ggml_mode(),
                 "token log-probabilities are not available with Q3_SPEC=ggml (the ggml-arithmetic mode serves the reference's decoding only)");
        std::lock_guard<std::mutex> lk(lp_mu_);
        if (!lp_ready_.load()) {
            std::lock_guard<std::mutex> cap(capture_mutex());
            int prev = 0;
            Q3_HIP(hipGetDevice(&prev));
            Q3_HIP(hipSetDevice(dev_));
            try {
                lp_rows_ = p_.max_steps + 1;
                d_lp_.alloc((size_t)B_ * lp_rows_ * Q3_LOGPROB_COLS);
                d_plp_.alloc((size_t)15 * B_ * Q3_CODEBOOK_SIZE);
                d_lp_rec_.alloc(B_); d_lp_rec_.zero();
                Q3_HIP(hipStreamSynchronize(nullptr)); // the memset ran on the null stream; the engine's streams do not wait for it
            } catch (...) { (void)hipSetDevice(prev); throw; }
            Q3_HIP(hipSetDevice(prev));
            lp_ready_ = true;
        }
    }
    lp_on_ = on;
}

Engine::Req& Engine::req(int64_t id) {
    auto it = reqs_.find(id);
    Q3_CHECK(it != reqs_.end(), "unknown request id");
    return *it->second;
}
int64_t Engine::enqueue(std::unique_ptr<Req> r, std::deque<Req*>& queue) {
    const int64_t id = r->job.id = next_id_++;
    queue.push_back(r.get());
    reqs_[id] = std::move(r);
    wake_++;
    cv_.notify_all();
    return id;
}

int64_t Engine::submit(const GenRequest& g, bool want_pcm, bool copy_prompt, bool may_record) {
    validate(g);
    if (g.n_trail > 0 || g.open) ensure_text_stream();
    std::unique_ptr<Req> r(new Req());
    r->r = g;
    r->r.logprobs = may_record && (g.logprobs || lp_on_.load()); // [EXT] the engine's flag, read once per request
    if (copy_prompt) { r->prompt_own.assign(g.prompt, g.prompt + (size_t)g.n_prompt * Q3_EMBD); r->r.prompt = r->prompt_own.data(); }
    if (g.open) r->trail_own.reserve((size_t)p_.max_prompt);
    r->trail_own.assign(g.trail, g.trail + g.n_trail);
    r->r.trail = r->trail_own.data();
    if (g.n_prefix > 0) { // [EXT] resume: the request starts with the caller's frames
        r->prefix_own.assign(g.prefix, g.prefix + (size_t)g.n_prefix * 16);
        r->codes = r->prefix_own; r->fed = g.n_prefix;
        if (r->r.logprobs) r->lp.assign((size_t)g.n_prefix * Q3_LOGPROB_COLS, Q3_LOGPROB_NONE); // nothing computed them
    }
    r->r.prefix = r->prefix_own.data();
    r->want_pcm = want_pcm && codec_;
    if (r->want_pcm && may_record) take_out(r.get(), g.max_steps); // [EXT] the engine's output settings, read once per request; throws before anything is queued; a blocking batch is native
    r->t_submit = now_ms();
    r->seed = g.sampler.has_seed ? g.sampler.seed
                                 : (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::system_clock::now().time_since_epoch()).count(); // :473-478
    if (may_record) { Req* one = r.get(); stem_match(&one, 1, g.stem); } // [EXT] prompt stems: the take rule, once per request; never a blocking batch
    std::lock_guard<std::mutex> lk(mu_);
    // [EXT] codec preambles: the engine-level setting or the caller's (a voice's), read once per request; a blocking batch is never primed
    const int pid = preamble_of_request(r->want_pcm && may_record, g.preamble, pres_.setting);
    if (pid >= 0) { try { pre_attach(r.get(), pid); } catch (...) { drop_held(r.get()); throw; } } // throws before anything is queued
    return enqueue(std::move(r), pending_);
}

// [EXT] candidate sets: n consecutive queue entries that share one copy of the prompt and trail; each is what submit() would queue with its seed.
void Engine::submit_candidates(const GenRequest& g0, bool want_pcm, const uint64_t* seeds, int n, int64_t* req_ids) {
    if (const char* why = candidates_refusal(n, B_, seeds, req_ids, g0.trail, g0.n_trail, p_.max_prompt, talker_->ggml_mode())) throw Error(why);
    GenRequest g = g0;
    g.open = false; g.prefix = nullptr; g.n_prefix = 0; // not in a set
    g.sampler.has_seed = true; g.sampler.seed = seeds[0];
    if (n == 1) { req_ids[0] = submit(g, want_pcm, true); return; }
    validate(g);
    if (g.n_trail > 0) ensure_text_stream();
    std::shared_ptr<CandSet> sh(new CandSet());
    sh->prompt.assign(g.prompt, g.prompt + (size_t)g.n_prompt * Q3_EMBD);
    sh->trail.assign(g.trail, g.trail + g.n_trail);
    g.prompt = sh->prompt.data(); g.trail = sh->trail.data();
    g.logprobs = g.logprobs || lp_on_.load(); // the engine's flag, read once per set
    std::vector<std::unique_ptr<Req>> rs;
    const double t = now_ms();
    for (int i = 0; i < n; i++) {
        std::unique_ptr<Req> r(new Req());
        r->r = g; r->r.sampler.seed = seeds[i]; r->seed = seeds[i];
        r->r.prefix = r->prefix_own.data();
        r->shared = sh;
        r->want_pcm = want_pcm && codec_;
        if (r->want_pcm) take_out(r.get(), g.max_steps, i == 0 ? nullptr : &rs[0]->job.out); // [EXT] the output settings, read once per set
        r->t_submit = t;
        rs.push_back(std::move(r));
    }
    {   // [EXT] prompt stems: the take rule, once per set; every member holds the stem, since whichever stands first in the wave is restored
        std::vector<Req*> members;
        for (auto& r : rs) members.push_back(r.get());
        stem_match(members.data(), n, g.stem);
    }
    std::lock_guard<std::mutex> lk(mu_);
    {   // [EXT] codec preambles: the engine-level setting, read once per set; every member restores the same snapshot into its own stream
        const int pid = preamble_of_request(want_pcm && codec_, g.preamble, pres_.setting);
        try { for (int i = 0; pid >= 0 && i < n; i++) pre_attach(rs[i].get(), pid); }
        catch (...) { for (auto& r : rs) drop_held(r.get()); throw; }
    }
    const int64_t set = next_set_++;
    for (int i = 0; i < n; i++) { rs[i]->set = set; req_ids[i] = enqueue(std::move(rs[i]), pending_); }
    cand_sets_++;
}

// [EXT] live text append.  The caller's thread only copies under mu_; the scheduler thread moves the ids to the device between frame
// groups (collect_appends + run_group), so an append never issues a HIP call that could land inside another thread's graph capture.
int Engine::append_trail(int64_t id, const int32_t* ids, int n, bool close) {
    Q3_CHECK(n >= 0, "n must be >= 0");
    Q3_CHECK(n == 0 || ids, "ids missing");
    std::lock_guard<std::mutex> lk(mu_);
    Req& r = req(id);
    Q3_CHECK(r.r.open, "the request was not submitted with an open trail");
    Q3_CHECK(!r.closed, "the request's trail is already closed");
    if (r.job.cancel || (r.state != REQ_QUEUED && r.state != REQ_RUNNING)) return 1; // cancelled, finished (EOS / max_steps), done or failed: nothing appended
    Q3_CHECK(r.trail_own.size() + (size_t)n <= (size_t)p_.max_prompt, "the trail would exceed max_prompt ids");
    r.trail_own.insert(r.trail_own.end(), ids, ids + n);
    if (close) r.closed = true;
    trail_dirty_ = true;
    wake_++;
    cv_.notify_all();
    return 0;
}

void Engine::trail_progress(int64_t id, int* n_appended, int* n_consumed, bool* closed) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    Q3_CHECK(!r.job.decode, "a decode-only request has no trail");
    const int n = (int)r.trail_ids().size();
    *n_appended = n; *n_consumed = std::min(r.fed, n); *closed = !r.r.open || r.closed;
}

// scheduler thread: appended ids and close flags of live open slots go into the slot table; the ids are uploaded by run_group
void Engine::collect_appends() {
    std::lock_guard<std::mutex> lk(mu_);
    if (!trail_dirty_) return;
    trail_dirty_ = false;
    for (int b = 0; b < B_; b++) {
        if (!slots_.live[b] || !slot_req_[b]->r.open) continue;
        const Req& r = *slot_req_[b];
        int32_t& have = slots_.hi(SF_NTRAIL)[b]; int32_t& open = slots_.hi(SF_OPEN)[b];
        const int n = (int)r.trail_own.size();
        if (n > have) {
            if (h_pend_[b].empty()) h_pend_off_[b] = have;
            h_pend_[b].insert(h_pend_[b].end(), r.trail_own.begin() + have, r.trail_own.begin() + n);
            have = n;
            slot_dirty_ = true;
        }
        const int op = r.closed ? 0 : 1;
        if (op != open) { open = op; slot_dirty_ = true; }
    }
}

// [EXT] request cancellation.  Like an append, the caller's thread only marks the request under mu_ and wakes the scheduler, which does
// the device-side work between two frame groups; a request still in the queue owns nothing and ends right here.
int Engine::cancel(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    Req& r = req(id);
    Q3_CHECK(r.build_stem < 0, "unknown request id"); // [EXT] prompt stems: a build is internal; q3tts_stem_release is how a stem goes
    if (req_ended(r.state)) return 1;
    if (r.job.cancel) return 0; // the first cancel is still pending
    r.job.cancel = true;
    if (cancel_action(r.state, false, false, r.want_pcm) == CANCEL_AT_ONCE) {
        std::deque<Req*>& q = r.job.decode ? decode_q_ : pending_;
        q.erase(std::find(q.begin(), q.end(), &r));
        r.state = REQ_CANCELLED; r.t_done = now_ms();
        drop_held(&r); // [EXT] codec preambles, prompt stems: it never enqueued a restore
    } else cancel_ids_.push_back(id);
    wake_++;
    cv_.notify_all();
    return 0;
}

// scheduler thread, between two frame groups: live slots of cancelled requests are retired, draining ones lose their unstarted chunks;
// a request inside an asynchronous prefill wave stays on the list until activate() has kept it out of the batch
void Engine::collect_cancels() {
    std::vector<Req*> live;
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (cancel_ids_.empty()) return;
        std::vector<int64_t> ids;
        ids.swap(cancel_ids_);
        for (int64_t id : ids) {
            auto it = reqs_.find(id);
            if (it == reqs_.end()) continue; // ended and released meanwhile
            Req* r = it->second.get();
            const bool is_live = r->slot >= 0 && slots_.live[r->slot];
            switch (cancel_action(r->state, r->slot >= 0 && !is_live, is_live, r->want_pcm)) {
            case CANCEL_AT_ACTIVATE: cancel_ids_.push_back(id); break;
            case CANCEL_RETIRE: case CANCEL_RETIRE_FENCE: live.push_back(r); break;
            case CANCEL_PURGE: worker_->purge(&r->job); break;
            default: break;
            }
        }
    }
    for (Req* r : live) retire(r, false);
}

// moves queued requests into free slots (lowest slot first, so the live slots stay packed and a narrow graph suffices)
void Engine::admit(bool stalled) {
    if (async_pf_ && !pf_batch_.empty()) return; // one admission wave in flight at a time
    std::vector<Req*> batch;
    {
        std::lock_guard<std::mutex> lk(mu_);
        // admissions are grouped under load: wait until an eighth of the slots is free -- unless the engine is idle or the free slots
        // already cover the whole queue (a synchronous prefill stalls every running sequence; an asynchronous one still shares the GPU)
        int reserved = 0;
        for (int b = 0; b < B_; b++) if (slot_req_[b]) reserved++;
        static const int quantum_div = [] { const char* e = std::getenv("Q3_ADMIT_DIV"); return e ? std::max(1, atoi(e)) : 8; }();
        const int free_slots = B_ - reserved, quantum = std::max(1, B_ / quantum_div);
        if (free_slots < quantum && n_active_ > 0 && free_slots < (int)pending_.size() && !stalled) return; // waiting slots free nothing
        // what the wave takes (sched_logic.h): a slot each, a codec stream each with PCM, the 4096 rows of an asynchronous wave's staging arena,
        // [EXT] a candidate set whole or not at all.  The rule sees the entries the free slots could take and the rest of the last one's set
        std::vector<QueueEntry> q;
        for (Req* r : pending_) {
            if ((int)q.size() >= free_slots && (q.empty() || r->set == 0 || r->set != q.back().set)) break;
            q.push_back({admission_rows(r->r.n_prompt, r->n_skip, r->r.n_prefix), r->want_pcm, r->set});
        }
        for (int take = admission_take(q, free_slots, (int)cs_free_.size(), async_pf_ && n_active_ > 0); take > 0; take--) {
            Req* r = pending_.front();
            int slot = -1;
            for (int b = 0; b < B_; b++) if (!slot_req_[b]) { slot = b; break; }
            pending_.pop_front();
            r->slot = slot;
            if (r->want_pcm) { r->job.cs = cs_free_.back(); cs_free_.pop_back(); }
            r->state = REQ_RUNNING; r->t_admit = now_ms();
            slot_req_[slot] = r;
            batch.push_back(r);
        }
    }
    if (batch.empty()) return;
    alloc_stem_stores(batch); // [EXT] prompt stems: the stores of the wave's builds
    for (Req* r : batch) {
        if (r->want_pcm) worker_->push_reset(&r->job); // the decoder thread clears the codec stream's state right before the request's first chunk
        r->chunker.reset(new Chunker([this, r](const int64_t* codes, int n_codes, bool is_final) { if (r->want_pcm) worker_->push_chunk(&r->job, codes, n_codes, is_final); }));
        Q3_HIP(hipEventCreate(&r->ev_admit));
    }
    if (async_pf_ && n_active_ > 0) { prefill_async(batch); return; } // sequences are running: do not stall them
    // ---- in-line form (nothing is running, or a single-slot engine): one batched prefill of the whole wave on the AR stream ----
    for (Req* r : batch) kv_t_->release(r->slot), kv_t_->ensure(r->slot, kv_positions(r->r, r->score), st_);
    bool sampled = live_variant(slots_).sampled; // of the prefill heads: the wave joins whatever is live
    std::vector<Req*> live, scores, builds; // [EXT] scoring: a score request never goes live; its rows are computed by the walk.  Nor does a stem build
    for (Req* r : batch) {
        if (r->r.sampler.temperature > 0.0f) sampled = true;
        (r->build_stem >= 0 ? builds : r->score ? scores : live).push_back(r);
    }
    hipEvent_t e0, e1;
    Q3_HIP(hipEventCreate(&e0)); Q3_HIP(hipEventCreate(&e1));
    go_live(live); // slot state first: the prefill heads write code_0 / hidden straight into the live arrays
    { std::lock_guard<std::mutex> lk(mu_); n_active_ += (int)live.size(); }
    Q3_HIP(hipEventRecord(e0, st_));
    for (Req* r : batch) Q3_HIP(hipEventRecord(r->ev_admit, st_)); // the AR stream is idle here: marks "admitted"
    prefill_wave(ar_, batch, sampled);
    Q3_HIP(hipEventRecord(e1, st_));
    Q3_HIP(hipStreamSynchronize(st_));
    { float ms = 0; Q3_HIP(hipEventElapsedTime(&ms, e0, e1)); stats.prefill_ms += ms; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    {
        const double t = now_ms();
        std::lock_guard<std::mutex> lk(mu_);
        for (Req* r : batch) r->prefill_ms = t - r->t_submit;
    }
    finish_scores(scores);
    finish_builds(builds);
}

// [EXT] decoding given frames.  The request is the codec half of a request alone: a copy of the caller's frames that waits for a codec stream.
int64_t Engine::submit_decode(const int32_t* codes, int n) {
    if (const char* why = decode_refusal(codes, n, p_.max_steps, codec_ != nullptr)) throw Error(why);
    std::unique_ptr<Req> r(new Req());
    r->job.decode = true; r->want_pcm = true;
    take_out(r.get(), n); // [EXT] the engine's output settings
    r->r.max_steps = n; r->r.n_prompt = 0; r->r.sampler.temperature = 0.0f;
    r->codes.assign(codes, codes + (size_t)n * 16); r->fed = n;
    r->t_submit = now_ms();
    std::lock_guard<std::mutex> lk(mu_);
    if (pres_.setting >= 0) pre_attach(r.get(), pres_.setting); // [EXT] codec preambles: the engine-level setting, read once per request
    dec_reqs_++;
    return enqueue(std::move(r), decode_q_);
}

// scheduler thread, after admit(): the generating wave has taken its streams; decode-only requests take free ones in order, up to decode_w_
// holders.
void Engine::admit_decodes() {
    std::lock_guard<std::mutex> lk(mu_);
    for (int take = decode_admit((int)decode_q_.size(), (int)cs_free_.size(), n_decoding_, decode_w_); take > 0; take--) {
        Req* r = decode_q_.front();
        decode_q_.pop_front();
        r->job.cs = cs_free_.back(); cs_free_.pop_back();
        r->state = REQ_DRAINING; r->t_admit = now_ms();
        n_draining_++; n_decoding_++;
        dec_admitted_.push_back(r);
    }
}

// A request's whole task list -- reset, the chunks a Chunker cuts from its frames, fence -- goes to the low queue in one piece (part of run_group's hand-over, or one of its own).
void Engine::enqueue_decodes() {
    std::vector<Req*> batch;
    batch.swap(dec_admitted_);
    for (Req* r : batch) {
        Q3_HIP(hipEventCreate(&r->ev_admit));
        Q3_HIP(hipEventRecord(r->ev_admit, st_)); // the AR stream is idle here: marks "admitted"
        CodecWorker::Handover piece(worker_.get(), true);
        worker_->push_reset(&r->job);
        Chunker cut([&](const int64_t* codes, int n_codes, bool is_final) { worker_->push_chunk(&r->job, codes, n_codes, is_final); });
        push_frames(cut, r->codes.data(), r->fed);
        cut.push(nullptr, 0, true);
        worker_->push_fence(&r->job);
    }
}

// The asynchronous form's start: the wave is prefilled on the second talker context and its stream while the frame graph keeps stepping
// the running sequences.  Nothing here waits: every chunk is enqueued, and pf_done_ behind the last tells step() when to activate().
void Engine::prefill_async(const std::vector<Req*>& wave) {
    for (Req* r : wave) {
        kv_t_->release(r->slot);
        kv_t_->ensure(r->slot, kv_positions(r->r, r->score), st_pf_);
    }
    pf_.cur.reset(); // the previous wave has been activated: its staging has been consumed
    Q3_HIP(hipEventRecord(pf_e0_, st_pf_));
    for (Req* r : wave) Q3_HIP(hipEventRecord(r->ev_admit, st_pf_));
    prefill_wave(pf_, wave, false);
    Q3_HIP(hipEventRecord(pf_done_, st_pf_));
    pf_batch_ = wave;
    n_prefilling_ = (int)wave.size();
}

// The slots of a wave's requests join the frame graph: slot state (positions, sampler parameters, RNG stream, frame counters) goes live.
// Runs on st_ between two scheduler operations; in line before the walk, asynchronously behind it (activate).
void Engine::go_live(const std::vector<Req*>& batch) {
    ar_.cur.reset(); // st_ is idle between scheduler operations
    q3_u64 armed[17]; std::fill_n(armed, 17, pack_key(-INFINITY, 0));
    bool prefix_pcm = false; // [EXT] resume: the chunks the wave's prefixes make up are one hand-over to the decoder thread
    for (Req* r : batch) prefix_pcm = prefix_pcm || (r->want_pcm && r->r.n_prefix >= 4);
    {
        CodecWorker::Handover hold(worker_.get(), worker_ && prefix_pcm);
        for (Req* r : batch) {
            const int b = r->slot;
            slots_.load(b, r->r);
            // [EXT] resume: frame k's code_0 is talker draw k and the predictor stream stands at 15 k; greedy streams stay at 0.  The history row
            // takes the prefix frames as k_advance_keys would have written them, and the chunker the chunks the scheduler would have cut.
            const int k = r->r.n_prefix;
            const uint32_t draws = r->r.sampler.temperature > 0.0f ? (uint32_t)k : 0u, pdraws = 15u * (uint32_t)k;
            if (k > 0) {
                h2d(d_hist_.p + (size_t)b * hist_stride_, r->prefix_own.data(), (size_t)k * 64);
                push_frames(*r->chunker, r->prefix_own.data(), k);
            }
            StdRng rng(r->seed); // llama/mod.rs:648: the device regenerates this ChaCha12 stream from the key and a draw counter
            h2d(d_rngkey_.p + (size_t)b * 8, rng.key(), 32);
            h2d(d_draws_.p + b, &draws, 4);
            if (r->r.opts.pred_sampled()) { // [EXT] the predictor's own stream: seed_from_u64(seed ^ Q3_PRED_SEED_XOR)
                StdRng prng(r->seed ^ (uint64_t)Q3_PRED_SEED_XOR);
                h2d(d_prngkey_.p + (size_t)b * 8, prng.key(), 32);
                h2d(d_pdraws_.p + b, &pdraws, 4);
            }
            h_pend_[b].clear();
            std::vector<int32_t> ids; // [EXT] streaming text: the slot's trailing ids -- of an open trail those appended so far (later: collect_appends)
            { std::lock_guard<std::mutex> lk(mu_); ids = r->trail_ids(); slots_.hi(SF_OPEN)[b] = r->r.open && !r->closed; }
            slots_.hi(SF_NTRAIL)[b] = (int)ids.size(); // upload_slot_state below sends the count and the flag
            if (!ids.empty()) h2d(d_trail_.p + (size_t)b * p_.max_prompt, ids.data(), ids.size() * 4);
            h2d(d_keys_.p + (size_t)b * 16, armed, 16 * 8);
            h2d(d_next_key0_.p + b, armed, 8);
            if (lp_ready_.load()) { // [EXT] log-probabilities: the slot's record flag; a recording slot's rows start as "not computed"
                const int32_t rec = r->r.logprobs ? 1 : 0;
                h2d(d_lp_rec_.p + b, &rec, 4);
                if (rec) Q3_HIP(hipMemsetD32Async((hipDeviceptr_t)(d_lp_.p + (size_t)b * lp_rows_ * Q3_LOGPROB_COLS), (int)q3_f32_bits(Q3_LOGPROB_NONE),
                                                  (size_t)lp_rows_ * Q3_LOGPROB_COLS, st_));
            }
            slots_.live[b] = 1;
        }
    }
    upload_slot_state();
}

// The asynchronous wave's completion, on st_ between two frame groups once pf_done_ has completed: its requests go live, the staged hidden
// row of each is copied in and code_0 of its first frame is drawn from the staged logits with the slot's own sampler state (greedy slots
// take the sampler kernel's first-max branch).
void Engine::activate() {
    std::vector<Req*> batch, dropped, scores, builds;
    batch.swap(pf_batch_);
    for (Req* r : batch) if (r->build_stem >= 0) builds.push_back(r); // [EXT] prompt stems: a build never goes live and cannot be cancelled
    batch.erase(std::remove_if(batch.begin(), batch.end(), [](Req* r) { return r->build_stem >= 0; }), batch.end());
    {   // [EXT] requests cancelled while the wave ran do not go live; their wave-mates are not disturbed
        std::lock_guard<std::mutex> lk(mu_);
        const double t = now_ms();
        for (Req* r : batch) if (r->job.cancel) { r->prefill_ms = t - r->t_submit; dropped.push_back(r); }
        batch.erase(std::remove_if(batch.begin(), batch.end(), [](Req* r) { return r->job.cancel.load(); }), batch.end());
    }
    for (Req* r : dropped) retire(r, false); // slot, KV pages and -- through the fence, behind the reset task already queued -- codec stream
    for (Req* r : batch) if (r->score) scores.push_back(r); // [EXT] scoring: a score request never goes live
    batch.erase(std::remove_if(batch.begin(), batch.end(), [](Req* r) { return r->score; }), batch.end());
    go_live(batch);
    for (Req* r : batch) {
        const int b = r->slot;
        Q3_HIP(hipMemcpyAsync(d_thidden_.p + (size_t)b * Q3_EMBD, d_pf_hidden_.p + (size_t)b * Q3_EMBD, (size_t)Q3_EMBD * 4, hipMemcpyDeviceToDevice, st_));
        SampleArgs sa = first_head_args(d_pf_logits_.p + (size_t)b * tl_stride_, b);
        if (resumed_penalised(r->r)) head_history(sa, b);
        launch_sample(st_, sa, 1);
        if (r->r.logprobs) first_head_logprobs(st_, d_pf_logits_.p + (size_t)b * tl_stride_, b, r->r.n_prefix);
    }
    Q3_HIP(hipStreamSynchronize(st_));
    { float ms = 0; Q3_HIP(hipEventElapsedTime(&ms, pf_e0_, pf_done_)); stats.prefill_ms += ms; }
    n_prefilling_ = 0;
    {
        const double t = now_ms();
        std::lock_guard<std::mutex> lk(mu_);
        for (Req* r : batch) r->prefill_ms = t - r->t_submit;
        for (Req* r : scores) r->prefill_ms = t - r->t_submit;
        n_active_ += (int)batch.size();
    }
    finish_scores(scores);
    finish_builds(builds);
}

// [EXT] scoring given frames.  Like the log-probability buffers, the state goes to the device on first use, under the same locks.
void Engine::ensure_score() {
    std::lock_guard<std::mutex> lk(sc_mu_);
    if (sc_ready_.load()) return;
    std::lock_guard<std::mutex> cap(capture_mutex());
    int prev = 0;
    Q3_HIP(hipGetDevice(&prev));
    Q3_HIP(hipSetDevice(dev_));
    try {
        const int W = score_w_, rows = std::max(talker_->max_tok(), pf_chunk_); // rows: the widest prefill chunk of either lane
        pred_sc_.reset(new Transformer(*predictor_, 16 * W));
        kv_sc_.reset(new KvPool(predictor_->hp().n_layer, predictor_->hp().n_kv, W, W, 1));
        for (int w = 0; w < W; w++) kv_sc_->ensure(w, 16);
        std::vector<int32_t> seq, slot, pos;
        for (int F = 1; F <= W; F++)
            for (int p = 0; p < 16; p++)
                for (int f = 0; f < F; f++) { seq.push_back(f); slot.push_back(p); for (int s4 = 0; s4 < 4; s4++) pos.push_back(p); } // engine.rs:316-318
        d_sc_seq_.alloc(seq.size()); d_sc_seq_.upload(seq.data(), seq.size());
        d_sc_slot_.alloc(slot.size()); d_sc_slot_.upload(slot.data(), slot.size());
        d_sc_pos_.alloc(pos.size()); d_sc_pos_.upload(pos.data(), pos.size());
        std::vector<const float*> tabs(15); std::vector<int64_t> tab_rows(15);
        for (int q = 0; q < 15; q++) { tabs[q] = d_proj_tab_[q].p; tab_rows[q] = assets_->codec_rows[q]; }
        d_sc_tabs_.alloc(15); d_sc_tabs_.upload(tabs.data(), 15);
        d_sc_tab_rows_.alloc(15); d_sc_tab_rows_.upload(tab_rows.data(), 15);
        d_sc_codes_.alloc((size_t)rows * 16); d_sc_tlogits_.alloc((size_t)rows * tl_stride_); d_sc_hidden_.alloc((size_t)rows * Q3_EMBD);
        d_sc_hproj_.alloc((size_t)W * dP_); d_sc_in_.alloc((size_t)16 * W * dP_); d_sc_plogits_.alloc((size_t)15 * W * Q3_CODEBOOK_SIZE);
        d_sc_out_.alloc((size_t)B_ * p_.max_steps * Q3_LOGPROB_COLS);
        Q3_HIP(hipStreamSynchronize(nullptr)); // the pool's memsets ran on the null stream; the engine's streams do not wait for it
    } catch (...) { (void)hipSetDevice(prev); throw; }
    Q3_HIP(hipSetDevice(prev));
    sc_ready_ = true;
}

int64_t Engine::submit_score(const float* prompt, int n_prompt, const int32_t* trail, int n_trail, const int32_t* codes, int n) {
    if (const char* why = score_refusal(prompt, n_prompt, p_.max_prompt, trail, n_trail, codes, n, p_.max_steps, kv_rows_, talker_->ggml_mode()))
        throw Error(why);
    ensure_score();
    if (n_trail > 0) ensure_text_stream();
    std::unique_ptr<Req> r(new Req());
    r->score = true;
    GenRequest& g = r->r;
    g.n_prompt = n_prompt; g.max_steps = n; g.sampler.temperature = 0.0f; g.n_trail = n_trail;
    g.n_prefix = n - 1; // feedback rows behind the prompt: the last frame's row would only serve a frame n
    r->prompt_own.assign(prompt, prompt + (size_t)n_prompt * Q3_EMBD); g.prompt = r->prompt_own.data();
    r->trail_own.assign(trail, trail + n_trail); g.trail = r->trail_own.data();
    r->prefix_own.assign(codes, codes + (size_t)n * 16); g.prefix = r->prefix_own.data();
    r->t_submit = now_ms();
    std::lock_guard<std::mutex> lk(mu_);
    return enqueue(std::move(r), pending_);
}

// The score rows of one prefill chunk, behind the chunk's forward on its stream: per run the talker head over the rows (logits and hidden rows
// into chunk-wide buffers), then passes of at most W frames on the second predictor context -- projection of the hidden rows (k_project_mt, as
// the frame graph's), k_score_inputs, one forward of 16 F position-major tokens, 15 heads over contiguous token ranges, k_score_rows.
void Engine::score_chunk(hipStream_t st, Transformer& talker, const std::vector<Req*>& batch, const std::vector<ScoreRun>& runs, int32_t* h_codes) {
    if (runs.empty()) return;
    const int W = score_w_;
    int at = 0;
    for (const ScoreRun& run : runs) {
        Req* r = batch[run.req];
        Q3_CHECK((size_t)(at + run.n) * 16 <= d_sc_codes_.n && run.frame + run.n <= r->r.max_steps, "score rows outside the chunk buffers");
        std::copy(r->prefix_own.begin() + (size_t)run.frame * 16, r->prefix_own.begin() + (size_t)(run.frame + run.n) * 16, h_codes + (size_t)at * 16);
        Q3_HIP(hipMemcpyAsync(d_sc_codes_.p + (size_t)at * 16, h_codes + (size_t)at * 16, (size_t)run.n * 64, hipMemcpyHostToDevice, st));
        talker.head(st, run.row, run.n, 0, tl_stride_, d_sc_tlogits_.p + (size_t)at * tl_stride_, tl_stride_, nullptr, -1, d_sc_hidden_.p + (size_t)at * Q3_EMBD);
        for (int f0 = 0; f0 < run.n; f0 += W) {
            const int F = std::min(W, run.n - f0);
            const int32_t* codes = d_sc_codes_.p + (size_t)(at + f0) * 16;
            launch_project_blk(st, d_sc_hidden_.p + (size_t)(at + f0) * Q3_EMBD, Q3_EMBD, d_proj_wblk_.p, d_proj_b_.p, Q3_EMBD, dP_, d_sc_hproj_.p, dP_, F);
            launch_score_inputs(st, d_sc_hproj_.p, d_sc_tabs_.p, d_sc_tab_rows_.p, dP_, codes, F, d_sc_in_.p);
            const size_t m0 = (size_t)16 * F * (F - 1) / 2; // the routing tables of width F
            TokMeta tm{d_sc_seq_.p + m0, d_sc_slot_.p + m0, d_sc_pos_.p + m0 * 4};
            Transformer::Input in; in.x = d_sc_in_.p; in.x_stride = dP_;
            pred_sc_->set_same_seq_tokens(true);
            pred_sc_->forward(st, in, 16 * F, tm, kv_sc_->view(), nullptr);
            for (int q = 0; q < 15; q++) // the logits for codes[f][q + 1]: head slice q at position q + 1
                pred_sc_->head(st, (q + 1) * F, F, q * Q3_CODEBOOK_SIZE, Q3_CODEBOOK_SIZE, d_sc_plogits_.p + (size_t)q * W * Q3_CODEBOOK_SIZE, Q3_CODEBOOK_SIZE);
            ScoreRowsArgs sa;
            sa.tlogits = d_sc_tlogits_.p + (size_t)(at + f0) * tl_stride_; sa.t_stride = tl_stride_;
            sa.plogits = d_sc_plogits_.p; sa.p_head_stride = (size_t)W * Q3_CODEBOOK_SIZE; sa.codes = codes;
            sa.out = d_sc_out_.p + ((size_t)r->slot * p_.max_steps + run.frame + f0) * Q3_LOGPROB_COLS;
            launch_score_rows(st, sa, F);
        }
        at += run.n;
    }
    Q3_LAUNCH_CHECK();
}

// Scheduler thread, st_ idle and the wave's prefill complete: a score request's rows come to the host, rows and codes appear in one critical
// section, and the slot and its KV pages are free again.  A request cancelled meanwhile ends CANCELLED with no frames.
void Engine::finish_scores(const std::vector<Req*>& scores) {
    for (Req* r : scores) {
        const int b = r->slot, n = r->r.max_steps;
        bool cancelled;
        { std::lock_guard<std::mutex> lk(mu_); cancelled = r->job.cancel; }
        const float* rows = nullptr;
        if (!cancelled) {
            ar_.cur.reset();
            rows = (const float*)d2h_begin(d_sc_out_.p + (size_t)b * p_.max_steps * Q3_LOGPROB_COLS, (size_t)n * Q3_LOGPROB_COLS * 4);
            Q3_HIP(hipStreamSynchronize(st_));
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            if (r->job.cancel) r->state = REQ_CANCELLED;
            else {
                r->codes = r->prefix_own;
                r->lp.assign(rows, rows + (size_t)n * Q3_LOGPROB_COLS);
                r->fed = n;
                r->state = REQ_DONE;
            }
            slot_req_[b] = nullptr; r->slot = -1;
            r->t_done = now_ms();
            cv_.notify_all();
        }
        kv_t_->release(b);
    }
}

// A request gives its slot back.  flush_tail (EOS / max_steps; engine.rs:644-649): final flush of the chunker, then the decoder drains.
// [EXT] Without it (a cancel): the tail is not decoded and the chunks the decoder thread has not taken yet are dropped.  Either way a request
// with PCM ends behind a fence, once nothing of it is in flight; a slot that never went live (cancelled inside a prefill wave) is only unreserved.
void Engine::retire(Req* r, bool flush_tail) {
    if (flush_tail) r->chunker->push(nullptr, 0, true);
    const int b = r->slot;
    {
        std::lock_guard<std::mutex> lk(mu_);
        slot_req_[b] = nullptr;
        if (slots_.live[b]) { slots_.live[b] = 0; n_active_--; }
        r->slot = -1;
        r->state = retired_state(r->want_pcm, r->job.cancel);
        if (r->want_pcm) n_draining_++;
        else { r->t_done = now_ms(); drop_held(r); cv_.notify_all(); } // [EXT] prompt stems: its wave completed before it went live or was dropped (without PCM it holds no preamble)
    }
    if (r->want_pcm) {
        if (!flush_tail) worker_->purge(&r->job);
        worker_->push_fence(&r->job);
    }
    slots_.reset(b); h_pend_[b].clear();
    kv_t_->release(b); // from the next group on the slot steps on the scratch sequence (upload_slot_state)
    slot_dirty_ = true;
}

static int pick_width(int hi, int W) { // graph widths: powers of two (and the full width)
    int w = 1;
    while (w < hi) w <<= 1;
    return std::min(w, W);
}

// one streaming step (4 frames, engine.rs:505-512) for every active slot
void Engine::run_group() {
    int hi = 0, remaining = 0;
    int32_t* h_nfr = slots_.hi(SF_NFRAMES); int32_t* h_fin = slots_.hi(SF_FINISHED);
    for (int b = 0; b < B_; b++)
        if (slots_.live[b]) { hi = b + 1; remaining = std::max(remaining, slot_req_[b]->r.max_steps - h_nfr[b]); }
    const FrameVariant v = live_variant(slots_);
    ar_.cur.reset(); // st_ is idle between scheduler operations: everything staged earlier has been consumed
    for (int b = 0; b < B_; b++) // [EXT] appended ids collected since the last group: the new tail of the slot's id row
        if (!h_pend_[b].empty()) {
            h2d(d_trail_.p + (size_t)b * p_.max_prompt + h_pend_off_[b], h_pend_[b].data(), h_pend_[b].size() * 4);
            h_pend_[b].clear();
        }
    if (slot_dirty_) upload_slot_state();
    const int width = pick_width(hi, B_);
    const int group = std::max(1, std::min(4, remaining));
    const bool eager = instrument_ || !p_.use_graph;
    FrameGraph& fg = frame_graph(width, v, !eager);
    if (instrument_) { talker_->timer = &timer_; predictor_->timer = &timer_; talker_->timer_gu = &timer_gu_; }
    hipEvent_t e0, e1;
    Q3_HIP(hipEventCreate(&e0)); Q3_HIP(hipEventCreate(&e1));
    Q3_HIP(hipEventRecord(e0, st_));
    for (int g = 0; g < group; g++) {
        if (eager) record_frame(fg, v);
        else Q3_HIP(hipGraphLaunch(fg.exec, st_));
    }
    Q3_HIP(hipEventRecord(e1, st_));
    // results of the group: frame counters, finished flags and the (at most `group`) new code rows of every active slot
    const int32_t* p_nfr = (const int32_t*)d2h_begin(di(SF_NFRAMES), (size_t)width * 4);
    const int32_t* p_fin = (const int32_t*)d2h_begin(di(SF_FINISHED), (size_t)width * 4);
    std::vector<const int32_t*> p_hist(width, nullptr);
    std::vector<const float*> p_lp(width, nullptr); // [EXT] the same rows of d_lp_, for the slots that record
    for (int b = 0; b < width; b++)
        if (slots_.live[b]) {
            Req* r = slot_req_[b];
            const int rows = std::min(group, r->r.max_steps - r->fed);
            if (rows > 0) p_hist[b] = (const int32_t*)d2h_begin(d_hist_.p + (size_t)b * hist_stride_ + (size_t)r->fed * 16, (size_t)rows * 64);
            if (rows > 0 && r->r.logprobs)
                p_lp[b] = (const float*)d2h_begin(d_lp_.p + ((size_t)b * lp_rows_ + r->fed) * Q3_LOGPROB_COLS, (size_t)rows * Q3_LOGPROB_COLS * 4);
        }
    Q3_HIP(hipStreamSynchronize(st_));
    { float ms = 0; Q3_HIP(hipEventElapsedTime(&ms, e0, e1)); stats.frame_loop_ms += ms; }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    stats.steps++; stats.slot_frames += (double)width * group; stats.graph_frames += group;
    talker_->timer = nullptr; predictor_->timer = nullptr; talker_->timer_gu = nullptr;
    if (instrument_) {
        stats.gemv_ms += timer_.collect_ms(); stats.gemv_bytes += timer_.bytes; stats.gemv_launches += timer_.launches; timer_.bytes = 0; timer_.launches = 0;
        stats.gu_ms += timer_gu_.collect_ms(); stats.gu_bytes += timer_gu_.bytes; stats.gu_launches += timer_gu_.launches; timer_gu_.bytes = 0; timer_gu_.launches = 0;
    }
    std::memcpy(h_nfr, p_nfr, (size_t)width * 4); std::memcpy(h_fin, p_fin, (size_t)width * 4);
    // The group's chunks, the tails and fences of the slots it retires and the tasks of the decode-only requests admitted in this step reach
    // the decoder thread as one hand-over (CodecWorker::Handover): it forms no pass meanwhile (microseconds)
    CodecWorker::Handover hold(worker_.get(), worker_ != nullptr);
    for (int b = 0; b < width; b++) {
        if (!slots_.live[b]) continue;
        Req* r = slot_req_[b];
        if (h_nfr[b] > r->fed) { // hand new frames to the chunker (engine.rs:613-620)
            const int nnew = h_nfr[b] - r->fed;
            const int32_t* hbuf = p_hist[b];
            {   // codes and log-probabilities grow in one critical section: fetch() and fetch_logprobs() never disagree on n_frames
                std::lock_guard<std::mutex> lk(mu_);
                r->codes.insert(r->codes.end(), hbuf, hbuf + (size_t)nnew * 16);
                if (p_lp[b]) r->lp.insert(r->lp.end(), p_lp[b], p_lp[b] + (size_t)nnew * Q3_LOGPROB_COLS);
                r->fed = h_nfr[b];
            }
            push_frames(*r->chunker, hbuf, nnew);
            stats.frames += nnew;
        }
        if (h_fin[b] || h_nfr[b] >= r->r.max_steps) retire(r, true);
    }
    enqueue_decodes();
}

static double g_t_harvest = 0, g_t_admit = 0, g_t_group = 0, g_t_idle = 0;
static const bool g_trace = std::getenv("Q3_SCHED_TRACE") != nullptr;
bool Engine::step() {
    std::lock_guard<std::mutex> step_lock(step_mu_);
    Q3_HIP(hipSetDevice(dev_)); // HIP's current device is per thread: any thread may drive any engine of a multi-device group
    if (worker_) worker_->start();
    const double t0 = now_ms();
    harvest(false);
    const double t1 = now_ms();
    if (async_pf_ && n_prefilling_ > 0) { // has the admission wave finished its prefill?  (wait for it when nothing else can run)
        if (n_active_ == 0) Q3_HIP(hipEventSynchronize(pf_done_));
        if (hipEventQuery(pf_done_) == hipSuccess) activate();
    }
    free_stem_stores(); // [EXT] prompt stems: the stores of stems recycled since the last step
    collect_appends();
    collect_cancels(); // before admit: a slot a cancel frees can be refilled in this step
    admit(n_active_ > 0 && slots_.all_live_stalled());
    if (codec_) admit_decodes();
    if (!(n_active_ > 0 && !slots_.all_live_stalled())) enqueue_decodes(); // no frame group in this step: nothing to meet, the tasks go at once
    const double t2 = now_ms();
    // [EXT] live text append: when every live slot waits for text, no frame group runs (graph_frames stays put); prefill and codec
    // work still proceed, and with none left the driver sleeps until a submit or an append
    const bool stalled = n_active_ > 0 && slots_.all_live_stalled();
    const int dec_pending = stalled && worker_ ? worker_->pending() : 0;
    if (n_active_ > 0 && !stalled) run_group();
    else if (n_prefilling_ > 0) { Q3_HIP(hipEventSynchronize(pf_done_)); activate(); }
    else if (n_draining_ > 0 || dec_pending > 0) harvest(true);
    const double t3 = now_ms();
    if (g_trace) {
        g_t_harvest += t1 - t0; g_t_admit += t2 - t1; (n_active_ > 0 ? g_t_group : g_t_idle) += t3 - t2;
        fprintf(stderr, "[sched] harvest %.1f admit %.1f group %.1f drain-wait %.1f ms (frame_loop %.1f prefill %.1f)\n", g_t_harvest, g_t_admit, g_t_group, g_t_idle,
                stats.frame_loop_ms, stats.prefill_ms);
    }
    std::lock_guard<std::mutex> lk(mu_);
    stalled_idle_ = stalled && n_prefilling_ == 0 && dec_pending == 0;
    return n_active_ > 0 || n_prefilling_ > 0 || n_draining_ > 0 || !pending_.empty() || !decode_q_.empty();
}

ReqStatus Engine::poll(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    ReqStatus s;
    const bool ended = r.state == REQ_DONE || r.state == REQ_CANCELLED; // t_done is set, the PCM sits in r.pcm
    s.state = r.state; s.n_frames = r.fed; s.n_pcm = ended ? r.pcm_n : (int64_t)r.pcm_ready;
    s.queue_ms = (r.t_admit > 0 ? r.t_admit : ended ? r.t_done : now_ms()) - r.t_submit; // cancelled in the queue: until then
    s.prefill_ms = r.prefill_ms; s.first_chunk_ms = r.first_chunk_ms;
    s.total_ms = (ended ? r.t_done : now_ms()) - r.t_submit;
    s.error = r.error;
    return s;
}

void Engine::fetch(int64_t id, int32_t* codes, int frame_off, int max_frames, float* pcm, int64_t pcm_off, int64_t pcm_cap, int* got_frames, int64_t* got_pcm) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    if (pcm) Q3_CHECK(r.job.out.fmt.encoding == Q3_PCM_F32, "the request delivers int16 PCM: fetch it with fetch_pcm16"); // [EXT] output formats; nothing is copied
    int nf = 0; int64_t np = 0;
    if (codes && frame_off >= 0 && frame_off < r.fed) {
        nf = std::min(max_frames, r.fed - frame_off);
        std::copy(r.codes.begin() + (size_t)frame_off * 16, r.codes.begin() + (size_t)(frame_off + nf) * 16, codes);
    }
    if (pcm && pcm_off >= 0) np = copy_pcm(r, pcm, pcm_off, pcm_cap);
    if (got_frames) *got_frames = nf;
    if (got_pcm) *got_pcm = np;
}

// samples [off, off + cap) of the request's format that are available now, as bytes (mu_ held)
int64_t Engine::copy_pcm(const Req& r, void* out, int64_t off, int64_t cap) const {
    const bool done = r.state == REQ_DONE || r.state == REQ_CANCELLED;
    const int64_t avail = done ? r.pcm_n : (int64_t)r.pcm_ready;
    const unsigned char* src = done ? reinterpret_cast<const unsigned char*>(r.pcm.data())
                                    : (r.job.cs >= 0 ? reinterpret_cast<const unsigned char*>(worker_->staging(r.job.cs)) : nullptr);
    if (!src || off >= avail || cap <= 0) return 0;
    const int64_t n = std::min(cap, avail - off);
    const size_t b = r.job.sample_bytes();
    std::memcpy(out, src + (size_t)off * b, (size_t)n * b);
    return n;
}

// [EXT] output formats (q3tts_spec.h "output formats")
void Engine::set_output_format(const q3tts_pcm_format* f) {
    if (const char* why = pcm_format_refusal(f, codec_ != nullptr)) throw Error(why);
    std::lock_guard<std::mutex> lk(out_mu_);
    out_.fmt = f ? *f : OutSpec().fmt;
}
q3tts_pcm_format Engine::request_format(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    return req(id).job.out.fmt;
}
void Engine::fetch_pcm16(int64_t id, int16_t* out, int64_t off, int64_t cap, int64_t* got) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    Q3_CHECK(r.job.out.fmt.encoding == Q3_PCM_S16, "the request delivers f32 PCM: fetch it with fetch");
    Q3_CHECK(out && off >= 0, "null buffer or negative offset");
    const int64_t n = copy_pcm(r, out, off, cap);
    if (got) *got = n;
}
OutputStageStats Engine::output_stats() const { return codec_ ? codec_->output_stats() : OutputStageStats(); }

// [EXT] speaking rate (q3tts_spec.h "speaking rate")
void Engine::set_speech_rate(int pct) {
    Q3_CHECK(codec_, "the engine has no codec");
    if (const char* why = tsm_rate_why_not(pct)) throw Error(why);
    std::lock_guard<std::mutex> lk(out_mu_);
    out_.rate_pct = pct;
}
// the whole record is read at once, so that the rules judge settings that stood together at some instant
void Engine::take_out(Req* r, int max_steps, const OutSpec* given) const {
    OutSpec o;
    if (given) o = *given;
    else { std::lock_guard<std::mutex> lk(out_mu_); o = out_; }
    if (const char* why = out_submit_refusal(o, max_steps, worker_ ? (int64_t)worker_->slot_bytes() : 0, codec_ != nullptr)) throw Error(why);
    r->job.out = o;
}
int Engine::request_speech_rate(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    return req(id).job.out.rate_pct;
}
// [EXT] pitch (q3tts_spec.h "pitch")
void Engine::set_pitch(int pct) {
    Q3_CHECK(codec_, "the engine has no codec");
    if (const char* why = pitch_why_not(pct)) throw Error(why);
    std::lock_guard<std::mutex> lk(out_mu_);
    out_.pitch_pct = pct;
}
int Engine::request_pitch(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    return req(id).job.out.pitch_pct;
}
// [EXT] volume (q3tts_spec.h "volume")
void Engine::set_volume(int db10) {
    if (const char* why = volume_submit_refusal(db10, codec_ != nullptr)) throw Error(why);
    std::lock_guard<std::mutex> lk(out_mu_);
    out_.vol_db10 = db10;
}
int Engine::request_volume(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    return req(id).job.out.vol_db10;
}

// [EXT] loudness (q3tts_spec.h "loudness")
void Engine::set_loudness(bool on) {
    if (const char* why = loudness_submit_refusal(codec_ != nullptr)) throw Error(why);
    std::lock_guard<std::mutex> lk(out_mu_);
    out_.loud = on ? 1 : 0;
}
bool Engine::request_metered(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    return req(id).job.out.loud != 0;
}
void Engine::fetch_loudness(int64_t id, double* out, int64_t block_off, int64_t max_blocks, int64_t* got) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    Q3_CHECK(r.job.out.loud != 0, "the request is not metered");
    Q3_CHECK(out && block_off >= 0, "null buffer or negative offset");
    const bool done = r.state == REQ_DONE || r.state == REQ_CANCELLED;
    const double* src = done ? r.loud.data() : (r.job.cs >= 0 && r.loud_ready > 0 ? worker_->loud_staging(r.job.cs) : nullptr);
    const int64_t avail = done ? (int64_t)(r.loud.size() / 2) : (int64_t)r.loud_ready;
    int64_t n = 0;
    if (src && block_off < avail && max_blocks > 0) {
        n = std::min(max_blocks, avail - block_off);
        std::memcpy(out, src + (size_t)block_off * 2, (size_t)n * 2 * sizeof(double));
    }
    if (got) *got = n;
}

// [EXT] codec preambles and prompt stems (q3tts_spec.h "codec preambles" / "prompt stems"): the held objects.  Who holds what is counted by
// pres_ / stems_ (HeldTable, sched_logic.h); here is what the two kinds differ in, and the calls they share, once.
void Engine::recycled(const std::optional<PreHeld>& p) { // host bookkeeping only: every restore enqueued from the snapshot has completed
    if (!p) return;
    if (p->snap >= 0) codec_->snapshot_free(p->snap);
    pre_tail_free_.push_back(p->tail);
}
void Engine::recycled(const std::optional<StemHeld>& s) { // the scheduler thread frees the store: no HIP call in a caller's thread
    if (!s) return;
    if (s->store) stem_garbage_.emplace_back(s->store, s->bytes);
    wake_++; cv_.notify_all();
}
void Engine::drop_held(Req* r) {
    if (r->pre_held) { r->pre_held = false; recycled(pres_.unhold(r->pre)); }
    if (r->stem_held) { r->stem_held = false; recycled(stems_.unhold(r->stem)); }
}
void Engine::end_build(Req* r) {
    if (r->ev_admit) (void)hipEventDestroy(r->ev_admit);
    reqs_.erase(r->job.id);
    cv_.notify_all();
}
template <class T> void Engine::held_poll(T& tab, int id, int* state, int* n) {
    std::lock_guard<std::mutex> lk(mu_);
    const auto& e = tab.at(id);
    *state = e.refs.state; *n = e.n;
}
template <class T> bool Engine::held_wait(T& tab, int id, double timeout_ms) {
    const double t0 = now_ms();
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(mu_);
            if (tab.at(id).refs.state != HELD_BUILDING) return true;
            if (timeout_ms >= 0 && now_ms() - t0 > timeout_ms) return false;
            if (driver_on_) { cv_.wait_for(lk, std::chrono::milliseconds(5)); continue; }
        }
        step();
    }
}
template <class T> void Engine::held_release(T& tab, int id) {
    std::lock_guard<std::mutex> lk(mu_);
    recycled(tab.release_creator(id));
}
template <class T> void Engine::held_set(T& tab, int Voice::*field, int voice_id, int id) {
    std::lock_guard<std::mutex> lk(mu_);
    Q3_CHECK(!field || (voice_id >= 0 && voice_id < (int)voices_.size()), "unknown voice id");
    recycled(tab.swap_setting(field ? voices_[(size_t)voice_id].*field : tab.setting, id));
}
int Engine::voice_setting(int Voice::*field, int voice_id) {
    std::lock_guard<std::mutex> lk(mu_);
    Q3_CHECK(voice_id >= 0 && voice_id < (int)voices_.size(), "unknown voice id");
    return voices_[(size_t)voice_id].*field;
}
void Engine::preamble_poll(int id, int* state, int* n_frames) { held_poll(pres_, id, state, n_frames); }
void Engine::stem_poll(int id, int* state, int* n_rows) { held_poll(stems_, id, state, n_rows); }
bool Engine::preamble_wait(int id, double timeout_ms) { return held_wait(pres_, id, timeout_ms); }
bool Engine::stem_wait(int id, double timeout_ms) { return held_wait(stems_, id, timeout_ms); }
void Engine::preamble_release(int id) { held_release(pres_, id); }
void Engine::stem_release(int id) { held_release(stems_, id); }
void Engine::set_voice_preamble(int voice_id, int preamble_id) { held_set(pres_, &Voice::preamble, voice_id, preamble_id); }
void Engine::set_voice_stem(int voice_id, int stem_id) { held_set(stems_, &Voice::stem, voice_id, stem_id); }
void Engine::set_preamble(int preamble_id) { held_set(pres_, nullptr, 0, preamble_id); }
void Engine::set_stem(int stem_id) { held_set(stems_, nullptr, 0, stem_id); }
int Engine::voice_preamble(int voice_id) { return voice_setting(&Voice::preamble, voice_id); }
int Engine::voice_stem(int voice_id) { return voice_setting(&Voice::stem, voice_id); }

void Engine::pre_attach(Req* r, int pid) {
    auto* p = pres_.find(pid);
    Q3_CHECK(p && p->refs.state == Q3TTS_PREAMBLE_READY, "the request's preamble is not ready");
    pres_.hold(pid);
    r->pre = pid; r->pre_held = true; r->job.pre_snap = p->payload.snap; r->job.pre_tail = pre_tails_ + (size_t)p->payload.tail * Q3_PCM_HIST;
}
int Engine::preamble_create(const int32_t* codes, int n) {
    std::unique_ptr<Req> r(new Req());
    int live = 0;
    { std::lock_guard<std::mutex> lk(mu_); live = pres_.live(); }
    if (const char* why = preamble_refusal(codes, n, p_.max_steps, codec_ != nullptr, live, Q3TTS_CODEC_MAX_FRAMES)) throw Error(why);
    r->job.decode = true; r->want_pcm = true; // native format: the tail is taken from the staging region's floats
    r->r.max_steps = n; r->r.n_prompt = 0; r->r.sampler.temperature = 0.0f;
    r->codes.assign(codes, codes + (size_t)n * 16); r->fed = n;
    r->t_submit = now_ms();
    std::lock_guard<std::mutex> lk(mu_);
    Q3_CHECK(pres_.live() < Q3TTS_MAX_PREAMBLES && !pre_tail_free_.empty(), "Q3TTS_MAX_PREAMBLES preambles are live: release one first");
    const int pid = pres_.add(n);
    pres_.at(pid).payload.tail = pre_tail_free_.back(); pre_tail_free_.pop_back();
    r->build_pre = pid; r->job.snapshot = true;
    enqueue(std::move(r), decode_q_);
    return pid;
}
int Engine::request_preamble(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    return req(id).pre;
}
void Engine::preamble_stats(int64_t* built, int64_t* restores, int64_t* bytes_per_snapshot) const {
    *built = pre_built_.load(); *restores = worker_ ? worker_->pre_restores.load() : 0;
    *bytes_per_snapshot = codec_ ? (int64_t)codec_->snapshot_bytes() : 0;
}

// The take rule at submit, for one request or the members of one candidate set (they share a prompt).  The stem that applies is read under
// mu_, the rows are compared outside it (a 300-row stem is 2.4 MB), and the holds are taken under mu_ again -- if the stem is still there.
void Engine::stem_match(Req* const* rs, int n_reqs, int asked) {
    int sid, n = 0, state = Q3TTS_STEM_FAILED; std::shared_ptr<const std::vector<float>> rows;
    {
        std::lock_guard<std::mutex> lk(mu_);
        sid = stem_of_request(asked, stems_.setting);
        if (sid < 0) return;
        if (auto* s = stems_.find(sid)) { n = s->n; state = s->refs.state; rows = s->payload.rows; }
    }
    const GenRequest& g = rs[0]->r;
    bool take = stem_takes(state, n, rows ? rows->data() : nullptr, g.prompt, g.n_prompt, rs[0]->score);
    if (take) {
        std::lock_guard<std::mutex> lk(mu_);
        auto* s = stems_.find(sid);
        take = s && s->refs.state == Q3TTS_STEM_READY && s->payload.store;
        for (int i = 0; take && i < n_reqs; i++) {
            stems_.hold(sid);
            rs[i]->stem = sid; rs[i]->stem_held = true; rs[i]->n_skip = n; rs[i]->stem_store = s->payload.store;
        }
    }
    if (!take) stem_miss_ += n_reqs;
}
int Engine::stem_create(const float* rows, int n) {
    int live = 0;
    { std::lock_guard<std::mutex> lk(mu_); live = stems_.live(); }
    if (const char* why = stem_refusal(rows, n, p_.max_prompt, live, talker_->ggml_mode())) throw Error(why);
    std::unique_ptr<Req> r(new Req());
    r->stem_rows.reset(new std::vector<float>(rows, rows + (size_t)n * Q3_EMBD));
    r->r.prompt = r->stem_rows->data(); r->r.n_prompt = n; r->r.max_steps = 0; r->r.sampler.temperature = 0.0f;
    r->r.trail = r->trail_own.data(); r->r.prefix = r->prefix_own.data();
    r->t_submit = now_ms();
    std::lock_guard<std::mutex> lk(mu_);
    Q3_CHECK(stems_.live() < Q3TTS_MAX_STEMS, "Q3TTS_MAX_STEMS stems are live: release one first");
    const int sid = stems_.add(n);
    stems_.at(sid).payload.rows = r->stem_rows;
    r->build_stem = sid;
    enqueue(std::move(r), pending_);
    return sid;
}
void Engine::request_stem(int64_t id, int* stem_id, int* rows_reused) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    *stem_id = r.stem; *rows_reused = r.n_skip;
}
Engine::StemStats Engine::stem_stats() const {
    StemStats s;
    s.built = stem_built_.load(); s.restores = stem_restores_.load(); s.rows_skipped = stem_rows_.load(); s.pages_copied = stem_pages_.load();
    s.mismatches = stem_miss_.load(); s.bytes_held = stem_bytes_.load();
    return s;
}

void Engine::fetch_logprobs(int64_t id, float* out, int frame_off, int max_frames, int* got_frames) {
    std::lock_guard<std::mutex> lk(mu_);
    const Req& r = req(id);
    Q3_CHECK(r.r.logprobs || r.score, "the request does not record log-probabilities (q3tts_engine_set_logprobs was off when it was submitted)");
    int nf = 0;
    if (out && frame_off >= 0 && frame_off < r.fed && max_frames > 0) {
        nf = std::min(max_frames, r.fed - frame_off);
        std::copy(r.lp.begin() + (size_t)frame_off * Q3_LOGPROB_COLS, r.lp.begin() + (size_t)(frame_off + nf) * Q3_LOGPROB_COLS, out);
    }
    if (got_frames) *got_frames = nf;
}

bool Engine::wait(int64_t id, double timeout_ms) {
    const double t0 = now_ms();
    uint64_t seen = 0;
    for (;;) {
        {
            std::unique_lock<std::mutex> lk(mu_);
            if (req_ended(req(id).state)) return true;
            if (timeout_ms >= 0 && now_ms() - t0 > timeout_ms) return false;
            if (driver_on_) { cv_.wait_for(lk, std::chrono::milliseconds(5)); continue; }
            // every live slot waits for text: no busy loop until another thread submits or appends
            if (stalled_idle_ && wake_ == seen) { cv_.wait_for(lk, std::chrono::milliseconds(5)); continue; }
            seen = wake_;
        }
        step();
    }
}

void Engine::release(int64_t id) {
    std::lock_guard<std::mutex> lk(mu_);
    Req& r = req(id);
    Q3_CHECK(req_ended(r.state), "request still in flight");
    if (r.ev_admit) (void)hipEventDestroy(r.ev_admit);
    reqs_.erase(id);
}

void Engine::start_driver() {
    std::lock_guard<std::mutex> lk(mu_);
    if (driver_on_) return;
    driver_on_ = true; driver_stop_ = false;
    driver_ = std::thread([this] {
        try {
            Q3_HIP(hipSetDevice(dev_));
            for (;;) {
                uint64_t seen;
                { std::lock_guard<std::mutex> lk(mu_); seen = wake_; }
                const bool busy = step();
                std::unique_lock<std::mutex> lk(mu_);
                if (driver_stop_) return;
                if (!busy) cv_.wait_for(lk, std::chrono::milliseconds(1), [this] { return driver_stop_ || !pending_.empty() || !decode_q_.empty(); });
                else if (stalled_idle_) cv_.wait(lk, [&] { return driver_stop_ || wake_ != seen; }); // every live slot waits for text
            }
        } catch (const std::exception& ex) {
            std::lock_guard<std::mutex> lk(mu_);
            for (auto& kv : reqs_) if (kv.second->state != REQ_DONE && kv.second->state != REQ_CANCELLED) { kv.second->state = REQ_FAILED; kv.second->error = ex.what(); }
            pres_.fail_building(); stems_.fail_building(); // [EXT] nothing builds them any more
            cv_.notify_all();
        }
    });
}
void Engine::stop_driver() {
    {
        std::lock_guard<std::mutex> lk(mu_);
        if (!driver_on_) return;
        driver_stop_ = true;
        cv_.notify_all();
    }
    driver_.join();
    std::lock_guard<std::mutex> lk(mu_);
    driver_on_ = false;
}

int Engine::register_voice(const Voice& v) {
    Q3_CHECK(v.spk_emb.size() == (size_t)Q3_EMBD, "speaker embedding must have 2048 values");
    std::lock_guard<std::mutex> lk(mu_);
    voices_.push_back(v);
    return (int)voices_.size() - 1;
}
const Voice& Engine::voice(int id) const {
    Q3_CHECK(id >= 0 && id < (int)voices_.size(), "unknown voice id");
    return voices_[id];
}

void Engine::generate_batch(const std::vector<GenRequest>& reqs, std::vector<GenResult>& out, bool want_pcm) {
    const int n = (int)reqs.size();
    Q3_CHECK(n >= 1, "no requests");
    Q3_CHECK(!driver_on_, "generate_batch cannot be mixed with a running scheduler thread");
    out.assign(n, GenResult());
    for (const GenRequest& g : reqs) { validate(g); Q3_CHECK(!g.open, "open trails need the submit / append interface"); } // before anything is queued
    for (const GenRequest& g : reqs) if (g.n_trail > 0) ensure_text_stream(); // the one step that can fail after validation: before queueing
    std::vector<int64_t> ids(n);
    for (int i = 0; i < n; i++) ids[i] = submit(reqs[i], want_pcm, false, false); // [EXT] a blocking batch never records log-probabilities
    double t_ar_end = 0;
    while (step()) {
        if (t_ar_end == 0 && n_active_ == 0) { std::lock_guard<std::mutex> lk(mu_); if (pending_.empty()) t_ar_end = now_ms(); }
    }
    if (t_ar_end > 0) stats.codec_ms += now_ms() - t_ar_end; // only the part of the codec work the AR loop did not hide
    for (int i = 0; i < n; i++) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            Req& r = *reqs_.at(ids[i]);
            Q3_CHECK(r.state == REQ_DONE, "request did not finish");
            out[i].codes = std::move(r.codes); out[i].n_frames = r.fed; out[i].pcm = std::move(r.pcm);
            out[i].prefill_ms = r.prefill_ms; out[i].first_chunk_ms = r.first_chunk_ms; out[i].total_ms = r.t_done - r.t_submit;
        }
        release(ids[i]);
    }
}

} // namespace q3
