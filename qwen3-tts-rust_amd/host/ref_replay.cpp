// ref_replay.cpp -- replays /root/reference/src/tts/engine.rs:445-656 call-for-call against BOUNDARY A:
// it dlopens <cwd>/runtime/libllama.so exactly as the reference does (llama/mod.rs:152-218), resolves the same 28
// symbols, and drives them with the reference's own host-side glue (f32 project on the CPU in the reference's order,
// assets_manager.rs:383-399; greedy sampler llama/mod.rs:690-701).  Used by tests to show that the unmodified Rust
// crate, pointed at this library, would emit the oracle's codec tokens.
//   usage: ref_replay <model_quant_dir> <prompt.f32> <n_prompt> <max_steps> <codes_out.i32> [mask_eos [type_k type_v]]
// type_k / type_v: the talker context's llama_context_params.type_k / type_v (ggml type ids, llama.cpp's -ctk / -ctv); the reference leaves
// the defaults (f16), and the predictor's context keeps them here.
#include "../../include/q3tts.h"
#include "../../include/q3tts_llama.h"
#include <dlfcn.h>
#include <unistd.h>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define SYM(name) auto p_##name = (decltype(&name))dlsym(lib, #name); if (!p_##name) { fprintf(stderr, "missing symbol %s\n", #name); return 3; }

int main(int argc, char** argv) {
    if (argc < 6) { fprintf(stderr, "usage: ref_replay <quant_dir> <prompt.f32> <n_prompt> <max_steps> <codes_out> [mask_eos]\n"); return 2; }
    const std::string dir = argv[1];
    const int n_prompt = atoi(argv[3]), max_steps = atoi(argv[4]);
    const bool mask_eos = argc > 6 && atoi(argv[6]) != 0;
    char cwd[4096];
    if (!getcwd(cwd, sizeof(cwd))) return 2;
    const std::string libpath = std::string(cwd) + "/runtime/libllama.so"; // llama/mod.rs:152,195,216
    void* lib = dlopen(libpath.c_str(), RTLD_NOW | RTLD_LOCAL);
    if (!lib) { fprintf(stderr, "Failed to load libllama.so. Please ensure it is in the runtime/ directory. (%s)\n", dlerror()); return 3; }
    SYM(llama_backend_init) SYM(llama_backend_free) SYM(llama_model_default_params) SYM(llama_model_load_from_file) SYM(llama_model_free)
    SYM(llama_model_get_vocab) SYM(llama_model_n_embd) SYM(llama_model_n_head) SYM(llama_model_n_layer) SYM(llama_n_ctx) SYM(llama_n_vocab)
    SYM(llama_vocab_n_tokens) SYM(llama_vocab_eos) SYM(llama_context_default_params) SYM(llama_init_from_model) SYM(llama_free)
    SYM(llama_batch_init) SYM(llama_batch_free) SYM(llama_decode) SYM(llama_get_embeddings) SYM(llama_get_logits) SYM(llama_get_memory)
    SYM(llama_memory_clear) SYM(llama_memory_seq_rm) SYM(llama_memory_seq_pos_max) SYM(llama_sampler_init_temp) SYM(llama_sampler_sample)
    SYM(llama_sampler_free)
    (void)p_llama_n_ctx; (void)p_llama_n_vocab; (void)p_llama_batch_free; (void)p_llama_memory_clear; (void)p_llama_sampler_init_temp;
    (void)p_llama_sampler_sample; (void)p_llama_sampler_free; (void)p_llama_memory_seq_pos_max; (void)p_llama_model_n_head; (void)p_llama_model_n_layer;
    (void)p_llama_vocab_eos;
    // assets through the C ABI's host-side functions (same .so)
    auto a_open = (decltype(&q3tts_assets_open))dlsym(lib, "q3tts_assets_open");
    auto a_codec = (decltype(&q3tts_assets_codec_embedding))dlsym(lib, "q3tts_assets_codec_embedding");
    auto a_pad = (decltype(&q3tts_assets_tts_pad))dlsym(lib, "q3tts_assets_tts_pad");
    q3tts_assets* assets = nullptr;
    if (!a_open || a_open((dir + "/qwen3_assets.gguf").c_str(), &assets)) { fprintf(stderr, "assets load failed\n"); return 3; }
    // proj.weight / proj.bias straight from the file through a second tiny reader: reuse the oracle-free path
    // (the C ABI exposes project only as a device op, so read the tensors with the product's GGUF reader via q3tts_op_project? no:
    //  the reference projects on the HOST; do the same here from raw tensors)
    FILE* pf = fopen(argv[2], "rb");
    if (!pf) { perror(argv[2]); return 2; }
    std::vector<float> prompt((size_t)n_prompt * 2048);
    if (fread(prompt.data(), 4, prompt.size(), pf) != prompt.size()) { fprintf(stderr, "short prompt file\n"); return 2; }
    fclose(pf);
    auto a_proj = (int (*)(const q3tts_assets*, const float*, float*))dlsym(lib, "q3tts_assets_project_host");
    auto a_projdim = (int (*)(const q3tts_assets*))dlsym(lib, "q3tts_assets_proj_out");
    if (!a_proj || !a_projdim) { fprintf(stderr, "missing host project symbols\n"); return 3; }

    p_llama_backend_init();
    llama_model_params mp = p_llama_model_default_params();
    mp.n_gpu_layers = 99; // engine.rs:126
    llama_model* talker = p_llama_model_load_from_file((dir + "/qwen3_tts_talker.gguf").c_str(), mp);
    llama_model* pred = p_llama_model_load_from_file((dir + "/qwen3_tts_predictor.gguf").c_str(), mp);
    if (!talker || !pred) { fprintf(stderr, "Failed to load model\n"); return 4; }
    const int talker_embd = p_llama_model_n_embd(talker), pred_embd = p_llama_model_n_embd(pred);
    const int t_vocab = p_llama_vocab_n_tokens(p_llama_model_get_vocab(talker)), p_vocab = p_llama_vocab_n_tokens(p_llama_model_get_vocab(pred));
    const bool kv_types = argc > 8;
    const int type_k = kv_types ? atoi(argv[7]) : 0, type_v = kv_types ? atoi(argv[8]) : 0;
    auto mkctx = [&](llama_model* m, uint32_t n_ctx, uint32_t n_batch, bool emb, int thr, bool set_kv) { // llama/mod.rs:409-432
        llama_context_params cp = p_llama_context_default_params();
        cp.n_ctx = n_ctx; cp.n_batch = n_batch; cp.n_ubatch = 512; cp.n_seq_max = 1; cp.embeddings = emb; cp.flash_attn_type = 1;
        cp.offload_kqv = true; cp.no_perf = true; cp.n_threads = thr > 0 ? thr : 4;
        if (set_kv) { cp.type_k = (decltype(cp.type_k))type_k; cp.type_v = (decltype(cp.type_v))type_v; }
        return p_llama_init_from_model(m, cp);
    };
    llama_context* tctx = mkctx(talker, 4096, 2048, true, -1, kv_types);  // engine.rs:133
    llama_context* pctx = mkctx(pred, 512, 32, false, 4, false);          // engine.rs:136
    if (!tctx || !pctx) { fprintf(stderr, "Failed to create context\n"); return 4; }
    auto set_embd = [&](llama_batch& b, const float* e, size_t n_floats, int n_embd, const std::vector<int32_t>& pos, size_t cap) { // mod.rs:556-615
        const int n = (int)(n_floats / n_embd);
        memcpy(b.embd, e, n_floats * 4);
        memcpy(b.pos, pos.data(), std::min(pos.size(), cap) * 4);
        for (int i = 0; i < n; i++) { b.n_seq_id[i] = 1; b.seq_id[i][0] = 0; b.logits[i] = (i == n - 1) ? 1 : 0; }
        b.n_tokens = n;
    };
    auto qwen3_position = [](int start, int len) { std::vector<int32_t> p; for (int s = 0; s < 3; s++) for (int i = 0; i < len; i++) p.push_back(start + i); for (int i = 0; i < len; i++) p.push_back(0); return p; };
    const auto t_start = std::chrono::steady_clock::now();
    llama_batch tb = p_llama_batch_init(4096, talker_embd, 1);
    set_embd(tb, prompt.data(), prompt.size(), talker_embd, qwen3_position(0, n_prompt), 4096);
    if (p_llama_decode(tctx, tb) != 0) { fprintf(stderr, "Talker prefill failed\n"); return 5; }
    const auto t_prefill = std::chrono::steady_clock::now();
    llama_batch pb = p_llama_batch_init(32, pred_embd, 1);
    std::vector<int32_t> all_codes;
    int cur_pos = n_prompt;
    std::vector<float> tts_pad(2048), emb(2048), proj(pred_embd), pin((size_t)2 * pred_embd);
    a_pad(assets, tts_pad.data());
    for (int step = 0; step < max_steps; step++) {
        const int sample_idx = (cur_pos == n_prompt) ? n_prompt - 1 : 0; // :550-554
        const float* lg = p_llama_get_logits(tctx) + (size_t)sample_idx * t_vocab;
        float mv = -INFINITY; int code0 = 0;
        for (int i = 0; i < 2160 && i < t_vocab; i++) { const float v = (mask_eos && i == 2150) ? -INFINITY : lg[i]; if (v > mv) { mv = v; code0 = i; } }
        if (code0 == 2150 || code0 == 151673) break; // :558
        all_codes.push_back(code0);
        const int emb_idx = step == 0 ? n_prompt - 1 : 0; // :565
        std::vector<float> m_hidden(p_llama_get_embeddings(tctx) + (size_t)emb_idx * talker_embd, p_llama_get_embeddings(tctx) + (size_t)(emb_idx + 1) * talker_embd);
        a_proj(assets, m_hidden.data(), pin.data());
        a_codec(assets, 0, code0, emb.data());
        a_proj(assets, emb.data(), pin.data() + pred_embd);
        p_llama_memory_seq_rm(p_llama_get_memory(pctx), -1, 0, -1); // :575
        set_embd(pb, pin.data(), pin.size(), pred_embd, {0, 1}, 32);
        if (p_llama_decode(pctx, pb) != 0) { fprintf(stderr, "Predictor prefill failed\n"); return 5; }
        std::vector<std::vector<float>> step_embeds; step_embeds.push_back(emb);
        for (int q = 1; q < 16; q++) { // :587-611
            const float* pl = p_llama_get_logits(pctx);
            float bm = -INFINITY; int bi = (q - 1) * 2048;
            for (int i = (q - 1) * 2048; i < q * 2048 && i < p_vocab; i++) if (pl[i] > bm) { bm = pl[i]; bi = i; }
            const int code_q = bi - (q - 1) * 2048;
            all_codes.push_back(code_q);
            a_codec(assets, q, code_q, emb.data());
            step_embeds.push_back(emb);
            if (q < 15) {
                a_proj(assets, emb.data(), proj.data());
                set_embd(pb, proj.data(), proj.size(), pred_embd, {q + 1}, 32);
                if (p_llama_decode(pctx, pb) != 0) { fprintf(stderr, "Predictor decode failed\n"); return 5; }
            }
        }
        std::vector<float> feedback(2048, 0.0f); // :622-631
        for (auto& e : step_embeds) for (int i = 0; i < 2048; i++) feedback[i] += e[i];
        for (int i = 0; i < 2048; i++) feedback[i] += tts_pad[i];
        feedback.resize(talker_embd, 0.0f);
        set_embd(tb, feedback.data(), feedback.size(), talker_embd, qwen3_position(cur_pos, 1), 4096);
        if (p_llama_decode(tctx, tb) != 0) { fprintf(stderr, "Talker step failed\n"); return 5; }
        cur_pos++;
    }
    FILE* of = fopen(argv[5], "wb");
    fwrite(all_codes.data(), 4, all_codes.size(), of);
    fclose(of);
    const auto t_end = std::chrono::steady_clock::now();
    const double pre_ms = std::chrono::duration<double, std::milli>(t_prefill - t_start).count();
    const double loop_ms = std::chrono::duration<double, std::milli>(t_end - t_prefill).count();
    const size_t nfr = all_codes.size() / 16;
    printf("frames %zu\n", nfr);
    // Boundary A timing: the reference's own loop (17 llama_decode round trips + host projection / gathers per frame), no codec
    printf("timing prefill_ms %.2f loop_ms %.2f ms_per_frame %.3f rtf_ar_only %.4f\n", pre_ms, loop_ms, nfr ? loop_ms / nfr : 0.0, nfr ? (pre_ms + loop_ms) / (nfr * 80.0) : 0.0);
    p_llama_free(tctx); p_llama_free(pctx); p_llama_model_free(talker); p_llama_model_free(pred);
    p_llama_backend_free();
    return 0;
}
