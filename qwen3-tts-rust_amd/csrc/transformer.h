// transformer.h -- device-resident Qwen3-style decoder (talker / code predictor) driven from embeddings.
// Replaces the llama.cpp objects behind LlamaModel / LlamaContext (/root/reference/src/models/llama/mod.rs:326-513).
#pragma once
#include "q3_common.h"
#include "gguf.h"
#include "kernels.h"
#include "ggml_mode.h"
#include <memory>

namespace q3 {

struct TfHparams {
    std::string arch;
    int n_embd = 0, n_layer = 0, n_head = 0, n_kv = 0, n_ff = 0, n_vocab = 0;
    float eps = 1e-6f, rope_base = 1e6f;
    int32_t mrope_sec[4] = {0, 0, 0, 0};
};

// The attention forms of spec S7 (S4' per-head RMSNorm, S5 M-RoPE, S6 f16 KV append, causal GQA softmax.V), numbered as q3tts.h's
// Q3TTS_ATTN_*: UNFUSED = k_qk_rope_append + k_attention, FUSED = k_attention_fused, SHORT1 / SHORT2 = k_attention_short<1|2>,
// GGML = k_gg_qk_rope_append + k_gg_attention (the Q3_SPEC=ggml arithmetic).
enum AttnForm { ATTN_UNFUSED = 1, ATTN_FUSED = 2, ATTN_SHORT1 = 3, ATTN_SHORT2 = 4, ATTN_GGML = 5 };
struct AttnPlanIn {
    int ntok = 1;
    bool fused = true; int fused_max_tok = 8;   // Transformer::fused and the 5-launch layer path's token limit
    bool same_seq = false;                      // several tokens of one sequence in the step
    int short_attn_min = 0;                     // 0 = the short form is off
    int n_head = 1, n_kv = 1;
    int hpw1_max = 128;                         // short_attn_hpw1_max()
    bool float_mode = false, ggml_mode = false;
};
// host only: the form Transformer::forward runs for one step (its launches depend on nothing else)
int plan_attention(const AttnPlanIn& in);
// spec S5 RoPE tables [n_ctx][64]: cos / sin of p * base^(-i/64), in double, rounded once to f32
void build_rope_tables(float rope_base, int n_ctx, std::vector<float>& cos_out, std::vector<float>& sin_out);

class Transformer {
public:
    Transformer(const std::string& gguf_path, int n_ctx, int max_tok);
    // A second execution context over the SAME device weights (read-only: repacked matrices, norms, RoPE tables are shared through a
    // reference-counted store); only the activation workspace is new.  Used for the asynchronous prefill lane: no second 1.5 GB copy.
    Transformer(const Transformer& weights_of, int max_tok);
    const TfHparams& hp() const { return hp_; }
    int n_ctx() const { return n_ctx_; }
    int max_tok() const { return max_tok_; }
    // a new activation workspace for launches of up to max_tok tokens (before the context's first launch)
    void set_max_tok(int max_tok) { max_tok_ = max_tok; alloc_workspace(); }
    // every layer matrix is a uniform Q8_0 one: the shapes the wide prompt-chunk GEMM forms take (plan_linear above 256 tokens)
    bool q8_uniform() const {
        if (float_mode_ || ggml_mode_) return false;
        for (const Layer& L : layers_) if (L.wqkv.rg_type || L.wo.rg_type || L.wgu.rg_type || L.wdown.rg_type) return false;
        return true;
    }
    size_t weight_bytes() const { return weight_bytes_; }       // repacked matmul weights (algorithmic bytes/step)
    size_t layer_weight_bytes() const { return layer_weight_bytes_; }
    size_t head_bytes_per_row() const { return (size_t)hp_.n_embd + (size_t)(hp_.n_embd / 32) * 2; }

    struct Input {
        const float* x = nullptr; int x_stride = 0;   // [ntok][x_stride] embeddings ...
        const q3_u64* idx_keys = nullptr; int idx_stride = 0; // ... or table rows selected by argmax keys: x + code(idx_keys[tok*idx_stride])*x_stride
        // optional, with idx_keys: layer 0's q/k/v rows of the same table (build_layer0_qkv), row code(idx_keys[...]) at qkv0 + code*qkv0_stride.
        // Layer 0 then runs no attention norm and no q/k/v projection; its attention and its ffn norm read the two tables through the keys.
        const float* qkv0 = nullptr; int qkv0_stride = 0;
    };
    // fused = 5 launches/layer (decode steps: every token from a different sequence, or a single sequence's
    // tokens when `same_seq_tokens` is set, in which case attention stays unfused)
    bool fused = true;
    // Runs all layers for ntok tokens.  After return (on stream): xq_/xd_ hold the quantised final-norm hidden of
    // every token; hidden_out (optional) gets the f32 final-norm hidden [ntok][n_embd].
    void forward(hipStream_t st, const Input& in, int ntok, const TokMeta& tm, const KvCache& kv, float* hidden_out);
    // logits[tok_count][nrows] = output rows [row0,row0+nrows) . final hidden of tokens [tok0, tok0+tok_count)
    void head(hipStream_t st, int tok0, int tok_count, int row0, int nrows, float* logits, int logits_stride,
              const ArgmaxEpi* am = nullptr, int nrows_valid = -1, float* hidden_out = nullptr);
    // out[rows][(n_head + 2 n_kv) * 128] = layer 0's attention norm + q/k/v projection of x's rows, bit for bit what forward() computes for that
    // input: the rows Input::qkv0 takes.  Runs in chunks of max_tok rows on this context's workspace.
    void build_layer0_qkv(hipStream_t st, const float* x, int x_stride, int64_t rows, float* out);
    void set_same_seq_tokens(bool v) { same_seq_ = v; }
    // steps of at least `min_tok` tokens (0 = never) use the single-wave attention kernel, which reads page 0 of a sequence only: the
    // caller states that no sequence ever holds more than `max_positions` positions, and that must fit one KV page (64)
    void set_short_attention(int min_tok, int max_positions) {
        Q3_CHECK(min_tok <= 0 || (max_positions >= 1 && max_positions <= 64), "the short attention form serves at most 64 positions per sequence");
        short_attn_min_ = min_tok;
    }
    // largest token count that still takes the 5-launch fused layer path (its GEMVs re-read the weights once per 4-8 token tile,
    // which is fine for a model whose weights stay cache-resident, i.e. the code predictor)
    void set_fused_max_tokens(int n) { fused_max_tok_ = n; }

    // Q3_SPEC=ggml at construction: the opt-in "ggml-CPU" arithmetic mode (ggml_mode.hip) -- every forward() / head() then runs llama.cpp's portable
    // arithmetic (as the test suite's CPU restatement of the mode has it), on raw copies of the GGUF matrices; slow by design, bit-exact with that restatement
    bool ggml_mode() const { return ggml_mode_; }
    // the attention form forward() runs for an ntok-token step under the current flags
    int attention_form(int ntok) const;

    LaunchTimer* timer = nullptr;    // optional per-GEMV-launch event timing (instrumented bench leg): whole GEMV family
    LaunchTimer* timer_gu = nullptr; // ... and the gate/up kernel alone (the dominant launch by bytes)
    // op-level access for parity tests
    const Q8Mat& mat_qkv(int l) const { return layers_[l].wqkv; }
    const Q8Mat& mat_out() const { return output_; }

private:
    void head_impl(hipStream_t st, int tok0, int tok_count, int row0, int nrows, float* logits, int logits_stride, const ArgmaxEpi* am,
                   int nrows_valid, float* hidden_out);
    struct Layer { Q8Mat wqkv, wo, wgu, wdown; FMat fqkv, fo, fgu, fdown; float *attn_norm, *q_norm, *k_norm, *ffn_norm; };
    FMat make_fmat(const Gguf& g, const std::vector<std::string>& names, int K_expect);
    // The layer walk.  One forward() = one Pass: what the launch choice of every step depends on, computed once.
    struct Pass { hipStream_t st; int ntok; const TokMeta& tm; const KvCache& kv; int af /* AttnForm */; bool fused /* 5 launches per layer */, wgnorm /* LIN_NORM_WG */; };
    void norm(const Pass& s, const NormPro& a);                         // residual add + RMSNorm + quantise, as its own launch
    void linear(const Pass& s, const Q8Mat& w, const FMat& fw, const float* xf, const int8_t* xq, const uint16_t* xd, float* out);
    void qkv(const Pass& s, const Layer& L, const NormPro& a);          // attention norm + q/k/v projection -> qkv_
    void attention(const Pass& s, const Layer& L, int l, const QkvRows& rows); // -> aq_ / ad_ (+ attf_ in float mode)
    void gate_up(const Pass& s, const Layer& L, const NormPro& b);      // ffn norm + gate/up + SwiGLU -> fq_ / fd_ (actf_ in float mode)
    bool float_mode_ = false; FMat foutput_; DevBuf<float> xnf_, attf_, actf_;
    float* scratch_logits(int) { return scratch_.p; }
    DevBuf<float> scratch_, hid_, big_logits_;
    void gemv(hipStream_t st, const Q8Mat& w, int row0, int nrows, const int8_t* xq, const uint16_t* xd, float* out,
              int out_stride, int ntok);
    // looks the tensors up in the GGUF, plans the layout (wlayout.h) and builds it into a new blob
    Q8Mat make_mat(const Gguf& g, const std::vector<std::pair<std::string, int>>& rows /* tensor, first row */, int N, int K);
    float* load_f32(const Gguf& g, const std::string& name, int64_t n_expect);
    TfHparams hp_;
    int n_ctx_ = 0, max_tok_ = 0;
    std::vector<Layer> layers_;
    Q8Mat output_;
    float* output_norm_ = nullptr;
    struct WeightStore { // device memory shared by every context of one model
        std::vector<DevBuf<uint8_t>> blobs; DevBuf<float> rope_cos, rope_sin; DevBuf<int32_t> d_mrope;
    };
    std::shared_ptr<WeightStore> ws_;
    std::vector<DevBuf<uint8_t>>& blobs_ = ws_init()->blobs;
    size_t weight_bytes_ = 0, layer_weight_bytes_ = 0;
    DevBuf<float>& rope_cos_ = ws_->rope_cos; DevBuf<float>& rope_sin_ = ws_->rope_sin;
    DevBuf<int32_t>& d_mrope_ = ws_->d_mrope;
    WeightStore* ws_init() { if (!ws_) ws_ = std::make_shared<WeightStore>(); return ws_.get(); }
    void alloc_workspace();
    // activations
    DevBuf<float> h_, h2_, parts_o_, parts_d_, qkv_, qrot_, gu_;
    bool same_seq_ = false; int short_attn_min_ = 0; int fused_max_tok_ = 8; bool last_fused_ = false; int last_ntok_ = 0;
    DevBuf<int8_t> xq_, aq_, fq_;
    DevBuf<uint16_t> xd_, ad_, fd_;
    int nparts_d_ = 1;
    // ---- ggml-arithmetic mode ----
    struct GgLayer { GgMat wq, wk, wv, wo, gate, up, down; };
    bool ggml_mode_ = false;
    std::vector<GgLayer> gg_layers_;
    GgMat gg_output_;
    GgMat gg_load(const Gguf& g, const std::string& name, int n_expect, int k_expect);
    void forward_ggml(hipStream_t st, const Input& in, int ntok, const TokMeta& tm, const KvCache& kv, float* hidden_out);
    void gg_linear(hipStream_t st, const GgMat& w, int row0, int nrows, const float* x, float* out, int out_stride, int ntok); // quantise x for w, then the dots
    GgAct gg_act_{};
    DevBuf<int8_t> gg_q8_, gg_qk_; DevBuf<uint16_t> gg_d8_; DevBuf<float> gg_dk_, gg_xn_, gg_att_, gg_scores_, gg_act_f_; DevBuf<int16_t> gg_bs_;
};

// The one builder of a device Q8Mat: the blob wlayout.h planned, filled from the host GGUF rows raw[i] of L.tensors[i]; `blob` owns the memory.
// Transformer::make_mat and the parity ops all come through here.
Q8Mat build_q8mat(const WLayout& L, const void* const* raw, DevBuf<uint8_t>& blob);
// for the parity ops: one Q8_0 tensor in the uniform layout (any n), and nw stacked tensors in the row-group layout (forced, also when all are Q8_0)
Q8Mat q8mat_from_host(const void* raw_q8_0, int n, int k, DevBuf<uint8_t>& storage);
Q8Mat kqmat_from_host(const void* const* raw, const int32_t* types, const int32_t* rows, int nw, int k, DevBuf<uint8_t>& storage);

// simple paged KV pool (pages of 64 positions) -- "paged KV cache sized for 288 GB HBM3E"
class KvPool {
public:
    KvPool(int n_layer, int n_kv, int n_pages, int n_seq, int max_pages_per_seq);
    ~KvPool();
    KvPool(const KvPool&) = delete; KvPool& operator=(const KvPool&) = delete;
    KvCache view() const;
    // host-side page accounting
    int alloc_page();
    void free_page(int p);
    void assign(int seq, int logical_page, int physical_page); // updates host + device table
    void ensure(int seq, int n_positions);                      // make sure pages for [0,n_positions) exist
    void ensure(int seq, int n_positions, hipStream_t st);      // same; the new part of the table row is uploaded asynchronously on `st`
    void release(int seq);
    int pages_free() const { return (int)free_.size(); }
    int page(int seq, int logical_page) const { return table_[(size_t)seq * max_pages_ + logical_page]; }
    size_t bytes() const { return (k_.n + v_.n) * 2; }
private:
    int grow(int seq, int n_positions); // host table only: takes the missing pages, returns the first new logical page
    int n_layer_, n_kv_, n_pages_, n_seq_, max_pages_;
    DevBuf<uint16_t> k_, v_;
    DevBuf<int32_t> d_table_;
    int32_t* table_ = nullptr; // pinned host mirror of the page table
    std::vector<int> free_;
    std::vector<int> used_pages_; // per seq count
};

} // namespace q3
