// kernels.h -- launch API of the hand-written gfx950 kernels for the AR decode path.
// Every kernel implements the arithmetic of include/q3tts_spec.h exactly (bit-identical to oracle/).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <map>
#include <mutex>
#include <vector>
#include "wlayout.h"
#include "q3_common.h"

namespace q3 {

// Q8_0 matrix repacked for coalesced 1-KiB wave loads (see weights.cpp / DESIGN.md "HBM layout"):
//   qs : [N/32][K/32][2 halves][32 rows][16 B]   int8 quants, one 1-KiB tile per (row-group, block)
//   sc : [N/32][K/256][32 rows][8]               f16 block scales, one 16-B vector per (row, segment)
struct Q8Mat {
    const uint8_t* qs = nullptr;
    const uint16_t* sc = nullptr;
    int N = 0;      // logical rows
    int Npad = 0;   // rows padded to 32
    int K = 0;
    // K-quant rows (Q5_K / Q6_K) stay PACKED in HBM and are unpacked in registers in front of the int8 dot products.  A matrix with K-quant
    // row groups carries the ggml type and the byte offset (in 16-B units) of every 32-row group; per (row group, 256-segment):
    //   nibble plane   [8 blocks][2 halves][32 rows][8 B]   low 4 bits; byte b of word w holds weights 8w+b (low nibble) and 8w+4+b (high nibble) of the half
    //   high plane     Q5_K: [32 rows][8 blocks][4 B]        bit 8b+J of the word = bit 4 of weight 4J+b of the block
    //                  Q6_K: [32 rows][8 blocks][2][4 B]     the same for bit 4 (word 0) and bit 5 (word 1); values are stored +32 (unsigned 6 bit)
    // = 0.625 / 0.75 B per weight (+ 0.125 of scales and metadata), against 1.125 for the int8 planes round 1 expanded them to.
    // Metadata: one 16-B vector per (row, segment): Q5_K = {sc[8], m[8]} u8 with d,dmin in sc[0..1]; Q6_K = 16 i8 sub-block scales with d in sc[0].
    const uint8_t* rg_type = nullptr;   // [Npad/32], null => all Q8_0 (uniform 1-KiB tiles)
    const uint32_t* rg_off = nullptr;   // [Npad/32] offset of the row group's quants from qs in 16-B units (K-quant matrices only)
    const uint8_t* meta = nullptr;      // [N/32][K/256][32 rows][16 B]
    size_t qbytes = 0;                  // bytes of the quant planes as stored (0 => Npad*K)
    // The same map by tensor, in the kernel arguments (a fused matrix is at most 3 tensors: q, k, v): row groups [part_rg0[i], part_rg0[i+1])
    // have type part_type[i] and start at qs + 16 * part_off[i].  Kernels take type and address from here -- scalar loads of the argument
    // block -- because reading rg_type / rg_off first would put a dependent global load (~1.5 us) in front of the whole weight stream.
    // (plain fields, not arrays: selecting from an argument array makes the compiler copy the arguments to scratch and index them there)
    int nparts = 0; int p1_rg0 = 0x7fffffff, p2_rg0 = 0x7fffffff; int p0_type = 0, p1_type = 0, p2_type = 0; uint32_t p0_off = 0, p1_off = 0, p2_off = 0;
    size_t bytes() const { return (qbytes ? qbytes : (size_t)Npad * K) + (size_t)Npad * (K / 32) * 2 + (meta ? (size_t)Npad * (K / 256) * 16 : 0); }
};
// (row-group sizes, section order and the tensor map: wlayout.h)

// Per-token routing for batched steps (one entry per token row of the activation matrix)
struct TokMeta {
    const int32_t* seq;    // [ntok] sequence slot (page-table row)
    const int32_t* slot;   // [ntok] cache position this token is written to (= #cached before it)
    const int32_t* pos;    // [ntok][4] M-RoPE position streams (engine.rs:306-314)
    // Uniform form (the code predictor's passes: token t is sequence t, every token sits at the same position p in all four streams,
    // engine.rs:316-318): a value >= 0 replaces the three arrays, which removes two dependent global loads from the attention kernels.
    int uniform_pos = -1;
    __device__ __forceinline__ int seq_of(int tok) const { return uniform_pos >= 0 ? tok : seq[tok]; }
    __device__ __forceinline__ int slot_of(int tok) const { return uniform_pos >= 0 ? uniform_pos : slot[tok]; }
    __device__ __forceinline__ int pos_of(int tok, int stream) const { return uniform_pos >= 0 ? uniform_pos : pos[(size_t)tok * 4 + stream]; }
};

struct KvCache {           // paged f16 KV cache (pages of 64 positions)
    uint16_t* k;           // [page][layer][kvh][16 dchunks][64 pos][8]
    uint16_t* v;           // [page][layer][kvh][64 pos][128]
    const int32_t* page_table; // [n_seq][max_pages]; null = identity (sequence s owns page s, single-page contexts)
    int max_pages;
    int n_layer, n_kv;
    __host__ __device__ size_t page_stride() const { return (size_t)n_layer * n_kv * 8192; } // halfs per page (per K or V)
    __host__ __device__ size_t layer_stride() const { return (size_t)n_kv * 8192; }
    __device__ __forceinline__ int page_of(int seq, int logical) const { return page_table ? page_table[(size_t)seq * max_pages + logical] : seq; }
};

// out[(sseg*ntok + tok)*out_stride + r] = super-segment partial of row (row0+r) . x[tok]      (spec S3)
// batched steps: gate/up GEMM on the matrix cores with the SwiGLU + quantisation epilogue; false = shape not supported (caller falls back)
bool launch_gateup_mfma(hipStream_t st, const Q8Mat& wgu, int ff, const int8_t* xq, const uint16_t* xd, int8_t* aq, uint16_t* ad, int ntok);
void launch_gemv_q8(hipStream_t st, const Q8Mat& w, int row0, int nrows, const int8_t* xq, const uint16_t* xd,
                    float* out, int out_stride, int ntok, int lpr_hint = 0);

// h = h_in (+ sum of nparts partial slabs, in order); optional store h_out; xn = rmsnorm(h)*g (spec S4);
// quantise to int8 blocks (spec S2).  h_in may be indirect: row idx[tok] of a table (idx != nullptr).
struct NormArgs {
    const float* h_in; int h_stride;            // [ntok][h_stride]
    const int32_t* idx; int idx_stride;         // optional: h row = h_in + idx[tok*idx_stride]*h_stride
    const unsigned long long* idx_keys;         // optional: same, row selected by an argmax key (low word = ~index)
    const float* parts; int nparts; int parts_stride; // [p][ntok][parts_stride]
    float* h_out;                               // optional [ntok][d]
    const float* g; float eps; int d;
    int8_t* xq; uint16_t* xd;                   // [ntok][d], [ntok][d/32]
    float* xn_out;                              // optional [ntok][d] (final-norm hidden)
};
void launch_rmsnorm_quant(hipStream_t st, const NormArgs& a, int ntok);

// The q/k/v rows an attention front end reads: token t's row is base + t*stride, or -- keys set -- row code(keys[t*key_stride]) of a table
// (the code predictor's layer-0 rows, which depend on the code alone and are built once at load).  Null keys is the plain addressing.
struct QkvRows {
    const float* base = nullptr;
    const unsigned long long* keys = nullptr;   // argmax keys (low word = ~index)
    int stride = 0, key_stride = 0;             // (pointers first: 24 bytes, so the kernels' next arguments stay among the preloaded ones)
    QkvRows() = default;
    QkvRows(const float* b, int s, const unsigned long long* k = nullptr, int ks = 0) : base(b), keys(k), stride(s), key_stride(ks) {}
    __device__ __forceinline__ const float* row(int tok) const {
        return base + (size_t)(keys ? (int)(~(uint32_t)keys[(size_t)tok * key_stride]) : tok) * stride;
    }
};

// per-head q/k RMSNorm + NeoX M-RoPE; q -> qrot f32; k,v -> f16 paged cache (spec S4',S5,S6)
void launch_qk_rope_append(hipStream_t st, const QkvRows& qkv, const float* parts_unused, int n_head, int n_kv,
                           const float* q_norm_w, const float* k_norm_w, float eps, const float* rope_cos,
                           const float* rope_sin, int n_ctx, const int32_t* mrope_sec /*device [4]*/, const TokMeta& tm,
                           const KvCache& kv, int layer, float* qrot, int ntok);

// causal GQA attention over the paged cache (spec S7) + int8 quantisation of the output
void launch_attention(hipStream_t st, const float* qrot, int n_head, int n_kv, const TokMeta& tm, const KvCache& kv,
                      int layer, float* att /*optional [ntok][n_head*128]*/, int8_t* aq, uint16_t* ad, int ntok);

// a = silu(g)*u over gate/up slabs, quantise (spec S8,S2). gu layout: [ntok][2*ff] with gate first.
void launch_swiglu_quant(hipStream_t st, const float* gu, int ff, int8_t* aq, uint16_t* ad, int ntok);

// first-max argmax over logits[tok][start..end) with strict '>' (llama/mod.rs:690-701); mask index -> -inf
void launch_argmax(hipStream_t st, const float* logits, int stride, int start, int end, const int32_t* mask_per_tok,
                   int32_t* out, int out_stride, int add, int ntok);

// assets_manager.rs:383-399 : out[o] = b[o] + sum_i x[i]*W[o][i]  (mul then add, ascending i).  The two device layouts of the row-major
// weight W [n_out][n_in], built on the host: Wt [n_in][n_out] (k_project_table) and Wblk [ceil(n_out/16)][n_in][16] (k_project_mt; the columns
// of a partial last block are zero, and launch_project_blk refuses such a width)
inline std::vector<float> project_wt(const float* w, int n_in, int n_out) {
    std::vector<float> wt((size_t)n_in * n_out);
    for (int o = 0; o < n_out; o++)
        for (int i = 0; i < n_in; i++) wt[(size_t)i * n_out + o] = w[(size_t)o * n_in + i];
    return wt;
}
inline std::vector<float> project_wblk(const float* w, int n_in, int n_out) {
    std::vector<float> wb((size_t)((n_out + 15) / 16) * 16 * n_in, 0.0f);
    for (int o = 0; o < n_out; o++)
        for (int i = 0; i < n_in; i++) wb[((size_t)(o / 16) * n_in + i) * 16 + (o % 16)] = w[(size_t)o * n_in + i];
    return wb;
}
// batched form over table rows, used once at load to pre-project the codec tables (the same chain, over Wt)
void launch_project_table(hipStream_t st, const float* table, int64_t rows, const float* Wt, const float* b, int n_in,
                          int n_out, float* out);

void launch_argmax_keys(hipStream_t st, const float* logits, int stride, int n, const int32_t* mask_per_tok, unsigned long long* keys,
                        int key_stride, int ntok);


void launch_copy_f32(hipStream_t st, const float* src, float* dst, size_t n);
// per-device kernel attribute opt-ins (dynamic LDS above 64 KiB); call once per device outside any stream capture
void init_kernel_attributes();

// ---- 16/32-bit float weights (bf16 / f16 / f32 files): f32 activations, no activation quantisation (spec S3 float form:
// 8-element fma sub-chains, block = (c0+c1)+(c2+c3), blocks added in order inside a segment, segments / super-segments in order)
// w: row-major [N][K]; wt: the same elements tiled [ceil(N/64)][K/8][64][8] for k_gemm_float_mfma (rows past N are zero)
struct FMat { const void* w = nullptr; const void* wt = nullptr; int type = 0; int N = 0, K = 0; size_t bytes() const { return (size_t)N * K * (type == 0 ? 4 : 2); } };
void launch_gemv_float(hipStream_t st, const FMat& w, int row0, int nrows, const float* x, int x_stride, float* out, int out_stride, int ntok);
bool launch_gateup_float(hipStream_t st, const FMat& wgu, int ff, const float* x, int x_stride, float* act, int ntok);
void launch_tile_float(hipStream_t st, const void* w, void* wt, int type, int N, int K);
void launch_swiglu_f32(hipStream_t st, const float* gu, int ff, float* out, int ntok);

// ------------------------------- fused decode-step kernels (kernels_fused.hip) -------------------------------
typedef unsigned long long q3_u64;
// prologue of the fused GEMVs: h = h_in (+ parts); RMSNorm; quantise (spec S9,S4,S2)
struct NormPro {
    const float* h_in; int h_stride;
    const q3_u64* idx_keys; int idx_stride;     // optional: row = h_in + code(idx_keys[tok*idx_stride]) * h_stride
    const float* parts; int nparts; int parts_stride; size_t parts_slab; // slab p at parts + p*parts_slab, row tok at + tok*parts_stride
    float* h_out;                               // optional [ntok][d]; MUST NOT alias h_in (other workgroups still read it)
    const float* g; float eps;
    float* xn_out;                              // optional [ntok][d]
};
// epilogue of the head GEMV: first-max argmax through one 64-bit atomicMax per workgroup and token
struct ArgmaxEpi {
    // keys[tok*key_stride], pre-armed with pack_key(-inf, 0).  A row takes part when it is valid, not the masked index and its logit is > -inf
    // (NaN never does); among those the first maximum wins, as the oracle's greedy pick.  A token with no such row keeps the armed key: code 0,
    // whatever idx_add is.  The oracle returns `start` there; the engine passes idx_add = 0 with slice-relative codes, where the two agree.
    q3_u64* keys; int key_stride;
    const int32_t* mask_per_tok;                // optional: index excluded from the argmax (EOS masking)
    int idx_add;                                // added to the row index (0: slice-relative codes)
};
void launch_gemv_q8_norm(hipStream_t st, const Q8Mat& w, int row0, int nrows, const NormPro& a, float* out, int out_stride,
                         int ntok, const ArgmaxEpi* am);
void launch_rmsnorm_quant_wg(hipStream_t st, const NormPro& a, int d, int8_t* xq, uint16_t* xd, int ntok);
// the same norm as k_rmsnorm_quant's arguments: slabs are ntok * parts_stride apart there, and the row index may be a plain int32 (idx)
inline NormArgs norm_args(const NormPro& p, int d, int8_t* xq, uint16_t* xd, const int32_t* idx = nullptr) {
    return NormArgs{p.h_in, p.h_stride, idx, p.idx_stride, p.idx_keys, p.parts, p.nparts, p.parts_stride, p.h_out, p.g, p.eps, d, xq, xd, p.xn_out};
}
void launch_gateup_swiglu(hipStream_t st, const Q8Mat& wgu, int ff, const NormPro& a, int8_t* aq, uint16_t* ad, int ntok);
void launch_attention_fused(hipStream_t st, const QkvRows& qkv, int n_head, int n_kv, const float* q_norm_w,
                            const float* k_norm_w, float eps, const float* rope_cos, const float* rope_sin, int n_ctx,
                            const int32_t* mrope_sec, const TokMeta& tm, const KvCache& kv, int layer, int8_t* aq, uint16_t* ad,
                            int ntok);
// k_attention_short<hpw>: hpw = q heads per wave (1 or 2); needs n_head == 2*n_kv and every slot < 64 (page 0 of the sequence only)
void launch_attention_short(hipStream_t st, int hpw, const QkvRows& qkv, int n_head, int n_kv, const float* q_norm_w,
                            const float* k_norm_w, float eps, const float* rope_cos, const float* rope_sin, int n_ctx,
                            const int32_t* mrope_sec, const TokMeta& tm, const KvCache& kv, int layer, int8_t* aq, uint16_t* ad, int ntok,
                            float* att = nullptr /*optional f32 rows [ntok][n_head*128]*/);
// largest token count for which the engine runs k_attention_short<1> (Q3_SHORT_ATTN_HPW1_MAX, default 128); above it <2>
int short_attn_hpw1_max();
void launch_project_blk(hipStream_t st, const float* x, int x_stride, const float* Wblk /*[n_out/16][n_in][16]*/, const float* b,
                        int n_in, int n_out, float* out, int out_stride, int ntok);
// [EXT] streaming-text feedback (q3tts_spec.h): slot b's last addend is text(ids[b*ids_stride + f]) while f = n_frames[b] < n_trail[b],
// tts_pad after; text() reads table rows [0, rows) and computes the fallback row in-kernel for any other id
// ---- linear-layer dispatch: one host-only rule (plan_linear) that every launcher above and q3tts_op_linear follow ----
// The ops and forms mirror include/q3tts.h's Q3TTS_LOP_* / Q3TTS_LIN_* (same numbers).
enum LinearOp { LOP_GEMV = 0, LOP_GATEUP = 1, LOP_NORM = 2, LOP_NORM_GEMV = 3, LOP_NORM_ARGMAX = 4, LOP_NORM_GATEUP = 5, LOP_F_GEMV = 6,
                LOP_F_GATEUP = 7 };
enum LinearForm { LIN_AUTO = 0, LIN_GEMV_Q8 = 1, LIN_GEMM_Q8_TOK = 2, LIN_GEMM_Q8_MFMA = 3, LIN_GEMM_Q8_TILE1 = 4, LIN_GEMV_KQ = 5,
                  LIN_GEMM_KQ_MFMA = 6, LIN_GU_Q8_TILE1 = 7, LIN_GU_Q8_MFMA = 8, LIN_GU_KQ_MFMA = 9, LIN_GU_UNFUSED = 10, LIN_NORM = 11,
                  LIN_NORM_WG = 12, LIN_GEMV_NORM = 13, LIN_GEMV_NORM_ARGMAX = 14, LIN_GU_SWIGLU_NORM = 15, LIN_F_GEMV = 16, LIN_F_MFMA16 = 17,
                  LIN_F_MFMA = 18, LIN_F_GU_MFMA16 = 19, LIN_F_GU_UNFUSED = 20, LIN_GEMM_Q8_WIDE = 21, LIN_GU_Q8_WIDE = 22 };
bool prefill_wide(); // Q3_PREFILL_WIDE != 0 (the default): prompt chunks of 512 tokens on the wide int8 GEMM forms
struct LinearPlanIn {
    int op = LOP_GEMV;
    int K = 0, row0 = 0, nrows = 0, ntok = 0, ff = 0;
    int wts = 0;          // quantised: wslice_ts of the matrix (0 = all Q8_0, 8 / 13 / 14 = one K-quant-file type, -1 = mixed); float: 0 / 1 / 30
    bool kq = false;      // quantised matrix built from K-quant-file tensors (Q8Mat::rg_type != null)
    int kq_parts = 0;     // Q8Mat::nparts
    bool has_wt = false;  // float: the tiled copy exists
    int out_stride = 0; uintptr_t out_addr = 0;   // address bits only (alignment tests)
    int x_stride = 0; uintptr_t x_addr = 0;
    uintptr_t aq_addr = 0;
    int lpr_hint = 0;     // launch_gemv_q8's lpr_hint (0 = none)
    bool fused = true;    // LOP_GATEUP: the Transformer's `fused` switch (false: GEMV + k_swiglu_quant always)
};
struct LinearPlan { int form = LIN_AUTO, lpr = 0, mt = 0, z = 0, nseg = 0; };
LinearPlan plan_linear(const LinearPlanIn& in);
// the launch of one planned form (no dispatch left: the plan's form, LPR, MT and z tiles are used as given)
void run_gemv_q8(hipStream_t st, const LinearPlan& p, const Q8Mat& w, int row0, int nrows, const int8_t* xq, const uint16_t* xd, float* out,
                 int out_stride, int ntok);
void run_gateup_q8(hipStream_t st, const LinearPlan& p, const Q8Mat& wgu, int ff, const int8_t* xq, const uint16_t* xd, int8_t* aq, uint16_t* ad,
                   int ntok);
void run_gemv_q8_norm(hipStream_t st, const LinearPlan& p, const Q8Mat& w, int row0, int nrows, const NormPro& a, float* out, int out_stride,
                      int ntok, const ArgmaxEpi* am);
void run_gateup_swiglu(hipStream_t st, const LinearPlan& p, const Q8Mat& wgu, int ff, const NormPro& a, int8_t* aq, uint16_t* ad, int ntok);
void run_gemv_float(hipStream_t st, const LinearPlan& p, const FMat& w, int row0, int nrows, const float* x, int x_stride, float* out,
                    int out_stride, int ntok);
void run_gateup_float(hipStream_t st, const LinearPlan& p, const FMat& wgu, int ff, const float* x, int x_stride, float* act, int ntok);
LinearPlanIn linear_plan_in(int op, const Q8Mat& w, int row0, int nrows, int ntok);
struct TextTrail {
    const int32_t* n_frames = nullptr; const int32_t* n_trail = nullptr; const int32_t* ids = nullptr; int ids_stride = 0;
    const float* table = nullptr; int64_t rows = 0;
};
// trail == null: the reference's feedback (every slot adds tts_pad)
void launch_feedback_keys(hipStream_t st, const float* const* tables, const int64_t* table_rows, const q3_u64* keys, int key_stride,
                          const float* tts_pad, float* out, int ntok, const TextTrail* trail = nullptr);
// [EXT] resume (q3tts_spec.h): rows [n][2048] = the feedback rows of codes [n][16] (device, int32).  ids (device) holds the trailing id of
// rows [0, n_ids); the rows after it, and every row when ids is null, add tts_pad
struct FeedbackIds { const int32_t* ids = nullptr; int n_ids = 0; const float* table = nullptr; int64_t rows = 0; };
void launch_feedback_codes(hipStream_t st, const float* const* tables, const int64_t* table_rows, const int32_t* codes, const float* tts_pad,
                           float* out, int n, const FeedbackIds* ids = nullptr);
void launch_gather_rows_keys(hipStream_t st, const float* table, int64_t rows, const q3_u64* keys, int key_stride, int row_len,
                             float* dst, int ntok);
struct AdvanceKeysArgs {
    int B; int32_t *finished, *n_frames; const int32_t* max_frames; q3_u64* keys; q3_u64* next_key0; int32_t* hist; int hist_stride;
    int32_t *t_slot, *t_pos;
};
void launch_advance_keys(hipStream_t st, const AdvanceKeysArgs& a);
// [EXT] live text append (q3tts_spec.h): slot b waits this frame when
//   !finished[b] && n_frames[b] < max_frames[b] && open[b] && n_frames[b] >= n_trail[b]
// k_stall_save (the gated frame's first launch) copies a waiting slot's hidden row and talker / predictor draw counters to the save area;
// the gated k_advance_keys (the frame's last launch) copies them back, keeps keys[b][0], re-arms keys 1..15 and next_key0, and leaves
// n_frames / finished / history / positions alone.  Active slots take the plain advance.
struct StallArgs {
    const int32_t* open = nullptr; const int32_t* n_trail = nullptr;
    float* hidden = nullptr; uint32_t* draws = nullptr; uint32_t* pdraws = nullptr; // live state ([B][2048], [B], [B])
    float* save_hidden = nullptr; uint32_t* save_draws = nullptr;                   // save area ([B][2048], [B][2])
};
void launch_stall_save(hipStream_t st, const AdvanceKeysArgs& a, const StallArgs& s);
void launch_advance_keys_gated(hipStream_t st, const AdvanceKeysArgs& a, const StallArgs& s);

// on-device LlamaSampler::sample (sampler.hip): one workgroup per sequence over logits[b*stride + [0,n)), n <= 4096
struct SampleArgs {
    const float* logits; int stride; int n;
    const float* temperature; const int32_t* top_k; const float* top_p; // per sequence (SamplerConfig, engine.rs:13-45)
    const int32_t* mask_idx;                                            // optional per sequence: index forced to -inf
    const uint32_t* rng_key; uint32_t* draws;                           // [B][8] ChaCha12 key, [B] u32 words consumed so far
    q3_u64* out_key; int out_stride;                                    // receives pack_key(0, token)
    // [EXT] repetition penalty (k_sample only; null = off, spec "Repetition penalty"): the history of sequence b is code_0 of frames
    // [0, hist_len[b]) at hist[b*hist_stride + f*16] plus key_code(cur_key[b*cur_stride]) (the current frame; a code outside [0, n) is ignored;
    // cur_key null = no current frame)
    const float* penalty = nullptr;
    const int32_t* hist = nullptr; int hist_stride = 0; const int32_t* hist_len = nullptr;
    const q3_u64* cur_key = nullptr; int cur_stride = 0;
};
void launch_sample(hipStream_t st, const SampleArgs& a, int B);
// the code predictor's sampler: the same draw as k_sample (bit for bit, every T / top_k / top_p) for n <= 2048, without the 4096-key sort;
// the penalty / mask fields must be null
void launch_sample_pred(hipStream_t st, const SampleArgs& a, int B);

// [EXT] token log-probabilities (logprob.hip, q3tts_spec.h): out[col] = log softmax(row)[code] per row, f32, raw logits.
// One head group: row b of head h is logits[h*head_stride + b*stride + [0, n)), n <= 4096; its code is chosen[b] (plain int32, when set) or
// key_code(key[b*key_stride + h]) (the packed keys the samplers write); the value goes to column col + h, and -- extra_idx >= 0 --
// log softmax(row)[extra_idx] to column col_extra.  row_ahead: engine form only, rows past n_frames[b] the head's values belong to.
struct LogprobHead {
    const float* logits = nullptr; int stride = 0; size_t head_stride = 0; int n = 0;
    const q3_u64* key = nullptr; int key_stride = 0; const int32_t* chosen = nullptr;
    int extra_idx = -1; int col = 0, col_extra = -1; int row_ahead = 0;
};
// A launch covers n_first heads of shape p and, when t.logits is set, one more head of shape t (grid = B x heads).
// Plain form (n_frames null): row b writes out[b*out_stride + column].  Engine form: slot b writes row n_frames[b] + row_ahead of its
// out_rows rows, out[(b*out_rows + row)*out_stride + column], and only when it is live (!finished, n_frames < max_frames), does not
// wait for text (open && n_frames >= n_trail), records (record[b] != 0) and the row exists.
struct LogprobArgs {
    LogprobHead p; int n_first = 0; LogprobHead t;
    float* out = nullptr; int out_stride = 0, out_rows = 0;
    const int32_t* n_frames = nullptr; const int32_t* finished = nullptr; const int32_t* max_frames = nullptr;
    const int32_t* open = nullptr; const int32_t* n_trail = nullptr; const int32_t* record = nullptr;
};
void launch_logprob_rows(hipStream_t st, const LogprobArgs& a, int B);

// [EXT] scoring given frames (score.hip, q3tts_spec.h "scoring"): one teacher-forced predictor pass over F frames.
// Input rows out[(p*F + f)*dP + ..], p = 0..15: p = 0 copies hidden_proj[f] (the projected hidden row), p >= 1 row codes[f][p-1] of tabs[p-1]
// (tab_rows[p-1] rows of dP floats; a negative code reads row 0, a code past the table gives a zero row).  tabs / tab_rows / codes: device.
void launch_score_inputs(hipStream_t st, const float* hidden_proj, const float* const* tabs, const int64_t* tab_rows, int dP, const int32_t* codes,
                         int F, float* out);
// out[f][17] of frames f = 0..F-1 in k_logprob_rows' arithmetic: columns 0 / 16 from tlogits[f*t_stride + [0, Q3_SAMPLE_END)) at codes[f][0] /
// Q3_CODEC_EOS, column q + 1 from plogits[q*p_head_stride + f*2048 + [0, 2048)) at codes[f][q + 1]
struct ScoreRowsArgs {
    const float* tlogits = nullptr; int t_stride = 0;
    const float* plogits = nullptr; size_t p_head_stride = 0;
    const int32_t* codes = nullptr; float* out = nullptr;
};
void launch_score_rows(hipStream_t st, const ScoreRowsArgs& a, int F);

// [EXT] candidate sets (kvfork.hip, q3tts_spec.h "candidate sets"): logical pages [0, n_pages) of sequence src_seq are copied, whole and in
// both planes, into the same logical pages of the n_dst sequences dst_seqs[] (device array).  Physical page ids come from kv.page_table on
// the device (it must be set); every sequence involved must own those pages, and no two of the physical pages may coincide.
void launch_kv_fork(hipStream_t st, const KvCache& kv, int src_seq, const int32_t* dst_seqs, int n_dst, int n_pages);

// [EXT] prompt stems (kvstem.hip, q3tts_spec.h "prompt stems"): one launch for a device table of n_jobs jobs.  A job's store holds n_pages
// contiguous plane pages at k and as many at v.  Restore: store page l goes into logical page l of the sequences slots[first .. first + n_dst).
// Save: logical page l of sequence slots[first] goes into store page l.  max_pages = the largest n_pages among the jobs.  Physical page ids
// come from kv.page_table on the device (it must be set); every sequence involved must own logical pages [0, n_pages) of its job.
struct StemJob { uint16_t* k; uint16_t* v; int32_t n_pages, first, n_dst, pad; };
void launch_kv_stem(hipStream_t st, const KvCache& kv, const StemJob* jobs, int n_jobs, int max_pages, const int32_t* slots, bool save);

// [EXT] reference audio intake (intake.hip, q3tts_spec.h "reference audio intake"): decode, downmix and resampling to 24000 Hz in front
// of the encoders.  One entry per clip of a launch.
struct IntakeClipMeta {
    const unsigned char* src; // the clip's raw interleaved samples, on the device, aligned to its sample size (3-byte samples to nothing)
    float* dst;               // its n_out output samples, 16-byte aligned
    const float* tab;         // the ratio's table, phase-major [L][stride]; unused at 24000 Hz
    int32_t n, n_out;         // input frames; output samples
    int32_t L, M, stride, c;  // the ratio, floats per phase row (0: 24000 Hz, no filter), the prototype's centre
    int32_t tile, win;        // outputs per block; floats of LDS set aside for a tile's input window
    int32_t C, fmt, mix;      // channels, Q3_INTAKE_U8 .. F32, Q3_INTAKE_FIRST / MEAN
    int32_t flag_off;         // the clip's first entry of the launch's flag array, one per tile
};
struct IntakePlan;
// A device's intake state: the tables of the ratios it has met, each built and uploaded once.  intake_stage(device) is the process's one
// stage of that device; intake_run serialises its callers.
struct IntakeStage {
    explicit IntakeStage(int device);
    IntakeStage(const IntakeStage&) = delete; IntakeStage& operator=(const IntakeStage&) = delete;
    const float* table(int rate, IntakePlan* plan);   // under mu and capture_mutex(), on the stage's device
    int device;
    std::mutex mu;
    std::map<int, DevBuf<float>> tabs;
    // a call's raw clips, samples, per-tile flags and meta entries on the device: grown as calls need, kept for the next one
    DevBuf<unsigned char> in; DevBuf<float> out; DevBuf<int32_t> flags; DevBuf<IntakeClipMeta> meta;
};
IntakeStage& intake_stage(int device);
// the kernel alone: grid (tiles, n_clips); d_flags holds one int per tile of every clip, and every tile within a clip's n_out writes its own
void launch_intake(hipStream_t st, const IntakeClipMeta* d_meta, int n_clips, int tiles, int32_t* d_flags);
// host buffers in, host buffers out, synchronous: clip i's ceil(n L / M) samples go to out[i] (capacity out_cap[i] floats), their count to
// n_out[i].  Refused (intake_refusal, intake.h; a short capacity; more than 64 clips) before anything is allocated; a clip with a
// non-finite sample fails the call after the launch and before any output is copied.  A failed call writes nothing.
void intake_run(IntakeStage& s, const q3tts_intake_clip* clips, int n_clips, float* const* out, const int64_t* out_cap, int64_t* n_out);

} // namespace q3
