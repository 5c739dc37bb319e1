// ggml_mode.h -- launchers of the opt-in "ggml-CPU" arithmetic mode (ggml_mode.hip; Q3_SPEC=ggml).
#pragma once
#include "q3_common.h"
#include "kernels.h"

namespace q3 {

// the one type rule of the mode and its message (Q4_K, Q3_K, IQ4_XS, Q4_0 and Q5_0 are named: Q4_K_M, Q3_K_M, IQ4_XS, Q4_0 and Q5_0 files load in the spec arithmetic only)
inline bool gg_type_ok(int type) { return type == Q3_T_Q8_0 || type == Q3_T_Q5_K || type == Q3_T_Q6_K; }
inline std::string gg_type_msg(int type) { return "ggml mode serves Q8_0 / Q5_K / Q6_K matrices, not ggml type " + std::to_string(type) + (type == Q3_T_Q4_K ? " (Q4_K)" : type == Q3_T_Q3_K ? " (Q3_K)" : type == Q3_T_IQ4_XS ? " (IQ4_XS)" : type == Q3_T_Q4_0 ? " (Q4_0)" : type == Q3_T_Q5_0 ? " (Q5_0)" : ""); }
struct GgMat { const uint8_t* p = nullptr; int type = 0, n = 0, k = 0; size_t row_bytes = 0; }; // a GGUF matrix exactly as stored (raw blocks, row-major)
struct GgAct { int8_t* q8; uint16_t* d8; int8_t* qk; float* dk; int16_t* bs; };                 // activations as Q8_0 (per 32) and Q8_K (per 256) blocks

void gg_load_rows(hipStream_t st, const float* x, int x_stride, const int32_t* idx, int idx_stride, const unsigned long long* idx_keys, int d, float* h, int ntok);
void gg_add(hipStream_t st, float* h, const float* o, size_t n);
void gg_rmsnorm(hipStream_t st, const float* x, const float* g, int d, float eps, float* y, int ntok);
void gg_quant(hipStream_t st, const float* x, int k, const GgAct& a, int ntok);
void gg_matvec(hipStream_t st, const GgMat& w, int row0, int nrows, const GgAct& a, float* out, int out_stride, int ntok);
void gg_qk_rope_append(hipStream_t st, float* qkv, int stride, int n_head, int n_kv, const float* q_norm_w, const float* k_norm_w, float eps, const float* rope_cos,
                       const float* rope_sin, int n_ctx, const int32_t* mrope_sec, const TokMeta& tm, const KvCache& kv, int layer, int ntok);
void gg_attention(hipStream_t st, const float* qkv, int stride, int n_head, int n_kv, const TokMeta& tm, const KvCache& kv, int layer, float* att, float* scores,
                  int n_ctx, int ntok);
void gg_swiglu(hipStream_t st, const float* g, const float* u, float* y, size_t n);

} // namespace q3
