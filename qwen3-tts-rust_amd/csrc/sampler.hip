// sampler.hip -- LlamaSampler::sample on device (/root/reference/src/models/llama/mod.rs:666-776), one workgroup per
// sequence, so that temperature > 0 decoding stays inside the per-frame hipGraph (no logits round trip to the host).
//
// Same steps, same f32 order as host_logic.cpp::Sampler::sample (the C ABI's q3tts_sampler_*):
//   T <= 0 : first-max argmax (strict >)                                                       :690-701
//   T  > 0 : stable sort descending -> top-k truncate -> e_i = exp((l_i - l_0)/T), sum in sorted order, divide
//            -> top-p: first prefix with cum >= p (inclusive), renormalise -> r = u32/2^32 from the sequence's
//            ChaCha12 stream -> first i with r < cum_i, else candidate 0                        :703-775
// The sort is a 4096-key bitonic network in LDS on (order-preserving float image, ~index) keys: descending key order
// == descending value with ties in ascending index order == the reference's stable sort.
//
// [EXT] repetition penalty (q3tts_spec.h "Repetition penalty"): with SampleArgs::penalty set, k_sample marks the sequence's code_0 history
// in an LDS bitmap and applies l < 0 ? l*p : l/p to the marked logits while it builds the sort keys (no extra launch).
//
// k_sample_pred: the same draw for the code predictor's 2048-wide passes (one launch per pass for all slots).  Instead of sorting all 4096
// keys it selects the top-k keys first -- an MSB-first radix select on the 64-bit keys (8-bit digits, LDS histogram; it stops at the first
// digit whose bin holds exactly the keys still missing, keys are unique so that happens by the last digit) -- compacts them with 64-lane
// ballots and sorts only those (bitonic over the next power of two).  The sorted candidates are the same keys in the same order as
// k_sample's first c sorted keys, and the tail (exp, sequential sum, top-p scan, draw) is the same code, so the pick is bit-identical.
#include "kernels.h"
#include "kdev.h"
#include "q3_common.h"

namespace q3 {

#define SAMPLE_NS 4096
#define SAMPLE_THREADS 1024

__device__ __forceinline__ uint32_t rotl32(uint32_t x, int n) { return (x << n) | (x >> (32 - n)); }

// word `draw % 16` of ChaCha12 block `draw / 16` (rand_chacha layout: 64-bit block counter in words 12-13, stream id 0)
__device__ uint32_t chacha12_word(const uint32_t* __restrict__ key, uint32_t draw) {
    const uint64_t counter = draw >> 4;
    uint32_t s[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                      key[4], key[5], key[6], key[7], (uint32_t)counter, (uint32_t)(counter >> 32), 0u, 0u};
    uint32_t x[16];
#pragma unroll
    for (int i = 0; i < 16; i++) x[i] = s[i];
#define Q3_QR(a, b, c, d)                                                                                        \
    x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 12);                  \
    x[a] += x[b]; x[d] = rotl32(x[d] ^ x[a], 8);  x[c] += x[d]; x[b] = rotl32(x[b] ^ x[c], 7);
    for (int r = 0; r < 6; r++) {
        Q3_QR(0, 4, 8, 12) Q3_QR(1, 5, 9, 13) Q3_QR(2, 6, 10, 14) Q3_QR(3, 7, 11, 15)
        Q3_QR(0, 5, 10, 15) Q3_QR(1, 6, 11, 12) Q3_QR(2, 7, 8, 13) Q3_QR(3, 4, 9, 14)
    }
#undef Q3_QR
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) if ((int)(draw & 15u) == i) out = x[i] + s[i];
    return out;
}

__device__ __forceinline__ float key_value(u64 k) { // inverse of pack_key's float image
    const uint32_t ord = (uint32_t)(k >> 32);
    const uint32_t b = (ord & 0x80000000u) ? (ord & 0x7FFFFFFFu) : ~ord;
    return q3_bits_f32(b);
}

__global__ void __launch_bounds__(SAMPLE_THREADS) k_sample(SampleArgs a) {
    __shared__ u64 keys[SAMPLE_NS];
    __shared__ float prob[SAMPLE_NS];
    __shared__ uint32_t seen[SAMPLE_NS / 32]; // [EXT] penalty: history bitmap over [0, n)
    __shared__ float sh_f[2];
    __shared__ int sh_cut;
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* lg = a.logits + (size_t)b * a.stride;
    const int mask = a.mask_idx ? a.mask_idx[b] : -1;
    const float T = a.temperature[b];
    const int n = a.n;
    if (a.penalty) {
        for (int i = tid; i < SAMPLE_NS / 32; i += SAMPLE_THREADS) seen[i] = 0u;
        __syncthreads();
        const int32_t* h = a.hist + (size_t)b * a.hist_stride;
        const int len = a.hist_len[b];
        for (int f = tid; f < len; f += SAMPLE_THREADS) {
            const int c = h[(size_t)f * 16];
            if (c >= 0 && c < n) atomicOr(&seen[c >> 5], 1u << (c & 31));
        }
        if (tid == 0 && a.cur_key) { // null: hist_len covers the whole history (the head of a resumed prefill)
            const int c = key_code(a.cur_key[(size_t)b * a.cur_stride]);
            if (c >= 0 && c < n) atomicOr(&seen[c >> 5], 1u << (c & 31));
        }
        __syncthreads();
    }
    const float pen = a.penalty ? a.penalty[b] : 1.0f;
    for (int i = tid; i < SAMPLE_NS; i += SAMPLE_THREADS) {
        u64 k = 0; // pads sort below every real candidate (a real key always has a non-zero low word or high word)
        if (i < n) {
            float v = lg[i];
            if (a.penalty && ((seen[i >> 5] >> (i & 31)) & 1u)) v = v < 0.0f ? v * pen : v / pen; // transformers' RepetitionPenaltyLogitsProcessor
            v = (i == mask) ? -INFINITY : v;
            k = pack_key(v, i);
        }
        keys[i] = k;
    }
    __syncthreads();
    if (T <= 0.0f) { // greedy branch: max key == largest value, smallest index among equals
        u64 m = 0;
        for (int i = tid; i < SAMPLE_NS; i += SAMPLE_THREADS) m = keys[i] > m ? keys[i] : m;
        for (int s = 32; s >= 1; s >>= 1) { const u64 o = __shfl_xor(m, s); m = o > m ? o : m; }
        __syncthreads();
        if ((tid & 63) == 0) keys[tid >> 6] = m;
        __syncthreads();
        if (tid == 0) {
            u64 best = 0;
            for (int w = 0; w < SAMPLE_THREADS / 64; w++) best = keys[w] > best ? keys[w] : best;
            a.out_key[(size_t)b * a.out_stride] = pack_key(0.0f, key_code(best));
        }
        return;
    }
    // ---- bitonic sort, descending ----
    for (int k = 2; k <= SAMPLE_NS; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < SAMPLE_NS / 2; t += SAMPLE_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)); // lower index of the pair
                const int p = i | j;
                const bool desc = (i & k) == 0;
                const u64 x = keys[i], y = keys[p];
                if ((x < y) == desc) { keys[i] = y; keys[p] = x; }
            }
            __syncthreads();
        }
    }
    const int top_k = a.top_k[b];
    int c = (top_k > 0 && top_k < n) ? top_k : n; // :711-713
    const float max_logit = key_value(keys[0]);
    for (int i = tid; i < c; i += SAMPLE_THREADS) { const float sc = (key_value(keys[i]) - max_logit) / T; prob[i] = q3_expf(sc); } // :716-722
    __syncthreads();
    if (tid == 0) { float sum = 0.0f; for (int i = 0; i < c; i++) sum = sum + prob[i]; sh_f[0] = sum; }
    __syncthreads();
    { const float sum = sh_f[0]; if (sum > 0.0f) for (int i = tid; i < c; i += SAMPLE_THREADS) prob[i] = prob[i] / sum; } // :724-730
    __syncthreads();
    const float top_p = a.top_p[b];
    if (top_p < 1.0f) { // :734-753
        if (tid == 0) {
            float cum = 0.0f; int cut = c;
            for (int i = 0; i < c; i++) { cum = cum + prob[i]; if (cum >= top_p) { cut = i + 1; break; } }
            float ns = 0.0f;
            for (int i = 0; i < cut; i++) ns = ns + prob[i];
            sh_cut = cut; sh_f[1] = ns;
        }
        __syncthreads();
        c = sh_cut;
        const float ns = sh_f[1];
        if (ns > 0.0f) for (int i = tid; i < c; i += SAMPLE_THREADS) prob[i] = prob[i] / ns;
        __syncthreads();
    }
    if (tid == 0) { // :761-775
        const uint32_t draw = a.draws[b];
        const float r = (float)chacha12_word(a.rng_key + (size_t)b * 8, draw) / 4294967296.0f;
        a.draws[b] = draw + 1;
        int pick = key_code(keys[0]);
        float cum = 0.0f;
        for (int i = 0; i < c; i++) { cum = cum + prob[i]; if (r < cum) { pick = key_code(keys[i]); break; } }
        a.out_key[(size_t)b * a.out_stride] = pack_key(0.0f, pick);
    }
}

void launch_sample(hipStream_t st, const SampleArgs& a, int B) {
    Q3_CHECK(a.n >= 1 && a.n <= SAMPLE_NS, "sampler range exceeds 4096 candidates");
    hipLaunchKernelGGL(k_sample, dim3(B), dim3(SAMPLE_THREADS), 0, st, a);
}

#define PRED_NS 2048
#define PRED_THREADS 256
#define PRED_PER (PRED_NS / PRED_THREADS)

__global__ void __launch_bounds__(PRED_THREADS) k_sample_pred(SampleArgs a) {
    __shared__ u64 cand[PRED_NS];
    __shared__ float prob[PRED_NS];
    __shared__ uint32_t bins[256];
    __shared__ u64 red[PRED_THREADS / 64];
    __shared__ float sh_f[2];
    __shared__ int sh_cut, sh_bin, sh_rem, sh_cnt;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* lg = a.logits + (size_t)b * a.stride;
    const float T = a.temperature[b];
    const int n = a.n;
    u64 k[PRED_PER]; // element tid + j*PRED_THREADS (coalesced loads); 0 = no element
#pragma unroll
    for (int j = 0; j < PRED_PER; j++) { const int i = tid + j * PRED_THREADS; k[j] = i < n ? pack_key(lg[i], i) : 0ull; }
    if (T <= 0.0f) { // greedy: the largest key == first max, as ArgmaxEpi picks it
        u64 m = 0;
#pragma unroll
        for (int j = 0; j < PRED_PER; j++) m = k[j] > m ? k[j] : m;
        for (int s = 32; s >= 1; s >>= 1) { const u64 o = __shfl_xor(m, s); m = o > m ? o : m; }
        if (lane == 0) red[wave] = m;
        __syncthreads();
        if (tid == 0) {
            u64 best = 0;
            for (int w = 0; w < PRED_THREADS / 64; w++) best = red[w] > best ? red[w] : best;
            a.out_key[(size_t)b * a.out_stride] = pack_key(0.0f, key_code(best));
        }
        return;
    }
    const int top_k = a.top_k[b];
    int c = (top_k > 0 && top_k < n) ? top_k : n; // :711-713
    // ---- radix select: the c largest keys are those whose masked top bits are >= prefix ----
    u64 prefix = 0, mask = 0;
    if (c < n) {
        int rem = c; // keys still missing among those matching prefix under mask
        for (int d = 7; d >= 0; d--) {
            const int sh = d * 8;
            bins[tid] = 0u; // PRED_THREADS == 256 bins
            __syncthreads();
#pragma unroll
            for (int j = 0; j < PRED_PER; j++)
                if (k[j] != 0ull && (k[j] & mask) == prefix) atomicAdd(&bins[(int)((k[j] >> sh) & 255ull)], 1u);
            __syncthreads();
            if (wave == 0) { // lane l owns bins 255-4l .. 252-4l (descending); inclusive scan of the lane sums across the wave
                uint32_t h4[4], s = 0;
#pragma unroll
                for (int q = 0; q < 4; q++) { h4[q] = bins[255 - 4 * lane - q]; s += h4[q]; }
                uint32_t inc = s;
                for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(inc, o); if (lane >= o) inc += v; }
                uint32_t above = inc - s; // keys in higher bins than this lane's
                if (above < (uint32_t)rem && inc >= (uint32_t)rem) {
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        if (above < (uint32_t)rem && above + h4[q] >= (uint32_t)rem) { sh_bin = 255 - 4 * lane - q; sh_rem = rem - (int)above; sh_cnt = (int)h4[q]; }
                        above += h4[q];
                    }
                }
            }
            __syncthreads();
            prefix |= (u64)sh_bin << sh; mask |= (u64)255 << sh;
            rem = sh_rem;
            const bool exact = sh_cnt == rem;
            __syncthreads(); // sh_* are rewritten by the next digit
            if (exact) break;
        }
    }
    // ---- compaction (wave ballots, one LDS atomic per wave and element row), padding to a power of two ----
    int P = 1;
    while (P < c) P <<= 1;
    if (tid == 0) sh_cnt = 0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PRED_PER; j++) {
        const bool sel = k[j] != 0ull && (k[j] & mask) >= prefix;
        const u64 bal = __ballot(sel);
        int base = 0;
        if (lane == 0 && bal) base = atomicAdd(&sh_cnt, __popcll(bal));
        base = __shfl(base, 0);
        if (sel) cand[base + __popcll(bal & ((1ull << lane) - 1ull))] = k[j];
    }
    for (int i = c + tid; i < P; i += PRED_THREADS) cand[i] = 0ull;
    __syncthreads();
    // ---- bitonic sort of the P candidates, descending ----
    for (int kk = 2; kk <= P; kk <<= 1) {
        for (int j = kk >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < P / 2; t += PRED_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int p = i | j;
                const bool desc = (i & kk) == 0;
                const u64 x = cand[i], y = cand[p];
                if ((x < y) == desc) { cand[i] = y; cand[p] = x; }
            }
            __syncthreads();
        }
    }
    // ---- from here on the same steps as k_sample ----
    const float max_logit = key_value(cand[0]);
    for (int i = tid; i < c; i += PRED_THREADS) { const float sc = (key_value(cand[i]) - max_logit) / T; prob[i] = q3_expf(sc); }
    __syncthreads();
    if (tid == 0) { float sum = 0.0f; for (int i = 0; i < c; i++) sum = sum + prob[i]; sh_f[0] = sum; }
    __syncthreads();
    { const float sum = sh_f[0]; if (sum > 0.0f) for (int i = tid; i < c; i += PRED_THREADS) prob[i] = prob[i] / sum; }
    __syncthreads();
    const float top_p = a.top_p[b];
    if (top_p < 1.0f) {
        if (tid == 0) {
            float cum = 0.0f; int cut = c;
            for (int i = 0; i < c; i++) { cum = cum + prob[i]; if (cum >= top_p) { cut = i + 1; break; } }
            float ns = 0.0f;
            for (int i = 0; i < cut; i++) ns = ns + prob[i];
            sh_cut = cut; sh_f[1] = ns;
        }
        __syncthreads();
        c = sh_cut;
        const float ns = sh_f[1];
        if (ns > 0.0f) for (int i = tid; i < c; i += PRED_THREADS) prob[i] = prob[i] / ns;
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t draw = a.draws[b];
        const float r = (float)chacha12_word(a.rng_key + (size_t)b * 8, draw) / 4294967296.0f;
        a.draws[b] = draw + 1;
        int pick = key_code(cand[0]);
        float cum = 0.0f;
        for (int i = 0; i < c; i++) { cum = cum + prob[i]; if (r < cum) { pick = key_code(cand[i]); break; } }
        a.out_key[(size_t)b * a.out_stride] = pack_key(0.0f, pick);
    }
}

void launch_sample_pred(hipStream_t st, const SampleArgs& a, int B) {
    Q3_CHECK(a.n >= 1 && a.n <= PRED_NS, "predictor sampler range exceeds 2048 candidates");
    Q3_CHECK(!a.penalty && !a.mask_idx, "the predictor sampler takes no penalty or mask");
    hipLaunchKernelGGL(k_sample_pred, dim3(B), dim3(PRED_THREADS), 0, st, a);
}

} // namespace q3
