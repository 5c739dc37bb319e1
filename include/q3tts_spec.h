/*
 * q3tts_spec.h -- NORMATIVE arithmetic specification ("Q3TTS arithmetic spec v1")
 *
 * The reference (IuvenisSapiens/Qwen3-TTS-Rust) delegates all transformer arithmetic to llama.cpp
 * b8123, which is not in the reference tree.  Token parity "oracle <-> HIP" therefore
 * needs ONE written-down arithmetic; this header is it.  Every float reduction has a fixed order,
 * every transcendental is a fixed polynomial in IEEE fma/mul/add, so the C oracle (gcc, x86-64) and
 * the HIP kernels (gfx950) produce BIT-IDENTICAL logits and hence bit-identical codec tokens.
 *
 * The arithmetic mirrors ggml's CPU path in structure (activations quantised to int8 blocks of 32
 * with an f16 scale, exact integer block dot products, f32 accumulation of block terms), differing
 * only in the (explicitly fixed) order of the f32 accumulation.
 *
 * Compiles as C11, C++17 and HIP device code.  Both sides MUST be built with -ffp-contract=off and
 * without fast-math; fused multiply-adds appear only where q3_fmaf is written.
 *
 * Protocol constants are source-pinned by the reference: prompt.rs:5-16, engine.rs:505-518,555-558,587-596.
 */
#ifndef Q3TTS_SPEC_H
#define Q3TTS_SPEC_H

#include <stdint.h>
#include <string.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define Q3_HD __host__ __device__ static inline
#else
#define Q3_HD static inline
#endif

/* ---------------- protocol constants (reference file:line in comments) ---------------- */
#define Q3_CODEC_PAD        2148   /* prompt.rs:5  */
#define Q3_CODEC_BOS        2149   /* prompt.rs:6  */
#define Q3_CODEC_EOS        2150   /* prompt.rs:7, engine.rs:558 */
#define Q3_TEXT_BOS         151672 /* prompt.rs:8  */
#define Q3_TEXT_EOS         151673 /* prompt.rs:9  */
#define Q3_CODEC_THINK      2154   /* prompt.rs:10 */
#define Q3_CODEC_NOTHINK    2155   /* prompt.rs:11 */
#define Q3_CODEC_THINK_BOS  2156   /* prompt.rs:12 */
#define Q3_CODEC_THINK_EOS  2157   /* prompt.rs:13 */
#define Q3_TEXT_AUDIO_MARKER 151671 /* prompt.rs:16, assets_manager.rs:244 */
#define Q3_CODEC_AUDIO_START 2160  /* prompt.rs:68 */
#define Q3_LANG_CHINESE     2055   /* engine.rs:267,407,425 */
#define Q3_SAMPLE_END       2160   /* engine.rs:555: talker sampling range [0,2160) */
#define Q3_N_CODEBOOKS      16     /* engine.rs:587 */
#define Q3_CODEBOOK_SIZE    2048   /* engine.rs:588-589,518 */
#define Q3_CHUNK_CODES      64     /* engine.rs:510 */
#define Q3_EMBD             2048   /* assets_manager.rs:244-247,423-425 (hard-coded row width) */
#define Q3_SAMPLE_RATE      24000  /* engine.rs:653 */
#define Q3_TALKER_NCTX      4096   /* engine.rs:133 */
#define Q3_PRED_NCTX        512    /* engine.rs:136 */
#define Q3_DEFAULT_MAX_STEPS 512   /* engine.rs:152 */

/* ---------------- arithmetic-spec structural constants ---------------- */
#define Q3_QBLK      32    /* activation / weight quantisation block (elements)            */
#define Q3_SEG_BLKS  8     /* blocks per segment: one f32 fma chain (256 elements)           */
#define Q3_SEG       256
#define Q3_SSEG_SEGS 8     /* segments per super-segment (2048 elements)                     */
#define Q3_SSEG      2048
#define Q3_HEAD_DIM  128   /* talker & predictor head dim (spec lane maps assume 128)        */
#define Q3_ATT_CHUNK 256   /* attention positions per softmax chunk                          */

/* ---------------- f16 / bf16 <-> f32, IEEE round-to-nearest-even ---------------- */
Q3_HD uint32_t q3_f32_bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
Q3_HD float q3_bits_f32(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

Q3_HD float q3_f16_to_f32(uint16_t h) {
    uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1Fu;
    uint32_t man = h & 0x3FFu;
    uint32_t out;
    if (exp == 0) {
        if (man == 0) {
            out = sign;
        } else { /* subnormal: normalise */
            int e = -1;
            do { man <<= 1; e++; } while ((man & 0x400u) == 0);
            man &= 0x3FFu;
            out = sign | ((uint32_t)(127 - 15 - e) << 23) | (man << 13);
        }
    } else if (exp == 31) {
        out = sign | 0x7F800000u | (man << 13);
    } else {
        out = sign | ((exp + 112u) << 23) | (man << 13);
    }
    return q3_bits_f32(out);
}

Q3_HD uint16_t q3_f32_to_f16(float f) {
    uint32_t x = q3_f32_bits(f);
    uint32_t sign = (x >> 16) & 0x8000u;
    uint32_t ax = x & 0x7FFFFFFFu;
    if (ax >= 0x7F800000u) { /* inf / nan */
        return (uint16_t)(sign | 0x7C00u | ((ax > 0x7F800000u) ? 0x200u : 0u));
    }
    if (ax >= 0x477FF000u) { /* >= 65520 -> inf after rounding */
        return (uint16_t)(sign | 0x7C00u);
    }
    if (ax < 0x33000001u) { /* < 2^-25 (or == 2^-25, ties to even -> 0) */
        return (uint16_t)sign;
    }
    int32_t e = (int32_t)(ax >> 23) - 127;
    uint32_t man = (ax & 0x7FFFFFu) | 0x800000u; /* 24-bit significand */
    uint32_t shift;
    uint32_t hexp;
    if (e < -14) { /* subnormal half */
        shift = (uint32_t)(13 + (-14 - e));
        hexp = 0;
    } else {
        shift = 13;
        hexp = (uint32_t)(e + 15);
    }
    uint32_t half_man = man >> shift;
    uint32_t rem = man & ((1u << shift) - 1u);
    uint32_t halfway = 1u << (shift - 1);
    if (rem > halfway || (rem == halfway && (half_man & 1u))) half_man++;
    /* for normal numbers half_man carries the implicit bit at 0x400: adding (hexp-1)<<10 folds it in,
       and a mantissa overflow correctly bumps the exponent */
    uint32_t out;
    if (hexp == 0) out = half_man;
    else out = ((hexp - 1u) << 10) + half_man;
    return (uint16_t)(sign | out);
}

Q3_HD float q3_bf16_to_f32(uint16_t h) { return q3_bits_f32((uint32_t)h << 16); }
Q3_HD uint16_t q3_f32_to_bf16(float f) {
    uint32_t x = q3_f32_bits(f);
    if ((x & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((x >> 16) | 0x40u);
    return (uint16_t)((x + 0x7FFFu + ((x >> 16) & 1u)) >> 16);
}

/* ---------------- explicit fused multiply-add ---------------- */
#if defined(__HIP_DEVICE_COMPILE__)
#define q3_fmaf(a, b, c) __builtin_fmaf((a), (b), (c))
#define q3_rintf(x) __builtin_rintf(x)
#define q3_sqrtf(x) __builtin_sqrtf(x)
#define q3_fabsf(x) __builtin_fabsf(x)
#else
#define q3_fmaf(a, b, c) fmaf((a), (b), (c))
#define q3_rintf(x) rintf(x)
#define q3_sqrtf(x) sqrtf(x)
#define q3_fabsf(x) fabsf(x)
#endif

/* ---------------- expf: Cephes-style, only fma/mul/add/rint + exponent bit add ----------------
 * |rel err| ~ 1e-7.  Returns 0 for x < -87, +inf for x > 88.72. */
Q3_HD float q3_expf(float x) {
    if (x < -87.0f) return 0.0f;
    if (x > 88.72f) return q3_bits_f32(0x7F800000u);
    float n = q3_rintf(x * 1.44269504088896341f);
    float r = q3_fmaf(n, -0.693359375f, x);
    r = q3_fmaf(n, 2.12194440e-4f, r);
    float p = 1.9875691500E-4f;
    p = q3_fmaf(p, r, 1.3981999507E-3f);
    p = q3_fmaf(p, r, 8.3334519073E-3f);
    p = q3_fmaf(p, r, 4.1665795894E-2f);
    p = q3_fmaf(p, r, 1.6666665459E-1f);
    p = q3_fmaf(p, r, 5.0000001201E-1f);
    float r2 = r * r;
    float y = q3_fmaf(p, r2, r);
    y = y + 1.0f;
    int32_t ni = (int32_t)n;
    if (ni > 127) { /* x in (88.02, 88.72]: split the scale to stay finite */
        y = y * 2.0f;
        ni -= 1;
    }
    uint32_t yb = q3_f32_bits(y) + ((uint32_t)ni << 23);
    return q3_bits_f32(yb);
}

/* silu(g)*u, SwiGLU (spec S8) */
Q3_HD float q3_swiglu(float g, float u) {
    float e = q3_expf(-g);
    float den = 1.0f + e;
    float sg = g / den;
    return sg * u;
}

/* ---------------- activation quantisation, one block of 32 (spec S2; ggml quantize_row_q8_0 shape)
 * amax exact; d = amax/127; id = 1/d; q = rint(x*id); stored scale = f16(d). */
Q3_HD uint16_t q3_quant_block32(const float* x, int8_t* q) {
    float amax = 0.0f;
    for (int i = 0; i < 32; i++) {
        float a = q3_fabsf(x[i]);
        if (a > amax) amax = a;
    }
    float d = amax / 127.0f;
    float id = (d != 0.0f) ? (1.0f / d) : 0.0f;
    for (int i = 0; i < 32; i++) q[i] = (int8_t)(int)q3_rintf(x[i] * id);
    return q3_f32_to_f16(d);
}

/* RoPE rotation of one NeoX pair (x1 = x[i], x2 = x[i+64]) (spec S5) */
Q3_HD void q3_rope_pair(float x1, float x2, float c, float s, float* o1, float* o2) {
    float t = x2 * s;
    *o1 = q3_fmaf(x1, c, -t);
    float u = x1 * s;
    *o2 = q3_fmaf(x2, c, u);
}

/* which M-RoPE position stream (0..3) rotates pair index i; sections sum may be 0 => stream 0.
 * llama.cpp-style sector assignment [EXT]. */
Q3_HD int q3_mrope_stream(int i, const int32_t sec[4]) {
    int tot = sec[0] + sec[1] + sec[2] + sec[3];
    if (tot <= 0) return 0;
    int s = i % tot;
    if (s < sec[0]) return 0;
    if (s < sec[0] + sec[1]) return 1;
    if (s < sec[0] + sec[1] + sec[2]) return 2;
    return 3;
}

/* ---------------- "ggml-CPU" arithmetic mode (opt-in, Q3_SPEC=ggml) ----------------
 * expf as glibc's generic (non-FMA) float routine computes it [EXT: sysdeps/ieee754/flt-32/e_expf.c + exp2f_data, N = 32]: a 32-entry table of
 * 2^(i/32) and a degree-3 polynomial, all in double, one rounding to float at the end.  Restated so that the oracle's ggml mode and the HIP
 * ggml-mode kernels share ONE definition (libm's expf differs between hosts: FMA builds contract differently); on the build container's glibc the
 * two agree on every one of 200 000 random arguments (table recomputed with exact integer arithmetic, tests/test_ggml_mode_cpu.py keeps checking). */
Q3_HD float q3_expf_ggml(float x) {
    static const uint64_t T[32] = {
        0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull, 0x3fef72b83c7d517bull, 0x3fef54873168b9aaull,
        0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull, 0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
        0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull, 0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull,
        0x3feea11473eb0187ull, 0x3feea589994cce13ull, 0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
        0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull, 0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full,
        0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};
    if (x != x) return x;
    if (x > 88.72283172607421875f) return q3_bits_f32(0x7F800000u);
    if (x < -103.97208404541015625f) return 0.0f;
    const double InvLn2N = 0x1.71547652b82fep+0 * 32.0, Shift = 0x1.8p+52;
    const double C0 = 0x1.c6af84b912394p-5 / 32.0 / 32.0 / 32.0, C1 = 0x1.ebfce50fac4f3p-3 / 32.0 / 32.0, C2 = 0x1.62e42ff0c52d6p-1 / 32.0;
    const double z = InvLn2N * (double)x;
    double kd = z + Shift;
    uint64_t ki; memcpy(&ki, &kd, 8);
    kd = kd - Shift;
    const double r = z - kd;
    uint64_t t = T[ki % 32] + (ki << (52 - 5));
    double s; memcpy(&s, &t, 8);
    const double zz = C0 * r + C1;
    const double r2 = r * r;
    double y = C2 * r + 1.0;
    y = zz * r2 + y;
    y = y * s;
    return (float)y;
}
/* ggml-quants.c nearest_int: magic-number rounding (half to even), |v| <= 4194303 */
Q3_HD int q3_nearest_int_ggml(float fval) {
    float val = fval + 12582912.f;
    int32_t i; memcpy(&i, &val, 4);
    return (i & 0x007fffff) - 0x00400000;
}

/* ---------------- generation controls beyond the reference [EXT] (q3tts_gen_options; defaults reproduce the reference) ----------------
 * Repetition penalty p (> 0, 1.0 = off) -- transformers' RepetitionPenaltyLogitsProcessor, upstream's talker default 1.05:
 *   applied to the talker's code_0 logits before the sampler step (EOS mask, sort, top-k, ...).  History = the set of DISTINCT code_0 values
 *   the sequence has emitted so far: for the logits of frame f+1, frames 0..f (the prompt is not part of it; the first code_0, drawn at
 *   prefill, sees an empty history).  Each history token is changed once: l < 0 ? l * p : l / p, f32, correctly rounded division.
 *   The penalty also applies when T <= 0 (greedy on the penalised logits).
 * Sampled code predictor (predictor_temperature > 0; <= 0 = greedy, the reference's LlamaSampler::greedy at engine.rs:470):
 *   each of the 15 passes draws with LlamaSampler::sample (llama/mod.rs:703-775) over that pass's 2048 logits with predictor_top_k /
 *   predictor_top_p, from a second per-sequence ChaCha12 stream seed_from_u64(seed ^ Q3_PRED_SEED_XOR), seed = the request's resolved seed.
 *   Draw order: passes 1..15 of frame 0, then of frame 1, ...  The talker's own stream is untouched. */
#define Q3_PRED_SEED_XOR 0x9E3779B97F4A7C15ull

/* ---------------- streaming-text ("dual-track") talker input [EXT] (q3tts_prompt_build_streaming, q3tts_submit_trailing) ----------------
 * Upstream's second talker layout, transformers 5.15 models/qwen3_omni_moe/modeling_qwen3_omni_moe.py:
 *   Qwen3OmniMoeForConditionalGeneration._get_talker_assistant_parts (prompt ends [tts_bos + codec_pad], [text_0 + codec_bos];
 *   trailing_text_hidden = [text_1 .. text_{n-1}, tts_eos]) and Qwen3OmniMoeTalkerForConditionalGeneration.prepare_inputs_for_generation
 *   (step input = sum of the codec rows + trailing_text_hidden[generation_step], or + tts_pad once the trailing rows are used up;
 *   prefill sets generation_step = -1 and every step adds 1).
 * In this engine's terms, for text ids t_0 .. t_{n-1} (n >= 1):
 *   prompt   = the reference prompt (build_core / build_clone_prompt) up to and including [text(Q3_TEXT_BOS) + E_0(Q3_CODEC_PAD)],
 *              then one row [text(t_0) + E_0(Q3_CODEC_BOS)]: n + 1 rows shorter than the reference prompt of the same text
 *   trailing = t_1 .. t_{n-1}, Q3_TEXT_EOS (n_trail = n ids)
 *   feedback of frame f (0-based; frame 0's code_0 comes from the prefill) =
 *              (sum_q E_q[code_q], q = 0..15 in order) + (f < n_trail ? text(trail[f]) : tts_pad), f32 left to right
 *   text(id) = HostAssets::text_embedding(id) exactly, the out-of-range fallback row fmod((float)((u64)id * 17 + i), 2) - 1 included
 *   (the synthetic models have 4096 text rows: Q3_TEXT_EOS takes the fallback there).  tts_pad = the reference's marker row 151671.
 * With n_trail = 0 the feedback is the reference's; a raw prompt with trailing ids may be submitted with any n_trail in [0, max_prompt]. */

/* ---------------- live text append [EXT] (q3tts_submit_trailing_open, q3tts_trail_append, q3tts_text_append) ----------------
 * A streaming-text request may be submitted with an OPEN trail.  Let n_avail = the number of trailing ids appended so far.
 *   while the trail is open:  frame f runs only when f < n_avail; otherwise the slot WAITS: that frame has no effect on anything the slot
 *                             owns (codes, history, positions, finished flag, the talker hidden row, the talker and predictor RNG draw
 *                             counters; the talker KV row at the frame's position is rewritten by the frame that runs there later)
 *   once it is closed:        frames behave as in the streaming-text definition above: trail[f] while f < n_trail, then tts_pad
 * Device predicate, slot b, read at the start and at the end of every gated frame (nothing inside a frame changes its inputs):
 *   waits = !finished[b] && n_frames[b] < max_frames[b] && open[b] && n_frames[b] >= n_trail[b]
 * Consequence: an open request that ends with the id list T, appended in any pieces, at any moments, with any number of waited frames,
 * gives the codes and PCM of the same request submitted closed with T (q3tts_submit_trailing).  Waiting never consumes an RNG draw, writes
 * history or advances a position, and the other slots of the batch step as they would without it.
 * Text level: q3tts_submit_text_streaming_open(t[:k]) opens the trail t_1 .. t_{k-1} (the prompt depends on t_0 only);
 * q3tts_text_append(t[k:], is_last = 1) appends t_k .. t_{n-1}, Q3_TEXT_EOS and closes: together the trail of q3tts_submit_text_streaming(t).
 * The total number of trailing ids stays within max_prompt. */

/* ---------------- resume [EXT] (q3tts_submit_resume, q3tts_group_submit_resume) ----------------
 * Let R be a request: prompt, sampler config with a given seed, q3tts_gen_options, and a trailing-id list that is closed or open.
 * Let c[0..k) be the first k frames R emits, 1 <= k < max_steps, none of them EOS.
 * resume(R, c[0..k)) is a request whose frame f equals R's frame f for every f: frames 0..k-1 are taken from the caller, frames k.. are
 * generated.  Nothing of R but its prompt, options, seed and emitted codes is needed:
 *   prefill    the talker prefill runs over n_prompt + k rows.  Row n_prompt + f is the feedback row of frame f exactly as defined above,
 *              (sum_q E_q[c[f][q]], q = 0..15 in order) + (f < n_trail ? text(trail[f]) : tts_pad), f32 left to right; a negative code
 *              reads row 0 and a code past its table the zero row, as the frame's own feedback does.  It sits at position n_prompt + f in
 *              the three running position streams (the fourth stays 0), as the decode step of that frame placed it.  The arithmetic is
 *              independent of launch geometry, batch size and chunking, so the K/V rows are the rows the decode steps wrote
 *   head       runs on the last row: the hidden row the predictor starts from, and the logits of frame k's code_0
 *   penalty    the history is the distinct code_0 values of frames 0..k-1, so the penalty applies to that first head, greedy requests
 *              included (a plain prefill's first head sees an empty history)
 *   RNG        frame k's code_0 consumes talker draw k; the predictor stream stands at draw 15 k; greedy streams stay at 0
 *   counters   the frame counter, the trailing cursor, the positions and the history length all start at k
 *   codec      the stream is reset, then fed frames 0..k-1 in the chunks the scheduler would have cut (4 frames each), then the new frames:
 *              codes and PCM are those of the whole utterance; n_frames starts at k and the prefix is fetchable at once
 *   k = 0      is q3tts_submit_trailing / q3tts_submit_trailing_open itself
 * An open trail must hold at least k ids when it is resumed: frames 0..k-1 ran, so their ids were known.
 * Consequence: for any split point k the codes of resume(R, c[0..k)) are bit-identical to R's, the PCM within 1e-4 RMS with the same
 * sample count.  With another seed (has_seed = 0 draws a fresh one) the prefix is kept and the rest is a fresh draw. */

/* ---------------- token log-probabilities [EXT] (q3tts_engine_set_logprobs, q3tts_fetch_logprobs, q3tts_op_logprob_rows) ----------------
 * A recording request carries Q3_LOGPROB_COLS = 17 floats per frame f:
 *   column 0      log softmax(L_T)[code_0]: L_T = the talker head's raw f32 logits over the sampling range [0, Q3_SAMPLE_END), of the head
 *                 that produced frame f's code_0 (the prefill head for the first generated frame, frame f-1's head otherwise)
 *   column q      q = 1..15: log softmax(L_q)[code_q] over the 2048 predictor logits of step q
 *   column 16     log softmax(L_T)[Q3_CODEC_EOS], same talker row as column 0: how close the model was to stopping at this frame
 * Raw = before the repetition penalty, before temperature / top-k / top-p and without the mask_eos knob: the model's own distribution,
 * whatever the sampler then did with it (column 16 is finite for a request that masks EOS).
 * Arithmetic, f32:  m = max_i x_i (over finite and -inf entries);  s = sum_i q3_expf(x_i - m), per-lane strided partial sums, then a tree;
 *   lp = (x_c - m) - logf(s).  An -inf logit at the chosen index gives -inf; results are <= 0, a positive rounding residue is clamped to 0.
 * NOT a bit-exact spec item (the summation order is the kernel's, logf is the device library's): pinned to the float64 log-softmax of the same
 * f32 logits within |lp - lp64| <= 1e-5 * max(1, |lp64|)  (a strided-plus-tree f32 sum of <= 4096 positive terms: < ~1e-6 relative; q3_expf
 * and logf a few ulp each; two subtractions, one rounding each: together < ~2e-6 * max(1, |lp|), the tolerance is 5 x that).
 * Q3_LOGPROB_NONE marks a value that was not computed -- rows 0 .. n_prefix-1 of a resumed request, requests that retire before a row is
 * complete.  A real value is never positive.
 * Recording changes nothing else: codes and PCM of a recording request are those of the same request without it. */
#define Q3_LOGPROB_COLS 17
#define Q3_LOGPROB_NONE 1.0f

/* ---------------- scoring given frames [EXT] (q3tts_submit_score, q3tts_group_submit_score, q3tts_op_score_rows / _inputs) ----------------
 * Given a prompt of n_prompt rows, optional closed trailing ids and codes c[0..n)[16], row f of the result is the row q3tts_fetch_logprobs
 * shows for frame f of a request that emitted exactly these codes.  Nothing is sampled; the pass is teacher-forced on the given codes:
 *   talker     columns 0 and 16 come from the raw talker logits [0, Q3_SAMPLE_END) of prefill row n_prompt - 1 + f: the last prompt row for
 *              f = 0, the feedback row of frame f - 1 for f >= 1, built and placed as "resume" builds the rows of a prefix (with
 *              text(trail[f - 1]) as its last addend while f - 1 < n_trail).  Column 0 is the log-softmax at c[f][0], column 16 at
 *              Q3_CODEC_EOS.  The feedback row of frame n - 1 would only serve a frame n; it is not needed
 *   predictor  columns 1..15 come from a 16-token sequence of the code predictor: position 0 is project(hidden of that talker row), position 1
 *              is project(E_0[c[f][0]]), position q + 1 is project(E_q[c[f][q]]) for q = 1..14 (a negative code reads row 0 and a code past
 *              its table the zero row); the logits for c[f][q + 1] are head slice q at position q + 1, q = 0..14
 *   raw        as for recording: no penalty, no temperature / top-k / top-p, no EOS mask
 * Arithmetic and tolerance are those of "token log-probabilities": q3_expf, |lp - lp64| <= 1e-5 * max(1, |lp64|) against the float64
 * log-softmax of the same f32 logits.  The logits are those of the generating request bit for bit (the arithmetic is independent of launch
 * geometry, batch size and chunking), so a scored row and the row recorded while the same engine generated the same codes differ by at most
 * 2e-5 * max(1, |lp|): both lie within the tolerance of one float64 value.
 * Refused: n < 1 or n > max_steps; a code_0 outside [0, Q3_SAMPLE_END) or equal to Q3_CODEC_EOS (no request emits a frame with it); a residual
 * code outside [0, 2048); n_prompt + n beyond the KV capacity of a slot; the ggml-arithmetic mode. */

/* ---------------- candidate sets [EXT] (q3tts_submit_candidates, q3tts_group_submit_candidates, q3tts_op_kv_fork) ----------------
 * n sampled takes of one prompt behind one prefill.  Candidate i of a set over (prompt, options, closed trail, seeds[0..n)) is, bit for bit in
 * its codes, PCM and log-probability rows, the request q3tts_submit_trailing queues for the same prompt, options and trail with seed seeds[i]:
 *   streams    talker draws from StdRng(seeds[i]), predictor draws (sampled predictor) from StdRng(seeds[i] ^ Q3_PRED_SEED_XOR), both from draw 0
 *   prefill    the talker's K/V of prompt position p depends on rows [0, p] of the prompt alone and the arithmetic is independent of launch
 *              geometry, batch size and chunking, so the K/V one member's prefill wrote is the K/V every member's own prefill would write.
 *              It is copied in whole pages: logical pages [0, ceil(n_prompt / 64)) of the prefilled member's sequence go, K plane and V
 *              plane, into the same logical pages of every other member.  Positions n_prompt .. of the last copied page carry whatever the
 *              source page held; no member reads a position before its own decode step has written it
 *   frame 0    every member's code_0 is drawn by its own sampler state from the raw logits of prompt row n_prompt - 1, and its predictor starts
 *              from that row's hidden state: one head pass per member in an in-line wave, one staged row copied per member in an asynchronous one
 *   afterwards a member is an ordinary request: nothing in the frame graph knows about sets
 * A set is admitted whole (one slot per member, one codec stream per member with PCM) and its rows count once against the 4096 rows of an
 * asynchronous wave.  A member cancelled in the queue leaves the set; the first member left is the one prefilled.
 * Refused: n < 1 or n > max_batch; a resumed prefix or an open trail (not expressible); the ggml-arithmetic mode. */

/* ---------------- decoding given frames [EXT] (q3tts_submit_decode, q3tts_group_submit_decode) ----------------
 * Let c[0..n) be frames [16] as q3tts_fetch returns them.
 *   D1  PCM        decode(c) delivers the PCM of a request that emitted exactly c and ended after frame n - 1: the same sample count, within the
 *                  standing PCM tolerance of 1e-4 RMS.  By construction: the codec stream is reset (AudioDecoder::create_state), and the frames
 *                  go through a Chunker as a generating request's do -- every code clamped to [0, 2047], chunks of Q3_CHUNK_CODES codes
 *                  (4 frames), then the is_final flush of the n % 4 frames left
 *   D2  others     the codes of every other request are bit-identical to those without the decode-only request (it touches nothing of the
 *                  talker or predictor); their PCM has the same count and stays within the same tolerance (a chunk's result does not depend
 *                  on which other streams share its pass beyond that)
 *   D3  resources  no talker slot, no KV pages, no prefill wave, no frame graph: on an otherwise idle engine q3tts_stats.graph_frames, frames,
 *                  sched_steps and prefill_ms stay where they were.  One codec stream and its PCM staging region, from admission to the fence
 * Admission: decode-only requests wait in a FIFO of their own.  In a scheduler step the generating wave takes its codec streams first; then
 * decode-only requests are admitted in order while a stream is free and fewer than decode_width = max(1, (n_cs - max_batch) / 2) of them
 * hold one (n_cs: the engine's codec streams; the surplus n_cs - max_batch serves requests whose slot is reused while they drain).
 * Seats: the decoder thread keeps the tasks of decode-only requests in a second queue.  A pass is led by the oldest pending chunk of a
 * generating request, seats the first pending chunks of the other generating requests with the lead's frame count, then those of decode-only
 * requests, one chunk per request, at most gmax; with no generating chunk the oldest decode-only chunk leads.  After 4 consecutive passes
 * that seated no decode-only chunk while one waited, the oldest decode-only chunk leads the next pass.  A decode-only request's reset and
 * fence run alone as soon as they head its tasks.  With no decode-only request the passes are those formed without this feature.
 * Hand-over: a request's tasks (reset, chunks, fence) reach the decoder thread in the scheduler step that admitted it -- at once when that step
 * runs no frame group, else together with the chunks the step's frame group produced, so that the two kinds meet in the queues.
 * Every frame group's chunks (with the tails and fences of the slots it retires) are one hand-over: the thread forms no pass while they
 * arrive, and the generating chunks of one pass come from one hand-over.  Which generating streams share a pass is therefore a function of
 * the schedule -- which step hands over which chunks --, not of the two threads' timing: two runs with the same schedule give the same PCM
 * bit for bit, and a request keeps its bits when only another request's codes change (a pass's row count picks the GEMM forms, so the bits
 * do depend on who shares the pass; D2's tolerance covers that).
 * States: Q3TTS_REQ_QUEUED until a stream is taken, Q3TTS_REQ_DRAINING until the fence, Q3TTS_REQ_DONE; n_frames = n from submission on.
 * Refused: n < 1 or n > max_steps; no codec; a code_0 outside [0, Q3_SAMPLE_END) or equal to Q3_CODEC_EOS; a residual code outside [0, 2048)
 * (no request emits such a frame). */

/* ---------------- output formats [EXT] (q3tts_pcm_out_plan / _filter / _samples, q3tts_op_pcm_convert) ----------------
 * The codec delivers f32 samples at 24000 Hz.  A converter strictly behind it turns a stream's samples into one of these formats:
 *   rates      8000, 12000, 16000, 22050, 24000 (native), 32000, 44100, 48000.  g = gcd(rate, 24000), L = rate / g, M = 24000 / g
 *              (22050 is 147/160, 44100 is 147/80)
 *   encodings  f32 for rates <= 24000 only, s16 for every rate: no format needs more bytes per native sample than the native one
 *              (48000 s16 needs exactly as many).  {24000, f32} is "native" and means no conversion at all
 *   filter     F = max(L, M), Z = 16, N = 2 Z F + 1 taps, fc = 0.9 / (2F);
 *              h[i] = L * 2fc * sinc(2fc * (i - Z F)) * kaiser_{beta = 9}(i), i = 0 .. N-1, in double, then rounded to f32 (h32).
 *              sinc(x) = sin(pi x) / (pi x); kaiser(i) = I0(beta * sqrt(1 - ((i - Z F) / (Z F))^2)) / I0(beta)
 *   sample     output sample n of a stream, counted from the stream's reset: t = n M, p = t mod L, j = t div L,
 *              y[n] = sum over k = 0, 1, ... with p + k L < N of h32[p + k L] * x[j - k], where x[< 0] = 0 (samples before the reset).
 *              One f32 accumulator starting at 0, k ascending, one fmaf per term; the result is clamped to [-1, 1] as the codec's output is.
 *              s16 is (int16) rintf(y * 32767.0f), ties to even, from that same clamped f32 value (the product rounded to f32 first), so
 *              the two encodings never disagree
 *   24000      no filter and no delay; s16 at 24000 is the clamp and the rounding alone
 *   counts     T native samples give exactly T L / M output samples.  A frame is 1920 samples and 1920 L / M is an integer for all eight
 *              rates, so no phase is carried between chunks and the converted stream does not depend on how the frames were cut into chunks
 *   delay      the converted stream is the native one delayed by Z F / L native samples: 48 at 8000 Hz (2 ms), 32 at 12000, 24 at 16000,
 *              16 at 32000, 44100 and 48000, 17.4 at 22050.  Nothing is held back and nothing is flushed: THE LAST Z F / L NATIVE SAMPLES
 *              OF AN UTTERANCE DO NOT COME OUT
 * One output sample sums 33 to 97 terms and reaches at most 96 native samples back: the converter keeps the last 96 samples per stream. */
typedef struct q3tts_pcm_format { int32_t sample_rate; int32_t encoding; } q3tts_pcm_format;   /* encoding: 0 = f32, 1 = s16 */
#define Q3_PCM_F32 0
#define Q3_PCM_S16 1
#define Q3_PCM_NATIVE_RATE 24000
#define Q3_PCM_FRAME 1920        /* native samples per frame */
#define Q3_PCM_FILTER_Z 16
#define Q3_PCM_FILTER_BETA 9.0
#define Q3_PCM_HIST 96           /* native samples of history per stream */

/* ---------------- codec preambles [EXT] (q3tts_preamble_*, q3tts_decoder_snapshot_*) ----------------
 * Every request's codec stream starts from a reset.  A preamble is a stream state to start from instead: the state behind frames p[0..m),
 * [16] codes each -- typically a clone voice's reference codes -- built once, kept on the device and restored per request.
 * Let c[0..n) be the frames a request emits or is given.
 *   P1 PCM     the request's native PCM is decode(p ++ c) with the first m * 1920 samples dropped.  decode is one stream from a reset; every
 *              code is clamped to [0, 2047]; p is cut into 4-frame chunks plus an m % 4 tail, then c as a Chunker cuts it (4-frame chunks,
 *              then the final flush).  The sample count is that of the unprimed request; tolerance 1e-4 RMS (D1, resume).  RoPE positions
 *              continue: frame f of the request sits at position m + f, so m + max_steps stays within Q3TTS_CODEC_MAX_FRAMES
 *   P2 codes   codes, log-probability rows and every other request's codes are bit-identical to the run without a preamble: nothing of
 *              the talker or the predictor knows about it
 *   P3 formats a converting request delivers the conversion of preamble_pcm ++ request_pcm with the first m * 1920 * L / M output samples
 *              dropped: at the restore the stream's converter history holds the preamble's last Q3_PCM_HIST native samples instead of
 *              zeros.  Counts and tolerances of "output formats" are unchanged
 *   P4 restore a restore writes the stream's history slots of every state tensor and its two counters (cached positions, frames seen) from
 *              the snapshot, and nothing else; a state blob exported after a restore equals the blob exported at the snapshot, bit for bit
 *   resume     the restore comes first, then the prefix frames, then the new ones
 *   decode     the PCM of a decode-only request is P1 with c = the given frames
 *   sets       every member of a candidate set restores the same snapshot into its own stream
 *   cancel     unchanged: the prefix kept is the primed run's prefix
 *   never      want_pcm = 0 and q3tts_generate_batch* are never primed
 * A setter takes a READY preamble only, so whether a request is primed never depends on timing and admission waits for nothing new.
 * At most Q3TTS_MAX_PREAMBLES preambles are live per engine; an id is never reused. */
#define Q3TTS_MAX_PREAMBLES 64
#define Q3TTS_PREAMBLE_BUILDING 0
#define Q3TTS_PREAMBLE_READY 1
#define Q3TTS_PREAMBLE_FAILED -1

/* ---------------- speaking rate [EXT] (q3tts_engine_set_speech_rate, q3tts_tsm_samples / _windows, q3tts_op_tsm) ----------------
 * A pitch-preserving time-scale change (WSOLA) of the native 24000 Hz stream, strictly behind the codec.  x[n] is the native stream, y[m] the
 * delivered one; every position is a sample index counted from the stream's reset.
 *   rate       pct, an integer percent in [Q3_TSM_MIN, Q3_TSM_MAX]; input consumed per second of output is pct / 100.  100 means off: the
 *              request is an ordinary one and nothing of this section runs
 *   analysis   synthesis frame k >= 0 covers y[480 k .. 480 k + 480).  Its analysis position is a_k = floor(k * 480 * pct / 100) in 64-bit
 *              integers
 *   windows    for i in [0, 480): w[i] = f32(0.5 - 0.5 cos(2 pi i / 960)), w2[i] = f32(0.5 + 0.5 cos(2 pi i / 960)), evaluated in double and
 *              then rounded to f32.  The two tables are normative, as the converter's h32 is
 *   template   p_{-1} = -480.  The natural continuation of frame k is t_k = p_{k-1} + 480
 *   candidates c = a_k + d for d in [-240, 240] with c >= 0
 *   cost       SSD_k(d) = sum over i = 0 .. 479 of (x[c + i] - x[t_k + i])^2, evaluated with one f32 accumulator starting at +0, i ascending,
 *              diff = x[c + i] - x[t_k + i] as one f32 subtraction, acc = fmaf(diff, diff, acc)
 *   selection  visit order o(0) = 0, o(-j) = 2 j - 1, o(+j) = 2 j.  The chosen d_k minimises (SSD, o) lexicographically; a non-negative f32's
 *              bit pattern orders as the value does, so the minimum of (bits << 32 | o) decides it.  p_k = a_k + d_k
 *   output     y[480 k + i] = fmaf(w[i], x[p_k + i], w2[i] * x[t_k + i]) with the product rounded to f32 first, clamped to [-1, 1].
 *              s16 is the converter's rule, (int16) rintf(y * 32767.0f) of the clamped value.  Every output sample depends on the input
 *              alone: no output state is carried
 *   available  frame k is computed once N, the native samples seen, satisfies a_k + 1200 <= N.  That suffices for every pct in range:
 *              p_k + 960 <= a_k + 1200 and t_k + 480 <= a_k + 1200.  While streaming, N samples have produced exactly
 *              480 * #{k : a_k + 1200 <= N} output samples, and the result does not depend on how the input was cut into chunks
 *   flush      at the end of an utterance x[n >= N] = 0 and every frame with a_k < N is produced: 480 * ceil(100 N / (480 pct)) samples in
 *              all.  A cancelled request is not flushed
 *   history    the next frame reaches back to a_k - 720 at most and forward to N, which is below a_k + 1200: the last Q3_TSM_HIST native
 *              samples per stream, d of the last frame and the two counters (N, frames made) are the whole state
 * What follows from it: at pct = 100, d_k = 0 for all k and |y - x| <= 2^-23 |x| (the engine never runs it: 100 is off).  For an exactly
 * periodic input x[n] = tab[n mod P] every chosen candidate has SSD exactly 0 and y[m] = tab[m mod P] within the same bound: the waveform
 * continues in phase at any rate.  All-zero input gives d = 0 everywhere.
 * A stretching request delivers 24000 Hz, f32 or s16; rates combined with resampled formats are not defined. */
#define Q3_TSM_HOP 480           /* synthesis hop: 20 ms */
#define Q3_TSM_WIN 960
#define Q3_TSM_SEARCH 240        /* +-10 ms */
#define Q3_TSM_LOOK 1200         /* native samples a frame needs past its analysis position */
#define Q3_TSM_HIST 1920         /* native samples of history per stream */
#define Q3_TSM_MIN 50
#define Q3_TSM_MAX 200

/* ---------------- pitch [EXT] (q3tts_engine_set_pitch, q3tts_pitch_samples / _plan / _filter, q3tts_op_pitch) ----------------
 * A pitch shift of the native 24000 Hz stream, strictly behind the codec: a time-scale change to the tempo rate / pitch ("speaking rate"
 * with a rational tempo) followed by a resample that consumes pitch / 100 intermediate samples per delivered sample ("output formats" with a
 * ratio that is no sample rate), inside one launch.  x[n] is the native stream, z[m] the intermediate one, y[n] the delivered one; every
 * position is a sample index counted from the stream's reset.  The duration is that of the rate alone, the fundamental is multiplied.
 *   pitch      P = pitch_pct, an integer percent in [Q3_PITCH_MIN, Q3_PITCH_MAX]; the delivered fundamental is P / 100 times the native one.
 *              100 means off: nothing of this section runs, and a request with rate_pct != 100 and pitch 100 is the stretched request of
 *              "speaking rate", bit for bit
 *   pair       with R = rate_pct the tempo R / P must lie in [1/2, 2]: 2 R >= P and R <= 2 P.  Checked at submit, where both settings are
 *              read together; a submit with a pair out of range fails and queues nothing
 *   stage 1    z is y of "speaking rate" word for word with a_k = floor(k * 480 * R / P) in 64-bit integers: windows, template, candidates,
 *              cost chain, selection order and the output rule with its clamp are unchanged, so z with P = 100 is that section's y
 *   reach      a_k - a_{k-1} lies in [floor(480 R / P), ceil(480 R / P)], inside [240, 960] by the pair rule.  t_k = a_{k-1} + d_{k-1} + 480,
 *              so t_k - a_k = 480 + d_{k-1} - (a_k - a_{k-1}) lies in [480 - 240 - 960, 480 + 240 - 240] = [-720, 480]: the template reads
 *              x[a_k - 720 .. a_k + 960).  A candidate reads x[a_k - 240 .. a_k + 720) and p_k + 960 <= a_k + 1200.  Frame k therefore reads
 *              inside [a_k - 720, a_k + 1200), Q3_TSM_HIST samples, whatever the pair
 *   available  frame k is computed once N, the native samples seen, satisfies a_k + 1200 <= N, which suffices by the reach.  While streaming, N
 *              samples have made #{k : a_k + 1200 <= N} frames: 0 for N < 1200, else (P (N - 1199) - 1) div (480 R) + 1.  Once flushed
 *              (x[n >= N] = 0, every frame with a_k < N): ceil(P N / (480 R)) frames
 *   history    the next frame k to make has a_k + 1200 > N and reaches back to a_k - 720 > N - 1920 at most: the last Q3_TSM_HIST native
 *              samples per stream, d of the last frame and the two counters (N, frames made) are stage 1's whole state, as in "speaking rate"
 *   stage 2    g = gcd(100, P), L = 100 / g, M = P / g, F = max(L, M), Z = Q3_PCM_FILTER_Z, N_taps = 2 Z F + 1, fc = 0.9 / (2F), and h32 the
 *              prototype of "output formats" for this (L, M): h[i] = L * 2fc * sinc(2fc (i - Z F)) * kaiser_9(i), in double, rounded to f32.
 *              Output sample n: t = n M, p = t mod L, j = t div L, y[n] = sum over k = 0, 1, ... with p + k L < N_taps of
 *              h32[p + k L] * z[j - k], z[< 0] = 0; one f32 accumulator from +0, k ascending, one fmaf per term; clamped to [-1, 1].
 *              s16 is (int16) rintf(y * 32767.0f) of the clamped value
 *   counts     Nz intermediate samples give exactly ceil(Nz L / M) delivered samples: y[n] needs z[j] and nothing later.  The phase is a pure
 *              function of n, so the delivered stream does not depend on how the native stream was cut into chunks
 *   delay      Z F / L intermediate samples, at most 32; as with the formats nothing is flushed for it
 *   state      stage 1's state, the last Q3_PITCH_HIST samples of z (one output reaches back 2 Z F / L <= 64) and the two data-independent
 *              counters (Nz, outputs made), which live on the host as the stretcher's do
 *   flush      at the end of an utterance stage 1 is flushed as in "speaking rate" and stage 2 delivers ceil(Nz_final L / M) in all.  A
 *              cancelled request is not flushed
 * A request with a pitch delivers 24000 Hz, f32 or s16; a pitch combined with a resampled format is not defined. */
#define Q3_PITCH_MIN 50
#define Q3_PITCH_MAX 200
#define Q3_PITCH_HIST 64         /* intermediate samples of history per stream */

/* ---------------- volume [EXT] (q3tts_engine_set_volume, q3tts_volume_gain, q3tts_op_volume) ----------------
 * A gain with a look-ahead peak limiter on the native 24000 Hz stream, behind the output conv and in front of every other output stage
 * ("output formats", "speaking rate", "pitch"): it rewrites the native samples those stages read, so it composes with all of them and a
 * boost never clips.  x[n] is the stream's native f32 samples since its reset (the output conv's clamped values), y[n] what replaces them;
 * every position is a sample index counted from the stream's reset.
 *   volume     db10, an integer in tenths of a dB in [Q3_VOL_MIN, Q3_VOL_MAX].  0 means off: nothing of this section runs.
 *              G = (float) pow(10.0, db10 / 200.0), computed on the host in double and rounded once (q3tts_volume_gain; NaN out of range)
 *   input      v[n] = G * x[n], one f32 multiply; v[n < 0] = 0
 *   required   r[j] = 1 for j < 0 or |v[j]| <= 1, else r[j] = 1.0f / |v[j]|, the correctly rounded f32 quotient
 *   hold       m[k] = min r[k - (Q3_VOL_HOLD - 1) .. k]; exact, whatever the order
 *   smoothing  s_0 = m, s_{i+1}[k] = s_i[k - 2^i] + s_i[k] for i = 0 .. 6 in f32: s_7[k] is the sum of m[k - 127 .. k] in that fixed tree
 *              (Q3_VOL_LOOK = 128 terms); g[n] = 0x1p-7f * s_7[n]
 *   output     y[n] = clamp(g[n] * v[n - Q3_VOL_DELAY], -1, 1), one f32 multiply.  In exact arithmetic |g[n] v[n - 127]| <= 1, since every
 *              hold window [k - 511, k] with k in [n - 127, n] contains n - 127: the clamp only removes rounding residue.  Where every |v| of
 *              the window is <= 1, g = 1 exactly (128 ones sum exactly) and y[n] = v[n - 127] bit for bit: any attenuation, and a boost of a
 *              quiet signal
 *   delay      Q3_VOL_DELAY = 127 native samples (5.3 ms).  Nothing is flushed, as with the converter's delay: the last 127 native samples of
 *              an utterance do not come out.  n native samples in give n samples out per chunk, so every count, offset and staging rule of
 *              the later stages is unchanged (q3tts_pcm_out_samples, q3tts_tsm_samples, q3tts_pitch_samples)
 *   state      per stream the last Q3_VOL_HIST = Q3_VOL_HOLD - 1 + Q3_VOL_DELAY values of v; zeroed by the stream's reset and by a preamble
 *              restore (a primed request starts from a reset).  No data-dependent counters: y depends on n and the stream alone, never on
 *              how the stream was cut into chunks
 *   error      given the same f32 v, y lies within 10 u |y64| + 2^-149 of the float64 evaluation and g within 8 u |g64|, u = 2^-24: one
 *              rounding in r, none in the minimum, seven in the tree of non-negative adds, one in the product */
#define Q3_VOL_MIN -400
#define Q3_VOL_MAX 200
#define Q3_VOL_LOOK 128          /* terms of the smoothing sum */
#define Q3_VOL_HOLD 512          /* samples of the hold minimum */
#define Q3_VOL_DELAY 127         /* native samples the stream is delayed by */
#define Q3_VOL_HIST 638          /* = Q3_VOL_HOLD - 1 + Q3_VOL_DELAY: values of v kept per stream */

/* ---------------- loudness [EXT] (q3tts_engine_set_loudness, q3tts_fetch_loudness, q3tts_loudness_*, q3tts_op_loudness) ----------------
 * An ITU-R BS.1770-4 meter on the native 24000 Hz stream: K-weighting and 100 ms block energies on the device, the gate on the host.  It
 * reads the output conv's chunk in front of "volume" and of every other output stage and writes no sample: what it measures is what the
 * model made, never the caller's gain, format, rate or pitch.  x[n] is the stream's native f32 samples since its reset; every position is
 * a sample index counted from the stream's reset (a preamble-primed request starts from a reset).  All of it is float64 without fused
 * multiply-adds.
 *   weighting  mono, channel weight 1, two biquads at fs = 24000.  The coefficients come from BS.1770's analog prototypes through the
 *              bilinear transform, on the host in double (q3tts_loudness_tables).  With K = tan(pi f0 / fs), a0 = 1 + K/Q + K^2:
 *                shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G/20),
 *                           Vb = Vh^0.4996667741545416; b = [(Vh + Vb K/Q + K^2)/a0, 2(K^2 - Vh)/a0, (Vh - Vb K/Q + K^2)/a0],
 *                           a1 = 2(K^2 - 1)/a0, a2 = (1 - K/Q + K^2)/a0
 *                high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1], a1' and a2' as above with this K and Q
 *              At fs = 48000 the formulas give the table printed in BS.1770
 *   filter     transposed direct form II, v = (double) x[n], state (s1, s2, t1, t2) zero at the reset:
 *                y = b0 v + s1;  s1 = (b1 v - a1 y) + s2;  s2 = b2 v - a2 y
 *                z = y + t1;     t1 = (-2 y - a1' z) + t2; t2 = y - a2' z
 *              Double is needed: the high-pass poles sit at radius 0.99 next to z = 1
 *   segments   the evaluation order is the definition.  The stream is cut into segments of Q3_LOUD_SEG = 96 samples (96 divides a frame
 *              of 1920 and a block of 2400).  M = A^96 is the 4x4 double matrix whose column i is the state after 96 zero-input steps from
 *              the unit state e_i.  Per chunk: (1) every segment k runs from the zero state to its end state z_k; (2) one ascending walk,
 *              start_0 = the stream's stored state, start_{k+1}[r] = (((M[r][0] s[0] + M[r][1] s[1]) + M[r][2] s[2]) + M[r][3] s[3]) + z_k[r]
 *              with s = start_k; (3) every segment runs again from start_k and gives q_k = the sum of z^2, a double sum ascending from +0,
 *              and p_k = max |x|
 *   blocks     block j covers samples [2400 j, 2400 j + 2400): e[j] = (..((q_25j + q_25j+1) + ..) + q_25j+24), peak[j] = max p.  A block a
 *              chunk leaves incomplete keeps its running sum and peak in the stream's state, so the sum is the same however the stream was
 *              cut.  A chunk of T samples at position pos completes floor((pos + T) / 2400) - floor(pos / 2400) blocks, each one row
 *              {energy, peak} of two doubles; n frames give floor(0.8 n) rows, and the unfinished last block does not come out
 *   state      per stream Q3_LOUD_STATE = 6 doubles: s1, s2, t1, t2, the running energy, the running peak; zeroed by the stream's reset and
 *              by a preamble restore.  No device counters: the host passes pos.  A row depends on the stream alone, never on the chunking
 *   gate       on the host (q3tts_loudness_gate), rows e[0 .. n): 400 ms blocks at 100 ms hop, z_j = (((e_j + e_j+1) + e_j+2) + e_j+3) / 9600,
 *              l_j = -0.691 + 10 log10 z_j.  Absolute gate l_j > -70; relative gate l_j > -0.691 + 10 log10(mean z of the absolutely gated
 *              blocks) - 10.  integrated = -0.691 + 10 log10(mean z of the blocks past both gates); momentary maximum = max l_j;
 *              peak = 20 log10 max peak[j] (the sample peak).  Where no block qualifies the value is -INFINITY and n_gated says so
 *   not here   true peak (4x oversampled), short-term 3 s loudness, loudness range, an automatic gain */
#define Q3_LOUD_SEG 96           /* samples per segment */
#define Q3_LOUD_BLOCK 2400       /* samples per 100 ms block */
#define Q3_LOUD_STATE 6          /* doubles of state per stream */

/* ---------------- prompt stems [EXT] (q3tts_stem_*, q3tts_op_kv_stem) ----------------
 * A stem is n rows [n][2048] f32, 1 <= n < max_prompt, together with the talker K/V of those rows at positions 0 .. n-1: the head a voice's
 * prompts share, prefilled once, kept on the device in a store of its own (ceil(n / 64) whole pages per plane, the pool's page layout) and
 * copied into a request's pages where the request's prefill would have written the same bits.
 *   applies    a text form takes its voice's stem (q3tts_voice_set_stem), a raw-prompt form (q3tts_submit, _ex, _trailing, _trailing_open,
 *              _resume, _candidates) the engine-level one (q3tts_engine_set_stem); read once per request at submit, once per candidate set
 *   takes      a request takes stem S when S applies to it, S is READY, n_prompt > n, and the first n * 2048 floats of its prompt are
 *              bytewise equal (memcmp) to S's rows.  The comparison runs once, at submit
 *   S1 result  a request that takes S produces exactly the codes, log-probability rows and PCM of the same request without a stem: its
 *              prefill starts at row n, rows [n, n_prompt) and the feedback rows of a resumed prefix land at the positions they always
 *              did, and positions [0, n) of its pages hold the store's bytes, which are the bytes its own prefill would have written
 *              (the talker's arithmetic is batch-invariant and chunk-invariant).  The stale positions of the store's last page, n .. , are
 *              written by the request's own rows before anything reads them
 *   S2 else    anything else runs the plain path and is counted as a mismatch, never an error: a wrong or stale stem costs time and
 *              cannot change a result
 *   sets       the first member of a candidate set restores, the others are forked from it
 *   never      score requests, decode-only requests, q3tts_generate_batch*, Q3_SPEC=ggml engines (q3tts_stem_create is refused there)
 * A setter takes a READY stem only.  At most Q3TTS_MAX_STEMS stems are live per engine; an id is never reused.  The states are the
 * preamble's, and so is the holder rule: the creator, the voices and the engine-level setting it is set on, and the requests that took it. */
#define Q3TTS_MAX_STEMS 64
#define Q3TTS_STEM_BUILDING 0
#define Q3TTS_STEM_READY 1
#define Q3TTS_STEM_FAILED -1

/* ---------------- reference audio intake [EXT] (q3tts_intake*, q3tts_wav_probe, q3tts_wav_intake) ----------------
 * The encoders read mono f32 at 24000 Hz.  The intake makes that of a clip in the caller's form: n frames of C interleaved channels at R Hz
 * in one of five sample formats.  It stands in front of the encoders as "output formats" stands behind the codec, with the same prototype.
 *   decode     u8 (v - 128) / 128; s16 v / 32768; s24 (3 bytes, little endian, sign-extended) v / 8388608; s32 (float)v / 2147483648;
 *              f32 as it is.  All in f32; s16, s32 and f32 are the reference's own arithmetic (engine.rs:348-359)
 *   downmix    Q3_INTAKE_FIRST: channel 0 (the reference).  Q3_INTAKE_MEAN: ((x0 + x1) + ... + x[C-1]) / (float)C, f32 adds in channel
 *              order and one f32 division (upstream's mono)
 *   ratio      L / M = 24000 / R in lowest terms, F = max(L, M), c = Z F, h32 = the prototype of "output formats" for this (L, M):
 *              N = 2 Z F + 1 taps, h[i] = L * 2fc * sinc(2fc (i - c)) * kaiser_9(i), fc = 0.9 / (2F), in double, rounded to f32
 *   sample     the clip is zero outside [0, n).  y[m] = sum over i of h32[c + m M - i L] * x[i], m in [0, n_out), n_out = ceil(n L / M):
 *              zero phase, nothing delayed and nothing dropped.  With t = m M + c, p = t mod L, j = t div L:
 *              y[m] = sum over k = 0, 1, ... with p + k L < N of h32[p + k L] * x[j - k].  One f32 accumulator starting at +0, k ascending,
 *              one fmaf per term (the converter's order).  No clamp: the encoders take what the reference would hand them
 *   24000      no filter: y is the decoded, downmixed clip bit for bit
 *   accepted   R in [8000, 192000] with max(L, M) <= Q3_INTAKE_MAX_F (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000,
 *              88200, 96000, 176400, 192000 among them); C in [1, 8]; n >= 1; n_out <= Q3_INTAKE_MAX_OUT (120 s), which keeps m M + c and
 *              i L below 2^31; at most Q3_INTAKE_MAX_CLIPS clips per call
 *   non-finite a downmixed sample that is not finite (an f32 clip's NaN or infinity, or a mean that overflows) fails the call, which names
 *              the clip; no output of that call is delivered
 * One output sample sums at most ceil(N / L) terms: 33 when upsampling, up to 257 at 192000 Hz. */
#define Q3_INTAKE_U8 0
#define Q3_INTAKE_S16 1
#define Q3_INTAKE_S24 2
#define Q3_INTAKE_S32 3
#define Q3_INTAKE_F32 4
#define Q3_INTAKE_FIRST 0
#define Q3_INTAKE_MEAN 1
#define Q3_INTAKE_MIN_RATE 8000
#define Q3_INTAKE_MAX_RATE 192000
#define Q3_INTAKE_MAX_F 320
#define Q3_INTAKE_MAX_CH 8
#define Q3_INTAKE_MAX_OUT 2880000
#define Q3_INTAKE_MAX_CLIPS 64
typedef struct { const void* data; int64_t n_frames; int32_t sample_rate, channels, sample_format, downmix; } q3tts_intake_clip;
typedef struct { int32_t sample_format, channels, sample_rate, bits; int64_t data_offset, n_frames; } q3tts_wav_info;

/* ggml tensor types used by this engine (public GGUF spec [EXT]) */
enum q3_ggml_type {
    Q3_T_F32 = 0, Q3_T_F16 = 1, Q3_T_Q8_0 = 8, Q3_T_Q5_K = 13, Q3_T_Q6_K = 14, Q3_T_BF16 = 30
};

#endif /* Q3TTS_SPEC_H */
