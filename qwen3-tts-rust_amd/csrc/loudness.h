// loudness.h -- [EXT] loudness (q3tts_spec.h "loudness"): everything of the BS.1770 meter that needs no device: the K-weighting tables, one
// step of the filter (the one definition the kernel and the host share), the segmented evaluation order on the host, the gate, the gain
// helper, what a launch refuses and the submit rule.  No HIP, no threads: tests/host/loudness_logic_main.cpp builds it with plain g++ under
// the host sanitizers.  Every expression here is meant to be compiled without contraction (-ffp-contract=off): a fused multiply-add anywhere
// in loud_step changes the bits.
#pragma once
#include "../../include/q3tts_spec.h"
#include "sched_logic.h"
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define Q3_LOUD_HD __host__ __device__ __forceinline__
#else
#define Q3_LOUD_HD inline
#endif

namespace q3 {

constexpr int LOUD_SEGS_PER_BLOCK = Q3_LOUD_BLOCK / Q3_LOUD_SEG;   // 25
static_assert(Q3_LOUD_BLOCK % Q3_LOUD_SEG == 0 && Q3_PCM_FRAME % Q3_LOUD_SEG == 0, "frame, chunk and block edges fall on segment edges");
static_assert(Q3_LOUD_STATE == 6, "s1 s2 t1 t2, the running block's energy and peak");

// coef: shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 (1, -2, 1) a1 a2.  m: A^Q3_LOUD_SEG, row-major [4][4]
struct LoudTables { double coef[10]; double m[16]; };

// one stage of K-weighting at sample rate fs through the bilinear transform of BS.1770's analog prototype; out = b0 b1 b2 a1 a2
inline void loud_stage(double fs, bool shelf, double* out) {
    const double pi = 3.14159265358979323846;
    if (shelf) {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = std::tan(pi * f0 / fs), Vh = std::pow(10.0, G / 20.0), Vb = std::pow(Vh, 0.4996667741545416);
        const double a0 = 1.0 + K / Q + K * K;
        out[0] = (Vh + Vb * K / Q + K * K) / a0; out[1] = 2.0 * (K * K - Vh) / a0; out[2] = (Vh - Vb * K / Q + K * K) / a0;
        out[3] = 2.0 * (K * K - 1.0) / a0; out[4] = (1.0 - K / Q + K * K) / a0;
    } else {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = std::tan(pi * f0 / fs);
        const double a0 = 1.0 + K / Q + K * K;
        out[0] = 1.0; out[1] = -2.0; out[2] = 1.0;
        out[3] = 2.0 * (K * K - 1.0) / a0; out[4] = (1.0 - K / Q + K * K) / a0;
    }
}
inline void loud_coefs(double fs, double* coef /* [10] */) { loud_stage(fs, true, coef); loud_stage(fs, false, coef + 5); }

// One sample through both stages, transposed direct form II; s = (s1, s2, t1, t2).  Returns z, the K-weighted sample
Q3_LOUD_HD double loud_step(double* s, double v, const double* c) {
    const double y = c[0] * v + s[0];
    s[0] = (c[1] * v - c[3] * y) + s[1];
    s[1] = c[2] * v - c[4] * y;
    const double z = y + s[2];
    s[2] = (-2.0 * y - c[8] * z) + s[3];
    s[3] = y - c[9] * z;
    return z;
}
// start_{k+1} = M start_k + z_k, row by row in the normative order
Q3_LOUD_HD void loud_carry(const double* m, const double* s, const double* z, double* out) {
    out[0] = (((m[0] * s[0] + m[1] * s[1]) + m[2] * s[2]) + m[3] * s[3]) + z[0];
    out[1] = (((m[4] * s[0] + m[5] * s[1]) + m[6] * s[2]) + m[7] * s[3]) + z[1];
    out[2] = (((m[8] * s[0] + m[9] * s[1]) + m[10] * s[2]) + m[11] * s[3]) + z[2];
    out[3] = (((m[12] * s[0] + m[13] * s[1]) + m[14] * s[2]) + m[15] * s[3]) + z[3];
}

inline void loud_tables(LoudTables* t) {
    loud_coefs((double)Q3_PCM_NATIVE_RATE, t->coef);
    for (int i = 0; i < 4; i++) {   // column i: Q3_LOUD_SEG zero-input steps from the unit state e_i
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        s[i] = 1.0;
        for (int n = 0; n < Q3_LOUD_SEG; n++) (void)loud_step(s, 0.0, t->coef);
        for (int r = 0; r < 4; r++) t->m[r * 4 + i] = s[r];
    }
}

// blocks a chunk of T samples at stream position pos completes
inline int64_t loud_blocks(int64_t pos, int64_t T) { return (pos + T) / Q3_LOUD_BLOCK - pos / Q3_LOUD_BLOCK; }

// The segmented evaluation ("parallel form") of one chunk on the host, phase by phase as the kernel runs it: x[T] at stream position pos,
// state[Q3_LOUD_STATE] in and out, rows [loud_blocks(pos, T)][2] out.  T and pos are multiples of Q3_LOUD_SEG.  Returns the rows written
inline int64_t loud_chunk_host(const LoudTables& t, const float* x, int64_t T, int64_t pos, double* state, double* rows) {
    const int64_t nseg = T / Q3_LOUD_SEG;
    double start[4] = {state[0], state[1], state[2], state[3]};
    double e = state[4], p = state[5];
    int64_t n_rows = 0;
    for (int64_t k = 0; k < nseg; k++) {
        const float* xs = x + k * Q3_LOUD_SEG;
        double z[4] = {0.0, 0.0, 0.0, 0.0};                                                  // phase 1
        for (int n = 0; n < Q3_LOUD_SEG; n++) (void)loud_step(z, (double)xs[n], t.coef);
        double s[4] = {start[0], start[1], start[2], start[3]};                              // phase 3, from start_k
        double q = 0.0; float pk = 0.0f;
        for (int n = 0; n < Q3_LOUD_SEG; n++) {
            const double w = loud_step(s, (double)xs[n], t.coef);
            q = q + w * w;
            pk = std::fmax(pk, std::fabs(xs[n]));
        }
        double nx[4];
        loud_carry(t.m, start, z, nx);                                                       // phase 2
        for (int r = 0; r < 4; r++) start[r] = nx[r];
        e = e + q; p = std::fmax(p, (double)pk);
        if ((pos / Q3_LOUD_SEG + k + 1) % LOUD_SEGS_PER_BLOCK == 0) { rows[2 * n_rows] = e; rows[2 * n_rows + 1] = p; n_rows++; e = 0.0; p = 0.0; }
    }
    for (int r = 0; r < 4; r++) state[r] = start[r];
    state[4] = e; state[5] = p;
    return n_rows;
}

// ---- the gate (q3tts_loudness of include/q3tts.h, restated here so that this header stands alone) ----
struct LoudResult { double integrated_lufs, momentary_max_lufs, peak_dbfs; int32_t n_blocks, n_gated; };
inline double loud_lufs(double z) { return -0.691 + 10.0 * std::log10(z); }
// rows [n][2] = {energy, peak} of n 100 ms blocks
inline void loud_gate(const double* rows, int32_t n, LoudResult* out) {
    const double ninf = -HUGE_VAL;
    out->integrated_lufs = ninf; out->momentary_max_lufs = ninf; out->peak_dbfs = ninf; out->n_blocks = n > 0 ? n : 0; out->n_gated = 0;
    double pk = 0.0;
    for (int32_t j = 0; j < n; j++) pk = std::fmax(pk, rows[2 * j + 1]);
    if (pk > 0.0) out->peak_dbfs = 20.0 * std::log10(pk);
    const int32_t nb = n - 3;   // 400 ms blocks at 100 ms hop
    if (nb < 1) return;
    auto zj = [&](int32_t j) { return (((rows[2 * j] + rows[2 * (j + 1)]) + rows[2 * (j + 2)]) + rows[2 * (j + 3)]) / 9600.0; };
    double sum = 0.0, mx = ninf; int32_t cnt = 0;
    for (int32_t j = 0; j < nb; j++) {
        const double z = zj(j), l = loud_lufs(z);
        if (l > mx) mx = l;
        if (l > -70.0) { sum = sum + z; cnt++; }
    }
    out->momentary_max_lufs = mx;
    if (cnt == 0) return;
    const double rel = loud_lufs(sum / (double)cnt) - 10.0;
    double sum2 = 0.0; int32_t cnt2 = 0;
    for (int32_t j = 0; j < nb; j++) {
        const double z = zj(j), l = loud_lufs(z);
        if (l > -70.0 && l > rel) { sum2 = sum2 + z; cnt2++; }
    }
    out->n_gated = cnt2;
    if (cnt2 > 0) out->integrated_lufs = loud_lufs(sum2 / (double)cnt2);
}

// the volume, in tenths of a dB, that takes a request measured at measured_lufs to target_lufs: rounded to nearest, clamped to the volume
// range; 0 for a non-finite input
inline int32_t loud_gain_db10(double measured_lufs, double target_lufs) {
    if (!std::isfinite(measured_lufs) || !std::isfinite(target_lufs)) return 0;
    const double d = std::nearbyint((target_lufs - measured_lufs) * 10.0);
    return d < (double)Q3_VOL_MIN ? Q3_VOL_MIN : d > (double)Q3_VOL_MAX ? Q3_VOL_MAX : (int32_t)d;
}

// what a loudness launch refuses (nullptr = it may run): G streams of T native samples each, streams[] slots of an n_streams state store,
// stream g metered where metered[g] != 0, then at stream position pos[g]
inline const char* loudness_launch_refusal(int G, int max_group, int64_t T, const int32_t* streams, int n_streams, const int32_t* metered, const int64_t* pos) {
    const char* const chunk_why = (T <= 0 || T % Q3_PCM_FRAME != 0) ? "chunk length is no positive multiple of 1920 samples"
                                  : T > (int64_t)1 << 24 ? "chunk too long" : (!streams || !metered || !pos) ? "null streams / metered / positions" : nullptr;
    return stage_launch_refusal(G, max_group, chunk_why, streams, n_streams, [&](int g) -> const char* {
        return (metered[g] && (pos[g] < 0 || pos[g] % Q3_PCM_FRAME != 0)) ? "stream position is no multiple of 1920 samples" : nullptr;
    });
}
// the submit rule of a metered request.  nullptr = it may be queued
inline const char* loudness_submit_refusal(bool have_codec) { return have_codec ? nullptr : "the engine has no codec"; }

} // namespace q3
