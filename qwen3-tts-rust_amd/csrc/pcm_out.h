// pcm_out.h -- [EXT] output formats (q3tts_spec.h "output formats"): what the converter needs beyond the rules in sched_logic.h (the eight
// rates, their ratios, which formats exist, how many samples and bytes come out) and still without a device: the normative prototype filter
// built in double and rounded to f32, its phase-major image as the kernel reads it, and what a convert launch refuses.  No HIP, no threads:
// tests/host/pcm_out_logic_main.cpp builds it with plain g++ under the host sanitizers.
#pragma once
#include "sched_logic.h"
#include <cmath>
#include <cstdint>
#include <vector>

namespace q3 {

constexpr int PCM_TAPS_ALIGN = 4;
// one phase's row in the kernel's table: its taps, rounded up to whole 16-byte vectors
inline int pcm_phase_stride(const PcmPlan& p) { return (p.taps_per_phase + PCM_TAPS_ALIGN - 1) / PCM_TAPS_ALIGN * PCM_TAPS_ALIGN; }

inline double pcm_bessel_i0(double x) { // power series; every term is positive, so it stops when a term no longer changes the sum
    const double q = x * x / 4.0;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; k++) {
        term *= q / ((double)k * (double)k);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}

// h[i] = L * 2fc * sinc(2fc * (i - Z*F)) * kaiser_9(i), i = 0 .. N-1, fc = 0.9 / (2F), in double, then rounded to f32
// the prototype of any ratio L / M in lowest terms (the eight rates here, a pitch's 100 / P in pitch.h): N = 2 Z max(L, M) + 1 taps
inline std::vector<float> pcm_filter_lm(int L, int M) {
    const int F = L > M ? L : M, c = Q3_PCM_FILTER_Z * F, n_taps = 2 * c + 1;
    const double pi = 3.14159265358979323846, fc2 = 0.9 / (double)F, i0b = pcm_bessel_i0(Q3_PCM_FILTER_BETA);
    std::vector<float> h((size_t)n_taps);
    for (int i = 0; i < n_taps; i++) {
        const double x = fc2 * (double)(i - c), r = (double)(i - c) / (double)c;
        const double sinc = (i == c) ? 1.0 : std::sin(pi * x) / (pi * x);
        const double w = pcm_bessel_i0(Q3_PCM_FILTER_BETA * std::sqrt(1.0 - r * r)) / i0b;
        h[(size_t)i] = (float)((double)L * fc2 * sinc * w);
    }
    return h;
}
inline std::vector<float> pcm_filter(int rate) {
    PcmPlan p;
    if (!pcm_plan(rate, &p) || p.n_taps == 0) return std::vector<float>();
    return pcm_filter_lm(p.L, p.M);
}
// [L][stride]: row p holds h[p], h[p + L], h[p + 2L], ... and zeros behind the last tap below N
inline std::vector<float> pcm_filter_phase_major(const PcmPlan& p, const std::vector<float>& h) {
    const int stride = pcm_phase_stride(p);
    std::vector<float> t((size_t)p.L * stride, 0.0f);
    for (int ph = 0; ph < p.L; ph++)
        for (int k = 0; ph + k * p.L < p.n_taps; k++) t[(size_t)ph * stride + k] = h[(size_t)(ph + k * p.L)];
    return t;
}

// what a convert launch refuses (nullptr = it may run): G streams of T native samples each, streams[] slots of an n_streams history store
inline const char* pcm_convert_refusal(int G, int max_group, int64_t T, const int32_t* streams, int n_streams, const q3tts_pcm_format* fmt) {
    const char* const chunk_why = (T < Q3_PCM_FRAME || T % Q3_PCM_FRAME != 0) ? "chunk length is no whole number of frames"
                                  : T > (int64_t)0x7fffffff / 147 ? "chunk too long"   // n * M and T * L stay below 2^31 for every rate
                                  : (!streams || !fmt) ? "null streams / formats" : nullptr;
    return stage_launch_refusal(G, max_group, chunk_why, streams, n_streams, [&](int g) { return pcm_format_why_not(fmt[g].sample_rate, fmt[g].encoding); });
}

} // namespace q3
