// pitch.h -- [EXT] pitch (q3tts_spec.h "pitch"): what the pitch shifter needs beyond the pair rule, the plan and the counts in sched_logic.h
// and still without a device: the prototype filter of a pitch's L / M resampler (the converter's builder, pcm_out.h, at another ratio), the
// image of all 151 tables as the device holds it, and what a pitch launch refuses.  No HIP, no threads: tests/host/pitch_logic_main.cpp
// builds it with plain g++ under the host sanitizers.
#pragma once
#include "pcm_out.h"
#include "tsm.h"
#include <cstdint>
#include <vector>

namespace q3 {

constexpr int PITCH_N = Q3_PITCH_MAX - Q3_PITCH_MIN + 1;   // 151 pitches, 100 among them (its table is never read: 100 is off)

// h32 of pitch P: N_taps floats; empty for a pitch out of range
inline std::vector<float> pitch_filter(int P) {
    PitchPlan p;
    if (!pitch_plan(P, &p)) return std::vector<float>();
    return pcm_filter_lm(p.L, p.M);
}

// every pitch's h32 one after the other, each starting on a 16-byte boundary; off[P - Q3_PITCH_MIN] = its first float
struct PitchTables { std::vector<float> all; int off[PITCH_N]; int64_t taps = 0; };
inline PitchTables pitch_tables() {
    PitchTables t;
    for (int P = Q3_PITCH_MIN; P <= Q3_PITCH_MAX; P++) {
        const std::vector<float> h = pitch_filter(P);
        t.off[P - Q3_PITCH_MIN] = (int)t.all.size();
        t.all.insert(t.all.end(), h.begin(), h.end());
        t.taps += (int64_t)h.size();
        t.all.resize((t.all.size() + 3) / 4 * 4, 0.0f);
    }
    return t;
}

// what a pitch launch refuses (nullptr = it may run): prosody_launch_refusal (tsm.h) with stream g at rate[g] percent and pitch[g] percent
// (pitch 100: the stream is not touched, whatever its rate)
inline const char* pitch_launch_refusal(int G, int max_group, int64_t T, bool flush, const int32_t* streams, int n_streams, const int32_t* rate,
                                        const int32_t* pitch, const int32_t* enc) {
    return prosody_launch_refusal(G, max_group, T, flush, streams, n_streams, enc, streams && rate && pitch && enc,
                                  "null streams / rates / pitches / encodings", [&](int g) { return prosody_pair_why_not(rate[g], pitch[g]); });
}

} // namespace q3
