// tsm.h -- [EXT] speaking rate (q3tts_spec.h "speaking rate"): what the stretcher needs beyond the counts and the submit rule in sched_logic.h
// and still without a device: the two normative window tables, built in double and rounded to f32, the visit order of the candidates, and
// what a stretch launch refuses.  No HIP, no threads: tests/host/tsm_logic_main.cpp builds it with plain g++ under the host sanitizers.
#pragma once
#include "sched_logic.h"
#include <cmath>
#include <cstdint>

namespace q3 {

// w[i] = f32(0.5 - 0.5 cos(2 pi i / 960)), w2[i] = f32(0.5 + 0.5 cos(2 pi i / 960)), i in [0, 480)
inline void tsm_windows(float* w, float* w2) {
    const double pi = 3.14159265358979323846;
    for (int i = 0; i < Q3_TSM_HOP; i++) {
        const double c = std::cos(2.0 * pi * (double)i / (double)Q3_TSM_WIN);
        w[i] = (float)(0.5 - 0.5 * c);
        w2[i] = (float)(0.5 + 0.5 * c);
    }
}

// the visit order of offset d in [-240, 240] and back: o(0) = 0, o(-j) = 2j - 1, o(+j) = 2j
constexpr int tsm_visit_order(int d) { return d == 0 ? 0 : (d < 0 ? -2 * d - 1 : 2 * d); }
constexpr int tsm_offset_of_order(int o) { return (o & 1) ? -((o + 1) >> 1) : (o >> 1); }

// what a stretch launch and a pitch launch refuse alike, in the order both state it: G streams of T native samples each (T = 0 is a flush
// alone), streams[] slots of an n_streams state store, encodings enc[].  no_nulls / null_text: whether the caller's arrays are all there,
// and what it says when not; why_not(g): what stream g's rate or pair is refused for, asked between its slot and its encoding
template <class WhyNot>
inline const char* prosody_launch_refusal(int G, int max_group, int64_t T, bool flush, const int32_t* streams, int n_streams, const int32_t* enc,
                                          bool no_nulls, const char* null_text, WhyNot why_not) {
    const char* const chunk_why = (T < 0 || T % Q3_TSM_HIST != 0 || (T == 0 && !flush)) ? "chunk length is no positive multiple of 1920 samples"
                                  : T > (int64_t)1 << 24 ? "chunk too long" : !no_nulls ? null_text : nullptr;
    return stage_launch_refusal(G, max_group, chunk_why, streams, n_streams, [&](int g) -> const char* {
        if (const char* why = why_not(g)) return why;
        return (enc[g] != Q3_PCM_F32 && enc[g] != Q3_PCM_S16) ? "unknown encoding" : nullptr;
    });
}

// what a stretch launch refuses (nullptr = it may run): stream g at pct[g] percent (100: the stream is not touched) in encoding enc[g]
inline const char* tsm_launch_refusal(int G, int max_group, int64_t T, bool flush, const int32_t* streams, int n_streams, const int32_t* pct,
                                      const int32_t* enc) {
    return prosody_launch_refusal(G, max_group, T, flush, streams, n_streams, enc, streams && pct && enc, "null streams / rates / encodings",
                                  [&](int g) { return tsm_rate_why_not(pct[g]); });
}

} // namespace q3
