// volume.h -- [EXT] volume (q3tts_spec.h "volume"): what the volume stage needs beyond the range, the gain and the submit rule in sched_logic.h
// and still without a device: the tile walk of a chunk and what a volume launch refuses.  No HIP, no threads:
// tests/host/volume_logic_main.cpp builds it with plain g++ under the host sanitizers.
#pragma once
#include "sched_logic.h"
#include <cstdint>

namespace q3 {

constexpr int VOL_TILE = Q3_PCM_FRAME;                    // samples a tile writes: a chunk is a whole number of them
constexpr int VOL_SPAN = VOL_TILE + Q3_VOL_HIST;          // values of v a tile holds in LDS: its own and the Q3_VOL_HIST below them

// what a volume launch refuses (nullptr = it may run): G streams of T native samples each, streams[] slots of an n_streams state store,
// stream g at db10[g] tenths of a dB (0: the stream is not touched)
inline const char* volume_launch_refusal(int G, int max_group, int64_t T, const int32_t* streams, int n_streams, const int32_t* db10) {
    if (G < 1 || G > max_group) return "group size out of range";
    if (T <= 0 || T % VOL_TILE != 0) return "chunk length is no positive multiple of 1920 samples";
    if (T > (int64_t)1 << 24) return "chunk too long";
    if (!streams || !db10) return "null streams / volumes";
    for (int g = 0; g < G; g++) {
        if (streams[g] < 0 || streams[g] >= n_streams) return "stream out of range";
        for (int h = 0; h < g; h++) if (streams[h] == streams[g]) return "a stream may appear once per launch";
        if (const char* why = volume_why_not(db10[g])) return why;
    }
    return nullptr;
}

} // namespace q3
