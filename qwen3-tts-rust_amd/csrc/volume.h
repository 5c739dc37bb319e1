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
    const char* const chunk_why = (T <= 0 || T % VOL_TILE != 0) ? "chunk length is no positive multiple of 1920 samples"
                                  : T > (int64_t)1 << 24 ? "chunk too long" : (!streams || !db10) ? "null streams / volumes" : nullptr;
    return stage_launch_refusal(G, max_group, chunk_why, streams, n_streams, [&](int g) { return volume_why_not(db10[g]); });
}

} // namespace q3
