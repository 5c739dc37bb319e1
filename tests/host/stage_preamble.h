// What the stage drivers' "preamble" command runs: the checks that every output stage's launch refusal shares (stage_launch_refusal,
// csrc/sched_logic.h) -- group size, stream out of range, stream listed twice -- against each other and against the stage's own two (the
// chunk length, one stream's own argument), any number failing at once.  The order is restated here as every refusal function spelled it
// out before they shared it: the group, the chunk, then stream by stream its slot, that it appears once, its own argument.
// refuse(G, max_group, chunk_ok, streams, n_streams, own_bad) calls the stage's refusal with stream own_bad's own argument bad (-1: none).
// Prints "preamble <cases>" or the first disagreement; returns whether all agreed.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>

template <class Refuse> bool check_stage_preamble(Refuse refuse, const char* chunk_text, const char* own_text) {
    const int gmax = 3, n_streams = 4;
    const int32_t vals[] = {-1, 0, 1, 2, 4};
    long n = 0;
    for (int G = 0; G <= gmax + 1; G++) for (int chunk_ok = 0; chunk_ok < 2; chunk_ok++) for (int own_bad = -1; own_bad < gmax; own_bad++)
        for (int32_t a : vals) for (int32_t b : vals) for (int32_t c : vals) {
            const int32_t s[4] = {a, b, c, 3};
            const char* want = nullptr;
            if (G < 1 || G > gmax) want = "group size out of range";
            else if (!chunk_ok) want = chunk_text;
            else for (int g = 0; g < G && !want; g++) {
                if (s[g] < 0 || s[g] >= n_streams) want = "stream out of range";
                for (int h = 0; h < g && !want; h++) if (s[h] == s[g]) want = "a stream may appear once per launch";
                if (!want && g == own_bad) want = own_text;
            }
            const char* got = refuse(G, gmax, chunk_ok != 0, s, n_streams, own_bad);
            if ((got == nullptr) != (want == nullptr) || (got && strcmp(got, want) != 0)) {
                printf("G %d chunk_ok %d streams %d %d %d own_bad %d: '%s' for '%s'\n", G, chunk_ok, a, b, c, own_bad, got ? got : "(none)", want ? want : "(none)");
                return false;
            }
            n++;
        }
    printf("preamble %ld\n", n);
    return true;
}
