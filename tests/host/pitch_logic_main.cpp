// Driver of tests/test_pitch_ref_cpu.py: the host half of [EXT] pitch -- the pair rule, the plan, the counts and the submit rule in
// csrc/sched_logic.h, the filter builder and the launch check in csrc/pitch.h -- alone, plain g++ under the host sanitizers.  Reads commands
// on stdin, prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/pitch.h"
#include "stage_preamble.h"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "pitch") { // pitch P -> refusal or "ok"
            int P;
            std::cin >> P;
            const char* why = pitch_why_not(P);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "pair") { // pair R P -> refusal or "ok"
            int R, P;
            std::cin >> R >> P;
            const char* why = prosody_pair_why_not(R, P);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "samples") { // samples R P n_native final -> "frames samples"
            int R, P, fin;
            long long n;
            std::cin >> R >> P >> n >> fin;
            printf("%lld %lld\n", (long long)pitch_frames(R, P, n, fin != 0), (long long)pitch_out_samples(R, P, n, fin != 0));
        } else if (cmd == "plan") { // plan P -> "L M n_taps taps_per_output" or "none"
            int P;
            std::cin >> P;
            PitchPlan p;
            if (pitch_plan(P, &p)) printf("%d %d %d %d\n", p.L, p.M, p.n_taps, p.taps_per_output);
            else printf("none\n");
        } else if (cmd == "filter") { // filter P -> the bit patterns of h32 in hex, one line
            int P;
            std::cin >> P;
            for (float v : pitch_filter(P)) { uint32_t b; memcpy(&b, &v, 4); printf("%08x ", b); }
            printf("\n");
        } else if (cmd == "tables") { // tables -> "floats taps offset_of_200 last_offset_plus_taps"
            const PitchTables t = pitch_tables();
            PitchPlan p;
            pitch_plan(Q3_PITCH_MAX, &p);
            printf("%zu %lld %d %d\n", t.all.size(), (long long)t.taps, t.off[PITCH_N - 1], t.off[PITCH_N - 1] + p.n_taps);
        } else if (cmd == "launch") { // launch G max_group T flush n_streams, then G x (slot rate pitch enc) -> refusal or "ok"
            int G, gmax, flush, n_streams;
            long long T;
            std::cin >> G >> gmax >> T >> flush >> n_streams;
            std::vector<int32_t> slots, rate, pitch, enc;
            for (int g = 0; g < G; g++) { int s, r, p, e; std::cin >> s >> r >> p >> e; slots.push_back(s); rate.push_back(r); pitch.push_back(p); enc.push_back(e); }
            slots.push_back(0); rate.push_back(0); pitch.push_back(0); enc.push_back(0);   // never read: keeps data() valid at G <= 0
            const char* why = pitch_launch_refusal(G, gmax, T, flush != 0, slots.data(), n_streams, rate.data(), pitch.data(), enc.data());
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "submit") { // submit R P sample_rate enc max_steps cap_bytes have_codec -> refusal or "ok"
            int R, P, rate, enc, max_steps, have_codec;
            long long cap;
            std::cin >> R >> P >> rate >> enc >> max_steps >> cap >> have_codec;
            const q3tts_pcm_format f{rate, enc};
            const char* why = pitch_submit_refusal(R, P, f, max_steps, cap, have_codec != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "preamble") { // preamble -> "preamble <cases>": the shared checks in their order (stage_preamble.h)
            if (!check_stage_preamble([](int G, int gmax, bool chunk_ok, const int32_t* s, int n, int bad) {
                    int32_t rate[4] = {100, 125, 80, 100}, pitch[4], enc[4] = {Q3_PCM_F32, Q3_PCM_S16, Q3_PCM_F32, Q3_PCM_S16};
                    for (int g = 0; g < 4; g++) pitch[g] = g == bad ? 49 : 80;
                    return pitch_launch_refusal(G, gmax, chunk_ok ? 1920 : 1000, false, s, n, rate, pitch, enc);
                }, "chunk length is no positive multiple of 1920 samples", "pitch out of range [50, 200]")) return 1;
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
