// Driver of tests/test_volume_ref_cpu.py: the host half of [EXT] volume -- the range, the gain and the submit rule in csrc/sched_logic.h and
// the launch check in csrc/volume.h -- alone, plain g++ under the host sanitizers.  Reads commands on stdin, prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/volume.h"
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
        if (cmd == "volume") { // volume db10 -> refusal or "ok"
            int v;
            std::cin >> v;
            const char* why = volume_why_not(v);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "gain") { // gain db10 -> the bit pattern of G in hex
            int v;
            std::cin >> v;
            const float g = volume_gain(v);
            uint32_t b;
            memcpy(&b, &g, 4);
            printf("%08x\n", b);
        } else if (cmd == "launch") { // launch G max_group T n_streams nulls, then G x (slot db10) -> refusal or "ok"
            int G, gmax, n_streams, nulls;
            long long T;
            std::cin >> G >> gmax >> T >> n_streams >> nulls;
            std::vector<int32_t> slots, vol;
            for (int g = 0; g < G; g++) { int s, v; std::cin >> s >> v; slots.push_back(s); vol.push_back(v); }
            slots.push_back(0); vol.push_back(0);   // never read: keeps data() valid at G <= 0
            const char* why = volume_launch_refusal(G, gmax, T, nulls ? nullptr : slots.data(), n_streams, vol.data());
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "submit") { // submit db10 have_codec -> refusal or "ok"
            int v, have_codec;
            std::cin >> v >> have_codec;
            const char* why = volume_submit_refusal(v, have_codec != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "preamble") { // preamble -> "preamble <cases>": the shared checks in their order (stage_preamble.h)
            if (!check_stage_preamble([](int G, int gmax, bool chunk_ok, const int32_t* s, int n, int bad) {
                    int32_t db10[4];
                    for (int g = 0; g < 4; g++) db10[g] = g == bad ? 201 : 60;
                    return volume_launch_refusal(G, gmax, chunk_ok ? 1920 : 1000, s, n, db10);
                }, "chunk length is no positive multiple of 1920 samples", "volume out of range [-400, 200]")) return 1;
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
