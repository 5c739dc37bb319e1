// Driver of tests/test_preamble_cpu.py: the rules of [EXT] codec preambles in csrc/sched_logic.h alone, plain g++.  Reads commands on stdin,
// prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "refusal") { // refusal n max_steps have_codec null_codes at code_0 residual live max_positions -> "ok" or the reason
            // max(n, 0) valid frames (code_0 = 5, residuals 7); frame `at` (if >= 0) gets code_0 and, in column 15, the residual
            int n, max_steps, have_codec, null_codes, at, c0, res, live; long long max_pos;
            std::cin >> n >> max_steps >> have_codec >> null_codes >> at >> c0 >> res >> live >> max_pos;
            std::vector<int32_t> codes((size_t)std::max(n, 0) * 16 + 16, 7);
            for (int f = 0; f < std::max(n, 0); f++) codes[(size_t)f * 16] = 5;
            if (at >= 0) { codes[(size_t)at * 16] = c0; codes[(size_t)at * 16 + 15] = res; }
            const char* why = preamble_refusal(null_codes ? nullptr : codes.data(), n, max_steps, have_codec != 0, live, (int64_t)max_pos);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "recyclable") { // recyclable creator holders state -> 0 / 1
            int creator, holders, state;
            std::cin >> creator >> holders >> state;
            PreambleRefs p;
            p.creator = creator != 0; p.holders = holders; p.state = state;
            printf("%d\n", preamble_recyclable(p) ? 1 : 0);
        } else if (cmd == "fresh") { // a new preamble: its creator holds it, nobody else, building
            PreambleRefs p;
            printf("%d %d %d %d\n", p.creator ? 1 : 0, p.holders, p.state, preamble_recyclable(p) ? 1 : 0);
        } else if (cmd == "set") { // set known state -> "ok" or the reason
            int known, state;
            std::cin >> known >> state;
            const char* why = preamble_set_refusal(known != 0, state);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "of") { // of want_pcm asked engine_level -> the preamble the request is primed with
            int want_pcm, asked, eng;
            std::cin >> want_pcm >> asked >> eng;
            printf("%d\n", preamble_of_request(want_pcm != 0, asked, eng));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
