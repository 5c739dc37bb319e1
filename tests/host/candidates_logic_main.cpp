// Driver of tests/test_candidates_cpu.py: the candidate-set rules of csrc/sched_logic.h alone, plain g++.  Reads commands on stdin, prints
// one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "refusal") { // refusal n max_batch null_seeds null_ids null_trail n_trail max_prompt ggml -> "ok" or the reason
            int n, max_batch, null_seeds, null_ids, null_trail, n_trail, max_prompt, ggml;
            std::cin >> n >> max_batch >> null_seeds >> null_ids >> null_trail >> n_trail >> max_prompt >> ggml;
            const uint64_t seed = 0; int64_t id = 0; const int32_t trail = 0; // never read: the rule looks at the pointers only
            const char* why = candidates_refusal(n, max_batch, null_seeds ? nullptr : &seed, null_ids ? nullptr : &id, null_trail ? nullptr : &trail,
                                                 n_trail, max_prompt, ggml != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "take") { // take free_slots free_codec limit_rows n, then per queue entry: rows want_pcm set -> the count taken
            int free_slots, free_codec, limit, n;
            std::cin >> free_slots >> free_codec >> limit >> n;
            std::vector<QueueEntry> q;
            for (int i = 0; i < n; i++) {
                int rows, pcm; long long set;
                std::cin >> rows >> pcm >> set;
                q.push_back({rows, pcm != 0, (int64_t)set});
            }
            printf("%d\n", admission_take(q, free_slots, free_codec, limit != 0));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
