// Driver of tests/test_score_cpu.py: the scoring rules of csrc/sched_logic.h alone, plain g++.  Reads commands on stdin, prints one result
// line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "refusal") { // refusal null_prompt n_prompt max_prompt null_trail n_trail null_codes n max_steps kv_rows ggml n_codes, then the codes -> "ok" or the reason
            int null_prompt, n_prompt, max_prompt, null_trail, n_trail, null_codes, n, max_steps, ggml, n_codes; long long kv_rows;
            std::cin >> null_prompt >> n_prompt >> max_prompt >> null_trail >> n_trail >> null_codes >> n >> max_steps >> kv_rows >> ggml >> n_codes;
            std::vector<int32_t> codes(n_codes);
            for (auto& c : codes) std::cin >> c;
            const float prompt = 0.0f; const int32_t trail = 0; // never read: the rule looks at the pointers only
            const char* why = score_refusal(null_prompt ? nullptr : &prompt, n_prompt, max_prompt, null_trail ? nullptr : &trail, n_trail,
                                            null_codes ? nullptr : codes.data(), n, max_steps, kv_rows, ggml != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "runs") { // runs n_max R, then per request: n_rows n_frames score -> per chunk "chunk n: req:row:frame:n ..."
            int n_max, R; std::cin >> n_max >> R;
            std::vector<float> rows; std::vector<PromptRef> batch; std::vector<char> score; std::vector<int> n_rows(R);
            int most = 0;
            for (int i = 0; i < R; i++) {
                int frames, sc; std::cin >> n_rows[i] >> frames >> sc;
                batch.push_back({nullptr, n_rows[i], i, sc ? frames - 1 : frames}); // a score request: frames - 1 feedback rows; a resumed one: its prefix
                score.push_back((char)sc);
                most = std::max(most, n_rows[i]);
            }
            rows.assign((size_t)most * Q3_EMBD, 0.0f);
            for (auto& b : batch) b.rows = rows.data();
            PrefillCursor c; std::vector<std::pair<int, int>> lasts; std::vector<FbRun> fb;
            std::vector<float> stage((size_t)n_max * Q3_EMBD); std::vector<int32_t> seq(n_max), slot(n_max), pos((size_t)4 * n_max);
            while (c.req < batch.size()) {
                const PrefillCursor before = c;
                const int n = pack_prefill_chunk(batch, c, n_max, stage.data(), seq.data(), slot.data(), pos.data(), lasts, &fb);
                printf("chunk %d:", n);
                for (auto& r : score_head_runs(batch, score, before, n)) {
                    // every row of a run belongs to the run's request and sits at position n_rows - 1 + frame of its sequence
                    for (int j = 0; j < r.n; j++)
                        if (seq[r.row + j] != r.req || slot[r.row + j] != n_rows[r.req] - 1 + r.frame + j) { fprintf(stderr, "run row mismatch\n"); return 3; }
                    printf(" %d:%d:%d:%d", r.req, r.row, r.frame, r.n);
                }
                printf("\n");
            }
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
