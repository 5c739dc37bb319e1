// Driver of tests/test_resume_cpu.py: the resume rules of csrc/sched_logic.h alone, plain g++.  Reads commands on stdin, prints one result
// line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "refusal") { // refusal n_prompt max_steps n_prefix null_codes open n_trail kv_rows n_codes, then n_codes codes -> "ok" or the reason
            int n_prompt, max_steps, n_prefix, null_codes, open, n_trail, n_codes; long long kv_rows;
            std::cin >> n_prompt >> max_steps >> n_prefix >> null_codes >> open >> n_trail >> kv_rows >> n_codes;
            std::vector<int32_t> codes(n_codes);
            for (auto& c : codes) std::cin >> c;
            const char* why = resume_refusal(n_prompt, max_steps, null_codes ? nullptr : codes.data(), n_prefix, open != 0, n_trail, kv_rows);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "pack") { // pack n_max R, then per request: n_rows slot n_fb; staged row t of request i holds 100 * i + t
            int n_max, R; std::cin >> n_max >> R;
            std::vector<std::vector<float>> rows(R); std::vector<PromptRef> batch;
            for (int i = 0; i < R; i++) {
                int n, slot, n_fb; std::cin >> n >> slot >> n_fb;
                rows[i].resize((size_t)n * Q3_EMBD);
                for (int t = 0; t < n; t++) std::fill_n(rows[i].begin() + (size_t)t * Q3_EMBD, Q3_EMBD, (float)(100 * i + t));
                batch.push_back({rows[i].data(), n, slot, n_fb});
            }
            PrefillCursor c; std::vector<std::pair<int, int>> lasts; std::vector<FbRun> fb;
            std::vector<float> stage((size_t)n_max * Q3_EMBD); std::vector<int32_t> seq(n_max), slot(n_max), pos((size_t)4 * n_max);
            while (c.req < batch.size()) {
                std::fill(stage.begin(), stage.end(), -1.0f);
                const int n = pack_prefill_chunk(batch, c, n_max, stage.data(), seq.data(), slot.data(), pos.data(), lasts, &fb);
                printf("chunk %d\nseq", n);
                for (int i = 0; i < n; i++) printf(" %d", seq[i]);
                printf("\nslot");
                for (int i = 0; i < n; i++) printf(" %d", slot[i]);
                printf("\npos");
                for (int i = 0; i < 4 * n; i++) printf(" %d", pos[i]);
                printf("\nlasts");
                for (auto& l : lasts) printf(" %d:%d", l.first, l.second);
                printf("\nfb");
                for (auto& f : fb) printf(" %d:%d:%d:%d", f.req, f.row, f.frame, f.n);
                printf("\nstaged");
                for (auto& s : staged_runs(n, fb)) printf(" %d+%d", s.first, s.second);
                printf("\nstage");
                for (int i = 0; i < n_max; i++) printf(" %g", stage[(size_t)i * Q3_EMBD]); // -1: untouched (a device-made row or past the chunk)
                printf("\n");
            }
        } else if (cmd == "load") { // load n_prompt n_prefix -> n_frames and routed position of a slot loaded with a resumed request
            GenRequest g; std::cin >> g.n_prompt >> g.n_prefix; g.max_steps = 40;
            SlotTable t(2);
            t.load(1, g); t.live[1] = 1; t.route();
            printf("%d %d %d %d %d %d\n", t.hi(SF_NFRAMES)[1], t.hi(SF_TSLOT)[1], t.hi(SF_TPOS)[4], t.hi(SF_TPOS)[5], t.hi(SF_TPOS)[6], t.hi(SF_TPOS)[7]);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
