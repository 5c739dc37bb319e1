// Driver of tests/test_sched_logic_cpu.py: csrc/sched_logic.h alone, plain g++.  Reads commands on stdin, prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

static const SlotField INT_FIELDS[] = {SF_TSEQ, SF_TSLOT, SF_FINISHED, SF_MAXFRAMES, SF_NFRAMES, SF_NPROMPT, SF_MASKEOS, SF_TOPK, SF_PTOPK, SF_NTRAIL, SF_OPEN};
static const SlotField FLT_FIELDS[] = {SF_TEMP, SF_TOPP, SF_PEN, SF_PTEMP, SF_PTOPP};

static void dump(SlotTable& t, int b) { // "row" + the 11 int fields, t_pos[4], the 5 float fields of slot b
    printf("row");
    for (SlotField f : INT_FIELDS) printf(" %d", t.hi(f)[b]);
    for (int s = 0; s < 4; s++) printf(" %d", t.hi(SF_TPOS)[4 * b + s]);
    for (SlotField f : FLT_FIELDS) printf(" %.9g", t.hf(f)[b]);
    printf("\n");
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "key") { // key W sampled pen pred trail gate
            int w; FrameVariant v;
            std::cin >> w >> v.sampled >> v.pen >> v.pred >> v.trail >> v.gate;
            printf("%d\n", v.key(w));
        } else if (cmd == "layout") { // layout B -> word offsets of the rows + the block size
            int B; std::cin >> B;
            SlotTable t(B);
            for (int f = 0; f <= SF_COUNT; f++) printf("%d ", t.off[f]);
            printf("%zu\n", t.host.size());
        } else if (cmd == "variant" || cmd == "stall") {
            // B, then per slot: has_request live temperature penalty pred_temperature n_trail open_request host_open finished n_frames max_frames
            int B; std::cin >> B;
            SlotTable t(B);
            std::vector<GenRequest> reqs(B);
            for (int b = 0; b < B; b++) {
                int has, live, open_req, host_open, fin, nf, maxf; GenRequest& r = reqs[b];
                std::cin >> has >> live >> r.sampler.temperature >> r.opts.repetition_penalty >> r.opts.predictor_temperature >> r.n_trail >> open_req >> host_open >> fin >> nf >> maxf;
                r.open = open_req != 0; r.max_steps = maxf;
                if (has) t.load(b, r);
                t.live[b] = (char)live; t.hi(SF_OPEN)[b] = host_open; t.hi(SF_FINISHED)[b] = fin; t.hi(SF_NFRAMES)[b] = nf;
            }
            if (cmd == "stall") { printf("%d\n", (int)t.all_live_stalled()); continue; }
            const FrameVariant v = live_variant(t);
            printf("%d %d %d %d %d\n", (int)v.sampled, (int)v.pen, (int)v.pred, (int)v.trail, (int)v.gate);
        } else if (cmd == "table") { // table B b n_frames: fresh row, loaded row, routed live row, row after reset, then t_seq/t_slot/t_pos of every slot
            int B, b, nf; std::cin >> B >> b >> nf;
            SlotTable t(B);
            dump(t, b);
            GenRequest r; r.n_prompt = 5; r.max_steps = 77; r.mask_eos = true; r.sampler.temperature = 0.625f; r.sampler.top_k = 13; r.sampler.top_p = 0.75f;
            r.opts.repetition_penalty = 1.5f; r.opts.predictor_temperature = 0.25f; r.opts.predictor_top_k = 9; r.opts.predictor_top_p = 0.5f; r.n_trail = 6; r.open = true;
            t.load(b, r);
            printf("req %d\n", (int)(t.req[b] == &r));
            dump(t, b);
            t.live[b] = 1; t.hi(SF_NFRAMES)[b] = nf; t.hi(SF_OPEN)[b] = 1;
            t.route();
            for (int s = 0; s < B; s++) dump(t, s);
            t.live[b] = 0; t.reset(b); t.route();
            printf("req %d\n", (int)(t.req[b] == nullptr));
            dump(t, b);
        } else if (cmd == "pack") { // pack n_max R, then per request: n_rows slot; row t of request i is filled with 100 * i + t
            int n_max, R; std::cin >> n_max >> R;
            std::vector<std::vector<float>> rows(R); std::vector<PromptRef> batch;
            for (int i = 0; i < R; i++) {
                int n, slot; std::cin >> n >> slot;
                rows[i].resize((size_t)n * Q3_EMBD);
                for (int t = 0; t < n; t++) std::fill_n(rows[i].begin() + (size_t)t * Q3_EMBD, Q3_EMBD, (float)(100 * i + t));
                batch.push_back({rows[i].data(), n, slot});
            }
            PrefillCursor c; std::vector<std::pair<int, int>> lasts;
            std::vector<float> stage((size_t)n_max * Q3_EMBD); std::vector<int32_t> seq(n_max), slot(n_max), pos((size_t)4 * n_max);
            while (c.req < batch.size()) {
                std::fill(stage.begin(), stage.end(), -1.0f);
                const int n = pack_prefill_chunk(batch, c, n_max, stage.data(), seq.data(), slot.data(), pos.data(), lasts);
                printf("chunk %d\nseq", n);
                for (int i = 0; i < n; i++) printf(" %d", seq[i]);
                printf("\nslot");
                for (int i = 0; i < n; i++) printf(" %d", slot[i]);
                printf("\npos");
                for (int i = 0; i < 4 * n; i++) printf(" %d", pos[i]);
                printf("\nlasts");
                for (auto& l : lasts) printf(" %d:%d", l.first, l.second);
                printf("\nstage");
                for (int i = 0; i < n_max; i++) { // every element of a staged row holds the row's constant (-1: untouched), else "bad"
                    const float* p = stage.data() + (size_t)i * Q3_EMBD;
                    bool same = true;
                    for (int k = 1; k < Q3_EMBD; k++) same = same && p[k] == p[0];
                    if (same) printf(" %g", p[0]); else printf(" bad");
                }
                printf("\n");
            }
            printf("cursor %zu %d\n", c.req, c.tok);
        } else if (cmd == "stage") { // stage cap n, then n sizes (-1: reset): per size "offset used", offset -1 = does not fit
            size_t cap; int n; std::cin >> cap >> n;
            StageCursor c; c.cap = cap;
            for (int i = 0; i < n; i++) {
                long long b; std::cin >> b;
                if (b < 0) { c.reset(); printf("reset %zu\n", c.used); continue; }
                const size_t at = c.take((size_t)b);
                printf("%lld %zu\n", at == StageCursor::NONE ? -1LL : (long long)at, c.used);
            }
        } else { fprintf(stderr, "unknown command %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
