// Driver of tests/test_stem_cpu.py: the rules of [EXT] prompt stems in csrc/sched_logic.h alone, plain g++.  Reads commands on stdin, prints
// one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <random>
#include <string>
#include <tuple>

using namespace q3;

namespace {
// one packed token as the engine sees it: where it came from, where it goes, what travels with it
struct Entry {
    int req, tok, seq, slot, pos[4];
    bool last, fb; int fb_frame; // fb: a feedback row (not staged); fb_frame: its frame
    float first;                 // staged rows: the first float of the row as staged
    bool operator==(const Entry& o) const {
        return std::tie(req, tok, seq, slot, pos[0], pos[1], pos[2], pos[3], last, fb, fb_frame, first) ==
               std::tie(o.req, o.tok, o.seq, o.slot, o.pos[0], o.pos[1], o.pos[2], o.pos[3], o.last, o.fb, o.fb_frame, o.first);
    }
};
// packs the whole batch in chunks of the given widths (cycled) and lists every token; the cursor tells which (req, tok) a token is
std::vector<Entry> pack_all(const std::vector<PromptRef>& batch, const std::vector<int>& widths, int* n_chunks) {
    std::vector<Entry> out;
    PrefillCursor cur;
    std::vector<std::pair<int, int>> lasts; std::vector<FbRun> fb;
    size_t total = 0;
    for (const PromptRef& r : batch) total += (size_t)admission_rows(r.n, r.n_skip, r.n_fb);
    *n_chunks = 0;
    for (size_t done = 0, w = 0; done < total; w++) {
        const int n_max = std::min<int>((int)(total - done), widths[w % widths.size()]);
        std::vector<float> stage((size_t)n_max * Q3_EMBD, -1.0f);
        std::vector<int32_t> seq(n_max), slot(n_max), pos((size_t)4 * n_max);
        PrefillCursor walk = cur;
        const int n = pack_prefill_chunk(batch, cur, n_max, stage.data(), seq.data(), slot.data(), pos.data(), lasts, &fb);
        if (n != n_max) { printf("chunk of %d rows where %d were due\n", n, n_max); exit(1); }
        for (int i = 0; i < n; i++) { // replay the cursor: the packer's own rule, token by token
            const PromptRef& r = batch[walk.req];
            if (walk.tok < r.n_skip) walk.tok = r.n_skip;
            Entry e{};
            e.req = (int)walk.req; e.tok = walk.tok; e.seq = seq[i]; e.slot = slot[i];
            for (int s = 0; s < 4; s++) e.pos[s] = pos[(size_t)4 * i + s];
            for (auto& l : lasts) if (l.second == i) { e.last = true; if (l.first != e.req) { printf("lasts names request %d at a row of %d\n", l.first, e.req); exit(1); } }
            for (const FbRun& f : fb) if (i >= f.row && i < f.row + f.n) { e.fb = true; e.fb_frame = f.frame + (i - f.row); if (f.req != e.req) { printf("FbRun names the wrong request\n"); exit(1); } }
            e.first = e.fb ? 0.0f : stage[(size_t)i * Q3_EMBD];
            if (!e.fb) for (int k = 0; k < Q3_EMBD; k += 511) if (stage[(size_t)i * Q3_EMBD + k] != r.rows[(size_t)e.tok * Q3_EMBD + k]) { printf("staged row differs from the prompt row\n"); exit(1); }
            out.push_back(e);
            if (walk.tok == r.n + r.n_fb - 1) { walk.req++; walk.tok = 0; } else walk.tok++;
        }
        if (walk.req != cur.req) { printf("cursor replay diverged\n"); exit(1); }
        done += (size_t)n; (*n_chunks)++;
    }
    return out;
}
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "refusal") { // refusal n max_prompt live ggml null_rows -> "ok" or the reason
            int n, max_prompt, live, ggml, null_rows;
            std::cin >> n >> max_prompt >> live >> ggml >> null_rows;
            std::vector<float> rows((size_t)std::max(n, 1) * Q3_EMBD, 0.5f);
            const char* why = stem_refusal(null_rows ? nullptr : rows.data(), n, max_prompt, live, ggml != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "set") { // set known state -> "ok" or the reason
            int known, state;
            std::cin >> known >> state;
            const char* why = stem_set_refusal(known != 0, state);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "of") { // of asked engine_level -> the stem that applies
            int asked, eng;
            std::cin >> asked >> eng;
            printf("%d\n", stem_of_request(asked, eng));
        } else if (cmd == "takes") { // takes state n n_prompt score differ_row differ_col negzero -> 0 / 1
            // the stem: n rows of distinct values; the prompt: n_prompt rows that start with them, then float (differ_row, differ_col) of the
            // prompt is changed when differ_row >= 0 (negzero: a +0 of the stem becomes -0 in the prompt instead: equal as floats, not as bytes)
            int state, n, n_prompt, score, drow, dcol, negzero;
            std::cin >> state >> n >> n_prompt >> score >> drow >> dcol >> negzero;
            std::vector<float> stem((size_t)n * Q3_EMBD), prompt((size_t)std::max(n_prompt, 1) * Q3_EMBD);
            for (size_t i = 0; i < stem.size(); i++) stem[i] = (float)(i % 1009) * 0.25f + 1.0f;
            for (size_t i = 0; i < prompt.size(); i++) prompt[i] = i < stem.size() ? stem[i] : -3.0f;
            if (drow >= 0) {
                const size_t at = (size_t)drow * Q3_EMBD + dcol;
                if (negzero) { if (at < stem.size()) stem[at] = 0.0f; prompt[at] = -0.0f; }
                else prompt[at] = prompt[at] + 1.0f;
            }
            printf("%d\n", stem_takes(state, n, stem.data(), prompt.data(), n_prompt, score != 0) ? 1 : 0);
        } else if (cmd == "takes_null") { // a stem without rows or a request without a prompt never takes
            std::vector<float> rows(Q3_EMBD, 1.0f);
            printf("%d %d\n", stem_takes(Q3TTS_STEM_READY, 1, nullptr, rows.data(), 2, false) ? 1 : 0, stem_takes(Q3TTS_STEM_READY, 1, rows.data(), nullptr, 2, false) ? 1 : 0);
        } else if (cmd == "rows") { // rows n_prompt n_skip n_prefix -> what admission counts
            int a, b, c;
            std::cin >> a >> b >> c;
            printf("%d\n", admission_rows(a, b, c));
        } else if (cmd == "take") { // take free_slots free_codec limit max_rows k (rows want_pcm set) x k -> admission_take
            int fs, fc, lim, k; long long mr;
            std::cin >> fs >> fc >> lim >> mr >> k;
            std::vector<QueueEntry> q;
            for (int i = 0; i < k; i++) { int rows, pcm; long long set; std::cin >> rows >> pcm >> set; q.push_back({rows, pcm != 0, (int64_t)set}); }
            printf("%d\n", admission_take(q, fs, fc, lim != 0, (size_t)mr));
        } else if (cmd == "store") { // store n n_layer n_kv -> pages bytes
            int n, nl, nk;
            std::cin >> n >> nl >> nk;
            printf("%d %lld\n", stem_pages(n), (long long)stem_store_bytes(n, nl, nk));
        } else if (cmd == "recyclable") { // recyclable creator holders state -> 0 / 1: the preamble's rule, which stems use as it is
            int creator, holders, state;
            std::cin >> creator >> holders >> state;
            PreambleRefs p;
            p.creator = creator != 0; p.holders = holders; p.state = state;
            printf("%d\n", preamble_recyclable(p) ? 1 : 0);
        } else if (cmd == "fresh") {
            PreambleRefs p;
            printf("%d %d %d %d\n", p.creator ? 1 : 0, p.holders, p.state, preamble_recyclable(p) ? 1 : 0);
        } else if (cmd == "packer") { // packer seed n_batches -> "ok <tokens> <skipped> <chunks>" or what differs
            // random batches: packing with skips gives exactly the plain packing's entries with the skipped ones removed
            unsigned seed; int n_batches;
            std::cin >> seed >> n_batches;
            std::mt19937 rng(seed);
            auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
            long long tokens = 0, skipped = 0, chunks = 0;
            bool ok = true;
            for (int b = 0; b < n_batches && ok; b++) {
                const int n_req = rnd(1, 6);
                std::vector<std::vector<float>> rows(n_req);
                std::vector<PromptRef> plain, skip;
                for (int i = 0; i < n_req; i++) {
                    const int n = rnd(1, 70), n_fb = rnd(0, 3) == 0 ? rnd(1, 5) : 0;
                    const int n_skip = rnd(0, 2) == 0 ? 0 : rnd(0, n - 1); // a taken stem is shorter than the prompt
                    rows[i].resize((size_t)n * Q3_EMBD);
                    for (size_t k = 0; k < rows[i].size(); k++) rows[i][k] = (float)(i * 1000 + (int)(k / Q3_EMBD)) + (float)(k % Q3_EMBD) / 4096.0f;
                    plain.push_back({rows[i].data(), n, 10 + i, n_fb, 0});
                    skip.push_back({rows[i].data(), n, 10 + i, n_fb, n_skip});
                }
                std::vector<int> wa, wb;
                for (int k = 0; k < 4; k++) { wa.push_back(rnd(1, 64)); wb.push_back(rnd(1, 64)); } // the two packings are chunked differently, too
                int ca = 0, cb = 0;
                std::vector<Entry> a = pack_all(plain, wa, &ca), s = pack_all(skip, wb, &cb), want;
                for (const Entry& e : a) if (e.tok >= skip[e.req].n_skip) want.push_back(e); else skipped++;
                if (!(want == s)) { printf("batch %d: the skipping packer differs from the plain one with the skipped entries removed\n", b); ok = false; }
                for (const Entry& e : s) if (e.seq != skip[e.req].slot || e.slot != e.tok || e.pos[0] != e.tok || e.pos[1] != e.tok || e.pos[2] != e.tok || e.pos[3] != 0) { printf("batch %d: routing\n", b); ok = false; break; }
                tokens += (long long)s.size(); chunks += cb;
            }
            if (ok) printf("ok %lld %lld %lld\n", tokens, skipped, chunks);
        } else if (cmd == "score_runs") { // score_runs seed n -> "ok": score_head_runs on a batch with skipping wave-mates equals the runs read off the packing
            unsigned seed; int n_batches;
            std::cin >> seed >> n_batches;
            std::mt19937 rng(seed);
            auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
            bool ok = true;
            for (int b = 0; b < n_batches && ok; b++) {
                const int n_req = rnd(1, 5);
                std::vector<std::vector<float>> rows(n_req);
                std::vector<PromptRef> batch; std::vector<char> score;
                for (int i = 0; i < n_req; i++) {
                    const bool sc = rnd(0, 1) == 1;
                    const int n = rnd(1, 50), n_fb = sc ? rnd(0, 6) : 0, n_skip = sc ? 0 : rnd(0, n - 1);
                    rows[i].assign((size_t)n * Q3_EMBD, 1.0f);
                    batch.push_back({rows[i].data(), n, i, n_fb, n_skip}); score.push_back(sc);
                }
                PrefillCursor cur; std::vector<std::pair<int, int>> lasts; std::vector<FbRun> fb;
                size_t total = 0;
                for (const PromptRef& r : batch) total += (size_t)admission_rows(r.n, r.n_skip, r.n_fb);
                for (size_t done = 0; done < total && ok;) {
                    const int n_max = std::min<int>((int)(total - done), rnd(1, 40));
                    std::vector<float> stage((size_t)n_max * Q3_EMBD);
                    std::vector<int32_t> seq(n_max), slot(n_max), pos((size_t)4 * n_max);
                    const PrefillCursor before = cur;
                    const int n = pack_prefill_chunk(batch, cur, n_max, stage.data(), seq.data(), slot.data(), pos.data(), lasts, &fb);
                    const std::vector<ScoreRun> runs = score_head_runs(batch, score, before, n);
                    std::vector<int> want_frame(n, -1), got_frame(n, -1);
                    for (int i = 0; i < n; i++) if (score[seq[i]] && slot[i] >= batch[seq[i]].n - 1) want_frame[i] = slot[i] - (batch[seq[i]].n - 1); // slot ids are the request indices here
                    for (const ScoreRun& r : runs) for (int k = 0; k < r.n; k++) { if (seq[r.row + k] != r.req) ok = false; got_frame[r.row + k] = r.frame + k; }
                    if (want_frame != got_frame) ok = false;
                    done += (size_t)n;
                }
                if (!ok) printf("batch %d: score runs differ\n", b);
            }
            if (ok) printf("ok\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
