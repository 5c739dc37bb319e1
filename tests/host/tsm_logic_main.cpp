// Driver of tests/test_tsm_ref_cpu.py: the host half of [EXT] speaking rate -- the counts and the submit rule in csrc/sched_logic.h, the
// window tables, the visit order and the launch check in csrc/tsm.h -- alone, plain g++ under the host sanitizers.  Reads commands on stdin,
// prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/tsm.h"
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
        if (cmd == "rate") { // rate pct -> refusal or "ok"
            int pct;
            std::cin >> pct;
            const char* why = tsm_rate_why_not(pct);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "samples") { // samples pct n_native final -> "frames samples"
            int pct, fin;
            long long n;
            std::cin >> pct >> n >> fin;
            printf("%lld %lld\n", (long long)tsm_frames(pct, n, fin != 0), (long long)tsm_out_samples(pct, n, fin != 0));
        } else if (cmd == "windows") { // windows -> the bit patterns of w then w2 in hex, one line
            std::vector<float> w(Q3_TSM_HOP), w2(Q3_TSM_HOP);
            tsm_windows(w.data(), w2.data());
            for (const auto* t : {&w, &w2}) for (float v : *t) { uint32_t b; memcpy(&b, &v, 4); printf("%08x ", b); }
            printf("\n");
        } else if (cmd == "order") { // order -> "ok" when o() is a bijection of [-240, 240] onto [0, 480] with the inverse given
            bool ok = true;
            std::vector<int> seen(2 * Q3_TSM_SEARCH + 1, 0);
            for (int d = -Q3_TSM_SEARCH; d <= Q3_TSM_SEARCH; d++) {
                const int o = tsm_visit_order(d);
                if (o < 0 || o > 2 * Q3_TSM_SEARCH || seen[(size_t)o]++ || tsm_offset_of_order(o) != d) ok = false;
            }
            ok = ok && tsm_visit_order(0) == 0 && tsm_visit_order(-1) == 1 && tsm_visit_order(1) == 2 && tsm_visit_order(-240) == 479 && tsm_visit_order(240) == 480;
            printf("%s\n", ok ? "ok" : "bad");
        } else if (cmd == "launch") { // launch G max_group T flush n_streams, then G x (slot pct enc) -> refusal or "ok"
            int G, gmax, flush, n_streams;
            long long T;
            std::cin >> G >> gmax >> T >> flush >> n_streams;
            std::vector<int32_t> slots, pct, enc;
            for (int g = 0; g < G; g++) { int s, p, e; std::cin >> s >> p >> e; slots.push_back(s); pct.push_back(p); enc.push_back(e); }
            slots.push_back(0); pct.push_back(0); enc.push_back(0);   // never read: keeps data() valid at G <= 0
            const char* why = tsm_launch_refusal(G, gmax, T, flush != 0, slots.data(), n_streams, pct.data(), enc.data());
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "submit") { // submit pct rate enc max_steps cap_bytes have_codec -> refusal or "ok"
            int pct, rate, enc, max_steps, have_codec;
            long long cap;
            std::cin >> pct >> rate >> enc >> max_steps >> cap >> have_codec;
            const q3tts_pcm_format f{rate, enc};
            const char* why = tsm_submit_refusal(pct, f, max_steps, cap, have_codec != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "preamble") { // preamble -> "preamble <cases>": the shared checks in their order (stage_preamble.h)
            if (!check_stage_preamble([](int G, int gmax, bool chunk_ok, const int32_t* s, int n, int bad) {
                    int32_t pct[4], enc[4] = {Q3_PCM_F32, Q3_PCM_S16, Q3_PCM_F32, Q3_PCM_S16};
                    for (int g = 0; g < 4; g++) pct[g] = g == bad ? 49 : 125;
                    return tsm_launch_refusal(G, gmax, chunk_ok ? 1920 : 1000, false, s, n, pct, enc);
                }, "chunk length is no positive multiple of 1920 samples", "speech rate out of range [50, 200]")) return 1;
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
