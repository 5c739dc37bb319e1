// Driver of tests/test_pcm_out_ref_cpu.py: the host half of [EXT] output formats -- the rules in csrc/sched_logic.h and the plan, table
// builder and launch check in csrc/pcm_out.h -- alone, plain g++ under the host sanitizers.  Reads commands on stdin, prints one result line
// per answer.
#include "../../qwen3-tts-rust_amd/csrc/pcm_out.h"
#include "stage_preamble.h"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "plan") { // plan rate -> "L M N taps stride" or "unknown"
            int rate;
            std::cin >> rate;
            PcmPlan p;
            if (!pcm_plan(rate, &p)) printf("unknown\n");
            else printf("%d %d %d %d %d\n", p.L, p.M, p.n_taps, p.taps_per_phase, pcm_phase_stride(p));
        } else if (cmd == "filter") { // filter rate -> the taps' bit patterns in hex, one line
            int rate;
            std::cin >> rate;
            for (float v : pcm_filter(rate)) { uint32_t b; memcpy(&b, &v, 4); printf("%08x ", b); }
            printf("\n");
        } else if (cmd == "phases") { // phases rate -> "ok" when the phase-major image holds every tap once, in place, and zeros elsewhere
            int rate;
            std::cin >> rate;
            PcmPlan p;
            if (!pcm_plan(rate, &p)) { printf("unknown\n"); continue; }
            const std::vector<float> h = pcm_filter(rate), t = pcm_filter_phase_major(p, h);
            const int stride = pcm_phase_stride(p);
            bool ok = t.size() == (size_t)p.L * stride && stride % 4 == 0;
            for (int ph = 0; ok && ph < p.L; ph++)
                for (int k = 0; k < stride; k++) {
                    const int i = ph + k * p.L;
                    const float want = i < p.n_taps ? h[(size_t)i] : 0.0f;
                    if (memcmp(&want, &t[(size_t)ph * stride + k], 4) != 0) ok = false;
                }
            printf("%s\n", ok ? "ok" : "bad");
        } else if (cmd == "rule") { // rule rate enc have_codec null frames -> "<refusal or ok> | samples bytes"
            int rate, enc, have_codec, null_fmt;
            long long frames;
            std::cin >> rate >> enc >> have_codec >> null_fmt >> frames;
            const q3tts_pcm_format f{rate, enc};
            const char* why = pcm_format_refusal(null_fmt ? nullptr : &f, have_codec != 0);
            printf("%s | %lld %lld\n", why ? why : "ok", (long long)pcm_out_samples(f, frames), (long long)pcm_out_bytes(f, frames));
        } else if (cmd == "launch") { // launch G max_group T n_streams, then G x (slot rate enc) -> refusal or "ok"
            int G, gmax, n_streams;
            long long T;
            std::cin >> G >> gmax >> T >> n_streams;
            std::vector<int32_t> slots; std::vector<q3tts_pcm_format> fmt;
            for (int g = 0; g < G; g++) { int s, r, e; std::cin >> s >> r >> e; slots.push_back(s); fmt.push_back({r, e}); }
            slots.push_back(0); fmt.push_back({0, 0});   // never read: keeps data() valid at G <= 0
            const char* why = pcm_convert_refusal(G, gmax, T, slots.data(), n_streams, fmt.data());
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "preamble") { // preamble -> "preamble <cases>": the shared checks in their order (stage_preamble.h)
            if (!check_stage_preamble([](int G, int gmax, bool chunk_ok, const int32_t* s, int n, int bad) {
                    q3tts_pcm_format fmt[4];
                    for (int g = 0; g < 4; g++) fmt[g] = q3tts_pcm_format{g == bad ? 12345 : 16000, Q3_PCM_S16};
                    return pcm_convert_refusal(G, gmax, chunk_ok ? 1920 : 1000, s, n, fmt);
                }, "chunk length is no whole number of frames", "unknown sample rate")) return 1;
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
