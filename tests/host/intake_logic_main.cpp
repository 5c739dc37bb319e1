// Driver of tests/test_intake_ref_cpu.py: the host half of [EXT] reference audio intake -- the plan, the sample count, the table builder, the
// clip check and the WAV header reader of csrc/intake.h -- alone, plain g++ under the host sanitizers.  Reads commands on stdin, prints one
// result line per answer.  A WAV file arrives as hex digits and is probed in a heap block of exactly its size, so that a read past the
// buffer is a sanitizer report.
#include "../../qwen3-tts-rust_amd/csrc/intake.h"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "plan") { // plan rate -> "L M N taps stride c tile lds_floats" or "refused: <why>"
            int rate;
            std::cin >> rate;
            IntakePlan p;
            if (const char* why = intake_rate_why_not(rate)) { printf("refused: %s\n", why); continue; }
            if (!intake_plan(rate, &p)) { printf("refused: no tile fits\n"); continue; }
            printf("%d %d %d %d %d %d %d %lld\n", p.L, p.M, p.n_taps, p.taps, p.stride, p.c, p.tile, p.n_taps ? (long long)intake_lds_floats(p, p.tile) : 0LL);
        } else if (cmd == "samples") { // samples rate n -> count or -1
            int rate; long long n;
            std::cin >> rate >> n;
            printf("%lld\n", (long long)intake_samples(rate, n));
        } else if (cmd == "filter") { // filter rate -> the taps' bit patterns in hex, one line
            int rate;
            std::cin >> rate;
            for (float v : intake_filter(rate)) { uint32_t b; memcpy(&b, &v, 4); printf("%08x ", b); }
            printf("\n");
        } else if (cmd == "phases") { // phases rate -> "ok" when the phase-major image holds every tap once, in place, and zeros elsewhere
            int rate;
            std::cin >> rate;
            IntakePlan p;
            if (!intake_plan(rate, &p)) { printf("refused\n"); continue; }
            const std::vector<float> h = intake_filter(rate), t = intake_table(p, h);
            bool ok = (int)t.size() == intake_table_floats(p) && p.stride % 4 == 0 && (int)h.size() == p.n_taps;
            for (int ph = 0; ok && p.n_taps && ph < p.L; ph++)
                for (int k = 0; k < p.stride; k++) {
                    const int i = ph + k * p.L;
                    const float want = i < p.n_taps ? h[(size_t)i] : 0.0f;
                    if (memcmp(&want, &t[(size_t)ph * p.stride + k], 4) != 0) ok = false;
                }
            printf("%s\n", ok ? "ok" : "bad");
        } else if (cmd == "clip") { // clip rate channels format downmix n_frames has_data -> refusal or "ok"
            int rate, ch, fmt, mix, has; long long n;
            std::cin >> rate >> ch >> fmt >> mix >> n >> has;
            static const char byte = 0;
            const q3tts_intake_clip c{has ? &byte : nullptr, n, rate, ch, fmt, mix};
            const char* why = has < 0 ? intake_refusal(nullptr) : intake_refusal(&c);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "wav") { // wav <hex digits or "-" for an empty file> -> "ok format channels rate bits offset frames" or "error: <why>"
            std::string hex;
            std::cin >> hex;
            if (hex == "-") hex.clear();
            const size_t n = hex.size() / 2;
            unsigned char* buf = new unsigned char[n ? n : 1];
            for (size_t i = 0; i < n; i++) buf[i] = (unsigned char)std::stoi(hex.substr(2 * i, 2), nullptr, 16);
            q3tts_wav_info w{};
            const char* why = wav_probe(n ? buf : (const void*)buf, (int64_t)n, &w);
            if (why) printf("error: %s\n", why);
            else if (w.data_offset < 0 || w.n_frames < 0 || w.data_offset + w.n_frames * w.channels * (w.bits / 8) > (int64_t)n) printf("error: PROBE RETURNED A RANGE PAST THE FILE\n");
            else printf("ok %d %d %d %d %lld %lld\n", w.sample_format, w.channels, w.sample_rate, w.bits, (long long)w.data_offset, (long long)w.n_frames);
            delete[] buf;
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
