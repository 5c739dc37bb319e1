// Driver of tests/test_logprobs_cpu.py, plain g++: the frame-variant key with the log-probability bit (csrc/sched_logic.h) and the error of
// q3_expf (include/q3tts_spec.h) against double exp on [-88, 0].  Reads commands on stdin, prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "key") { // key width sampled pen pred trail gate lp
            int w; FrameVariant v; int f[6];
            std::cin >> w >> f[0] >> f[1] >> f[2] >> f[3] >> f[4] >> f[5];
            v.sampled = f[0]; v.pen = f[1]; v.pred = f[2]; v.trail = f[3]; v.gate = f[4]; v.lp = f[5];
            printf("%d\n", v.key(w));
        } else if (cmd == "variant") { // variant n, then n lines "live logprobs": the lp bit of live_variant
            int n; std::cin >> n;
            SlotTable t(n);
            std::vector<GenRequest> reqs(n);
            for (int b = 0; b < n; b++) {
                int live, lp; std::cin >> live >> lp;
                reqs[b].logprobs = lp != 0; reqs[b].sampler.temperature = 0.0f;
                t.load(b, reqs[b]); t.live[b] = (char)live;
            }
            const FrameVariant v = live_variant(t);
            printf("%d %d %d %d %d %d\n", (int)v.sampled, (int)v.pen, (int)v.pred, (int)v.trail, (int)v.gate, (int)v.lp);
        } else if (cmd == "expf") { // expf n: q3_expf against double exp at n evenly spaced x and every 64th float of each range
            // line 1: [-87, 0], worst error in f32 ulps of exp(x) and where; line 2: [-88, -87), where q3_expf returns 0 by definition: worst ABSOLUTE error
            long n; std::cin >> n;
            double worst = 0, at = 0, worst_abs = 0;
            auto probe = [&](float x) {
                const double want = std::exp((double)x), got = (double)q3_expf(x);
                if (x < -87.0f) { worst_abs = std::fmax(worst_abs, std::fabs(got - want)); return; }
                int e; std::frexp(want, &e);                       // want in [2^(e-1), 2^e): one f32 ulp = 2^(e-24)
                const double err = std::fabs(got - want) / std::ldexp(1.0, e - 24);
                if (err > worst) { worst = err; at = x; }
            };
            for (long i = 0; i <= n; i++) probe((float)(-88.0 * (double)i / (double)n));
            for (uint32_t b = q3_f32_bits(-1e-6f); b <= q3_f32_bits(-88.0f); b += 64) probe(q3_bits_f32(b));
            probe(0.0f); probe(-87.0f); probe(-88.0f);
            printf("%.6f %.9g\n%.6g\n", worst, at, worst_abs);
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
