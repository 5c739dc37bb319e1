// Driver of tests/test_loudness_ref_cpu.py: the host half of [EXT] loudness (csrc/loudness.h) -- the tables, the segmented evaluation, the
// gate, the gain helper, the launch check and the submit rule -- alone, plain g++ under the host sanitizers.  Reads commands on stdin, prints
// one result line per answer.  Doubles and floats travel as hex bit patterns, so that nothing is rounded on the way.
#include "../../qwen3-tts-rust_amd/csrc/loudness.h"
#include "stage_preamble.h"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

using namespace q3;

static void put(double v) { uint64_t b; memcpy(&b, &v, 8); printf("%016llx ", (unsigned long long)b); }
static double get_double() { std::string s; std::cin >> s; const uint64_t b = std::stoull(s, nullptr, 16); double v; memcpy(&v, &b, 8); return v; }
static float get_float() { std::string s; std::cin >> s; const uint32_t b = (uint32_t)std::stoul(s, nullptr, 16); float v; memcpy(&v, &b, 4); return v; }

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "coefs") { // coefs fs -> the ten coefficients
            double fs, c[10];
            std::cin >> fs;
            loud_coefs(fs, c);
            for (double v : c) put(v);
            printf("\n");
        } else if (cmd == "tables") { // tables -> coef[10] then m[16]
            LoudTables t;
            loud_tables(&t);
            for (double v : t.coef) put(v);
            for (double v : t.m) put(v);
            printf("\n");
        } else if (cmd == "run") { // run pos n_chunks T.. then sum(T) floats -> one line of rows (energy peak ..), one line of the state
            long long pos; int nc;
            std::cin >> pos >> nc;
            std::vector<long long> T((size_t)nc);
            long long total = 0;
            for (auto& t : T) { std::cin >> t; total += t; }
            std::vector<float> x((size_t)total + 1);
            for (long long i = 0; i < total; i++) x[(size_t)i] = get_float();
            LoudTables t;
            loud_tables(&t);
            double state[Q3_LOUD_STATE] = {0, 0, 0, 0, 0, 0};
            long long at = 0;
            for (int c = 0; c < nc; c++) {
                std::vector<double> rows((size_t)(loud_blocks(pos + at, T[(size_t)c]) + 1) * 2);
                const int64_t n = loud_chunk_host(t, x.data() + at, T[(size_t)c], pos + at, state, rows.data());
                if (n != loud_blocks(pos + at, T[(size_t)c])) { fprintf(stderr, "row count differs from loud_blocks\n"); return 3; }
                for (int64_t i = 0; i < 2 * n; i++) put(rows[(size_t)i]);
                at += T[(size_t)c];
            }
            printf("\n");
            for (double v : state) put(v);
            printf("\n");
        } else if (cmd == "gate") { // gate n then 2 n doubles -> integrated momentary peak n_blocks n_gated
            int n;
            std::cin >> n;
            std::vector<double> rows((size_t)(n > 0 ? n : 0) * 2 + 1);
            for (int i = 0; i < 2 * n; i++) rows[(size_t)i] = get_double();
            LoudResult r;
            loud_gate(rows.data(), n, &r);
            put(r.integrated_lufs); put(r.momentary_max_lufs); put(r.peak_dbfs);
            printf("%d %d\n", r.n_blocks, r.n_gated);
        } else if (cmd == "gain") { // gain measured target -> tenths of a dB
            const double a = get_double(), b = get_double();
            printf("%d\n", loud_gain_db10(a, b));
        } else if (cmd == "blocks") { // blocks pos T
            long long pos, T;
            std::cin >> pos >> T;
            printf("%lld\n", (long long)loud_blocks(pos, T));
        } else if (cmd == "launch") { // launch G max_group T n_streams nulls, then G x (slot metered pos) -> refusal or "ok"
            int G, gmax, n_streams, nulls;
            long long T;
            std::cin >> G >> gmax >> T >> n_streams >> nulls;
            std::vector<int32_t> slots, met; std::vector<int64_t> pos;
            for (int g = 0; g < G; g++) { int s, m; long long p; std::cin >> s >> m >> p; slots.push_back(s); met.push_back(m); pos.push_back(p); }
            slots.push_back(0); met.push_back(0); pos.push_back(0);   // never read: keeps data() valid at G <= 0
            const char* why = loudness_launch_refusal(G, gmax, T, nulls == 1 ? nullptr : slots.data(), n_streams, nulls == 2 ? nullptr : met.data(),
                                                      nulls == 3 ? nullptr : pos.data());
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "submit") { // submit have_codec -> refusal or "ok"
            int have_codec;
            std::cin >> have_codec;
            const char* why = loudness_submit_refusal(have_codec != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "preamble") { // preamble -> "preamble <cases>": the shared checks in their order (stage_preamble.h)
            if (!check_stage_preamble([](int G, int gmax, bool chunk_ok, const int32_t* s, int n, int bad) {
                    int32_t met[4] = {1, 1, 1, 1}; int64_t pos[4];
                    for (int g = 0; g < 4; g++) pos[g] = g == bad ? 7 : 1920;
                    return loudness_launch_refusal(G, gmax, chunk_ok ? 1920 : 1000, s, n, met, pos);
                }, "chunk length is no positive multiple of 1920 samples", "stream position is no multiple of 1920 samples")) return 1;
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
