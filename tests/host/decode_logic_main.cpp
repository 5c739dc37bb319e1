// Driver of tests/test_decode_cpu.py: the rules of [EXT] decoding given frames in csrc/sched_logic.h alone, plain g++.  Reads commands on
// stdin, prints one result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

static bool g_epochs = false; // "epochs 1": every task line carries a fourth field, the hand-over it came with
static std::vector<TaskHead> read_queue(int n) { // per task: request id, frame count, kind (C chunk, R reset, F fence)[, epoch]
    std::vector<TaskHead> q;
    for (int i = 0; i < n; i++) {
        long long req, epoch = 0; int frames; char kind;
        std::cin >> req >> frames >> kind;
        if (g_epochs) std::cin >> epoch;
        q.push_back({(int64_t)req, frames, kind == 'R' ? TASK_RESET : kind == 'F' ? TASK_FENCE : TASK_CHUNK, (int64_t)epoch});
    }
    return q;
}

static void print_pass(const Seating& s, const std::vector<TaskHead>& live, const std::vector<TaskHead>& low) { // "L<req>/<frames><kind> ... | dry"
    for (const Seat& c : s.seats) {
        const TaskHead& t = (c.low ? low : live)[c.index];
        printf("%c%lld/%d%c ", c.low ? 'D' : 'L', (long long)t.req, t.frames, t.kind == TASK_RESET ? 'R' : t.kind == TASK_FENCE ? 'F' : 'C');
    }
    printf("| %d\n", s.dry);
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "refusal") { // refusal n max_steps have_codec null_codes at code_0 residual -> "ok" or the reason
            // max(n, 0) valid frames (code_0 = 5, residuals 7); frame `at` (if >= 0) gets code_0 and, in column 15, the residual
            int n, max_steps, have_codec, null_codes, at, c0, res;
            std::cin >> n >> max_steps >> have_codec >> null_codes >> at >> c0 >> res;
            std::vector<int32_t> codes((size_t)std::max(n, 0) * 16 + 16, 7);
            for (int f = 0; f < std::max(n, 0); f++) codes[(size_t)f * 16] = 5;
            if (at >= 0) { codes[(size_t)at * 16] = c0; codes[(size_t)at * 16 + 15] = res; }
            const char* why = decode_refusal(null_codes ? nullptr : codes.data(), n, max_steps, have_codec != 0);
            printf("%s\n", why ? why : "ok");
        } else if (cmd == "epochs") { // epochs 0|1: how the task lines that follow are read
            int on;
            std::cin >> on;
            g_epochs = on != 0;
        } else if (cmd == "width") { // width n_cs max_batch
            int n_cs, b;
            std::cin >> n_cs >> b;
            printf("%d\n", decode_width(n_cs, b));
        } else if (cmd == "admit") { // admit queued free_cs holding width
            int q, f, h, w;
            std::cin >> q >> f >> h >> w;
            printf("%d\n", decode_admit(q, f, h, w));
        } else if (cmd == "seat") { // seat gmax dry n_live n_low, then the two queues -> one pass
            int gmax, dry, nl, nd;
            std::cin >> gmax >> dry >> nl >> nd;
            const std::vector<TaskHead> live = read_queue(nl), low = read_queue(nd);
            print_pass(seat_chunks(live, low, gmax, dry), live, low);
        } else if (cmd == "drain") { // drain gmax n_live n_low, then the two queues -> every pass until both are empty, then "end"
            int gmax, nl, nd, dry = 0;
            std::cin >> gmax >> nl >> nd;
            std::vector<TaskHead> live = read_queue(nl), low = read_queue(nd);
            while (!live.empty() || !low.empty()) {
                const Seating s = seat_chunks(live, low, gmax, dry);
                if (s.seats.empty()) { printf("stuck\n"); return 1; }
                print_pass(s, live, low);
                dry = s.dry;
                for (int l = 0; l < 2; l++) {
                    std::vector<TaskHead>& q = l ? low : live;
                    std::vector<int> idx;
                    for (const Seat& c : s.seats) if ((int)c.low == l) idx.push_back(c.index);
                    std::sort(idx.rbegin(), idx.rend());
                    for (int i : idx) q.erase(q.begin() + i);
                }
            }
            printf("end\n");
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
