// Driver of tests/test_codec_queue_cpu.py: the decoder thread's queue bookkeeping (CodecQueue, csrc/sched_logic.h) against a shadow kept
// here, alone, plain g++ under the host sanitizers.  200 random sequences of 300 operations -- reset, chunk and fence pushes of generating and
// decode-only requests, hand-overs opened and closed, a request purged, a step taken, a completion popped -- and after every one the queues,
// the pending count and what left are compared with the shadow.  It prints one "name count" line per figure and exits 1 at the first
// disagreement.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <random>

using namespace q3;

struct Job {
    int64_t id; bool decode;
    int pushed = 0;          // 0 nothing yet, 1 its reset, 2 its fence too
    int left = 0;            // the same, of what the queue gave out
    int64_t last_serial = 0; // of the chunks that left
};
typedef CodecQueue<Job> Queue;
struct Shadow { Job* job; TaskKind kind; int64_t serial; int frames; int64_t epoch; };

#define FAIL(...) do { std::printf("seq %d op %d: ", g_seq, g_op); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } while (0)
static int g_seq = 0, g_op = 0;

static std::vector<TaskHead> heads(const std::vector<Shadow>& q) {
    std::vector<TaskHead> h;
    for (const Shadow& t : q) h.push_back({t.job->id, t.frames, (int)t.kind, t.epoch});
    return h;
}
static void same(const std::deque<Queue::Task>& q, const std::vector<Shadow>& s, const char* which) {
    if (q.size() != s.size()) FAIL("%s queue holds %zu tasks, the shadow %zu", which, q.size(), s.size());
    for (size_t i = 0; i < s.size(); i++) {
        const Queue::Task& t = q[i];
        if (t.job != s[i].job || t.kind != s[i].kind || (int)t.codes.size() != 16 * s[i].frames || t.epoch != s[i].epoch ||
            (t.kind == TASK_CHUNK && t.codes[0] != s[i].serial))
            FAIL("%s queue differs from the shadow at %zu", which, i);
    }
}

int main() {
    long n_ops = 0, n_pushes = 0, n_takes = 0, n_steps = 0, n_held_takes = 0, n_purges = 0, n_purged = 0, n_pops = 0, n_handovers = 0, n_nested = 0;
    long n_multi = 0, n_shared = 0, n_turns = 0, n_left = 0;
    static const int GMAX[] = {1, 3, 4, 16};
    for (g_seq = 0; g_seq < 200; g_seq++) {
        std::mt19937 rng(20240000u + (unsigned)g_seq);
        auto pick = [&](int n) { return (int)(rng() % (unsigned)n); };
        const int gmax = GMAX[g_seq % 4];
        Queue q;
        std::vector<std::unique_ptr<Job>> jobs; // every job of the sequence: tasks of a finished one may still wait
        std::vector<Job*> pool(6, nullptr);     // the ones still pushing
        std::vector<Shadow> live, low;
        int hold = 0, dry = 0, taken = 0; int64_t epoch = 0, next_id = 1, next_serial = 1; // taken: chunks and fences out, completion not popped
        for (g_op = 0; g_op < 300; g_op++, n_ops++) {
            const int what = pick(100);
            if (what < 50) { // a request's next push
                Job*& j = pool[pick((int)pool.size())];
                if (!j || j->pushed == 2) { jobs.emplace_back(new Job{next_id++, pick(3) == 0}); j = jobs.back().get(); }
                std::vector<Shadow>& s = j->decode ? low : live;
                if (j->pushed == 0) { q.push(j, TASK_RESET); s.push_back({j, TASK_RESET, 0, 0, 0}); j->pushed = 1; }
                else if (pick(5) == 0) { q.push(j, TASK_FENCE); s.push_back({j, TASK_FENCE, 0, 0, 0}); j->pushed = 2; }
                else {
                    const int frames = pick(4) == 0 ? 1 + pick(3) : 4; // a tail now and then
                    std::vector<int64_t> codes((size_t)16 * frames, 0);
                    codes[0] = next_serial;
                    q.push(j, TASK_CHUNK, codes.data(), (int)codes.size(), frames < 4);
                    s.push_back({j, TASK_CHUNK, next_serial++, frames, j->decode ? 0 : epoch});
                    if (q.live.empty() && q.low.empty()) FAIL("a push left both queues empty");
                    if ((j->decode ? q.low : q.live).back().is_final != (frames < 4)) FAIL("is_final lost");
                }
                n_pushes++;
            } else if (what < 54) { // a hand-over opens; one inside another belongs to it
                if (hold < 2) { q.open(); if (hold++ == 0) { epoch++; n_handovers++; } else n_nested++; }
            } else if (what < 64) {
                if (hold > 0) { q.close(); hold--; }
            } else if (what < 68) { // a request purged: its chunks nobody has taken, nothing else
                if (!jobs.empty()) {
                    Job* j = jobs[pick((int)jobs.size())].get();
                    std::vector<Shadow>& s = j->decode ? low : live;
                    const size_t before = s.size();
                    s.erase(std::remove_if(s.begin(), s.end(), [&](const Shadow& t) { return t.job == j && t.kind == TASK_CHUNK; }), s.end());
                    q.purge(j);
                    n_purges++; n_purged += (long)(before - s.size());
                }
            } else if (what < 90) { // a step taken
                const std::vector<Queue::Task> step = q.take(gmax);
                n_takes++;
                if (hold > 0) {
                    if (!step.empty()) FAIL("a step was taken while a hand-over was open");
                    n_held_takes++;
                } else {
                    // the call restated: the heads of both queues as they stand, the width, the count carried over
                    const bool turn_due = !live.empty() && dry >= SEAT_DRY_MAX;
                    const Seating want = seat_chunks(heads(live), heads(low), gmax, dry);
                    dry = want.dry;
                    if (q.dry != dry) FAIL("dry is %d, seat_chunks answered %d", q.dry, dry);
                    if (step.size() != want.seats.size()) FAIL("%zu tasks taken, %zu seated", step.size(), want.seats.size());
                    if (step.empty() != (live.empty() && low.empty())) FAIL("an empty step from queues that are not");
                    int64_t ep = -1; int n_low = 0;
                    for (size_t i = 0; i < step.size(); i++) {
                        const Shadow& w = (want.seats[i].low ? low : live)[want.seats[i].index];
                        const Queue::Task& t = step[i];
                        if (t.job != w.job || t.kind != w.kind || (int)t.codes.size() != 16 * w.frames || (t.kind == TASK_CHUNK && t.codes[0] != w.serial))
                            FAIL("task %zu of the step is not the seated one", i);
                        if (t.kind != TASK_CHUNK && step.size() != 1) FAIL("a reset or fence shares a step");
                        Job* j = t.job;
                        // a request's tasks leave as reset, chunks in the order pushed, fence
                        if (t.kind == TASK_RESET) { if (j->left != 0) FAIL("a reset left late"); j->left = 1; }
                        else if (t.kind == TASK_FENCE) { if (j->left != 1) FAIL("a fence left out of order"); j->left = 2; }
                        else {
                            if (j->left != 1 || t.codes[0] <= j->last_serial) FAIL("a chunk left out of order");
                            j->last_serial = t.codes[0];
                            if (!j->decode) { if (ep >= 0 && t.epoch != ep) FAIL("generating chunks of two epochs in one step"); ep = t.epoch; }
                            n_low += j->decode;
                        }
                        if (t.kind != TASK_RESET) taken++;
                        n_left++;
                    }
                    if (!step.empty()) {
                        n_steps++;
                        if (step.size() > 1) n_multi++;
                        if (n_low > 0 && n_low < (int)step.size()) n_shared++;
                        if (turn_due && step[0].kind == TASK_CHUNK && step[0].job->decode) n_turns++; // it led while generating tasks waited
                    }
                    for (int lo = 0; lo < 2; lo++) { // out of the shadow, last first
                        std::vector<int> idx;
                        for (const Seat& c : want.seats) if ((int)c.low == lo) idx.push_back(c.index);
                        std::sort(idx.rbegin(), idx.rend());
                        for (int i : idx) (lo ? low : live).erase((lo ? low : live).begin() + i);
                    }
                }
            } else { // a completion popped
                if (taken > 0) { q.popped(); taken--; n_pops++; }
            }
            // after every operation: the queues are the shadow's, and pending counts the chunks and fences queued or out
            same(q.live, live, "live"); same(q.low, low, "low");
            int want_pending = taken;
            for (const Shadow& t : live) want_pending += t.kind != TASK_RESET;
            for (const Shadow& t : low) want_pending += t.kind != TASK_RESET;
            if (q.pending != want_pending) FAIL("pending is %d, %d chunks and fences are queued or out", q.pending, want_pending);
            if (q.hold != hold || q.epoch != epoch) FAIL("hold %d epoch %lld, expected %d and %lld", q.hold, (long long)q.epoch, hold, (long long)epoch);
            if (q.ready() != (hold == 0 && !(live.empty() && low.empty()))) FAIL("ready() disagrees");
        }
    }
    std::printf("sequences %d\nops %ld\npushes %ld\ntakes %ld\nheld_takes %ld\nsteps %ld\ntasks_left %ld\npurges %ld\nchunks_purged %ld\npops %ld\n", g_seq, n_ops,
                n_pushes, n_takes, n_held_takes, n_steps, n_left, n_purges, n_purged, n_pops);
    std::printf("handovers %ld\nnested %ld\nmulti_seat %ld\nshared %ld\ndecode_turns %ld\n", n_handovers, n_nested, n_multi, n_shared, n_turns);
    return 0;
}
