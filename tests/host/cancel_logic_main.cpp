// Driver of tests/test_cancel_cpu.py: the cancellation rules of csrc/sched_logic.h alone, plain g++.  Reads commands on stdin, prints one
// result line per answer.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <string>

using namespace q3;

static const char* name(CancelAction a) {
    switch (a) {
    case CANCEL_NOTHING: return "nothing";
    case CANCEL_AT_ONCE: return "at_once";
    case CANCEL_AT_ACTIVATE: return "at_activate";
    case CANCEL_RETIRE: return "retire";
    case CANCEL_RETIRE_FENCE: return "retire_fence";
    case CANCEL_PURGE: return "purge";
    }
    return "?";
}

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "states") { // the values the C ABI promises
            printf("%d %d %d %d %d %d\n", REQ_QUEUED, REQ_RUNNING, REQ_DRAINING, REQ_DONE, REQ_CANCELLED, REQ_FAILED);
        } else if (cmd == "action") { // action state in_wave live want_pcm
            int state, in_wave, live, want_pcm;
            std::cin >> state >> in_wave >> live >> want_pcm;
            printf("%s\n", name(cancel_action(state, in_wave != 0, live != 0, want_pcm != 0)));
        } else if (cmd == "ended") { // ended state
            int state; std::cin >> state;
            printf("%d\n", req_ended(state) ? 1 : 0);
        } else if (cmd == "retired") { // retired want_pcm cancelled -> state after the slot is given back
            int want_pcm, cancelled; std::cin >> want_pcm >> cancelled;
            printf("%d\n", retired_state(want_pcm != 0, cancelled != 0));
        } else if (cmd == "fenced") { // fenced cancelled -> state after the fence
            int cancelled; std::cin >> cancelled;
            printf("%d\n", fenced_state(cancelled != 0));
        } else {
            fprintf(stderr, "unknown command %s\n", cmd.c_str());
            return 2;
        }
    }
    return 0;
}
