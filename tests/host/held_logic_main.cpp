// Driver of tests/test_held_cpu.py: the table codec preambles and prompt stems live in (HeldTable, csrc/sched_logic.h) alone, plain g++.  Reads
// commands on stdin, prints one result line per answer.  The table under test is a HeldTable<int> with three voice settings beside it;
// "new <noun>" starts a fresh one.  An operation answers "recycled <payload>" when it handed a payload back, "kept" when it did not, and
// "throw <message>" when it threw.
#include "../../qwen3-tts-rust_amd/csrc/sched_logic.h"
#include <cstdio>
#include <iostream>
#include <memory>
#include <random>
#include <string>

using namespace q3;

namespace {
typedef HeldTable<int> Table;
const int kVoices = 3;

void answer(const Table::Recycled& r) { if (r) printf("recycled %d\n", *r); else printf("kept\n"); }

// The seeded walk.  The model knows, per id ever handed out, its creator flag, its state and its open request holds, and beside them the voice
// settings and the engine-level one.  After every operation each entry's holder count is recomputed from scratch (voices set to it + the engine
// setting + open request holds), an id must be live in the table exactly while creator || holders > 0 || BUILDING held ever since it was added,
// and the payload an operation hands back must be that of the one id that died in it.  Returns an empty string, or what went wrong.
struct Model { bool live = true, creator = true; int state = HELD_BUILDING, req_holds = 0, handed_back = 0; };
std::string walk(const char* noun, unsigned seed, int steps, long long* n_recycled) {
    Table t(noun);
    const HeldWords words(noun);
    std::vector<Model> m; int voices[kVoices] = {-1, -1, -1};
    std::vector<int> open_holds; // one entry per open request hold: its id
    std::mt19937 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    auto n_live = [&] { int n = 0; for (const Model& x : m) n += x.live; return n; };
    auto any_id = [&] { // three times in four a live id, else any id ever handed out: most of those are long gone
        std::vector<int> live;
        for (int id = 0; id < (int)m.size(); id++) if (m[(size_t)id].live) live.push_back(id);
        if (!live.empty() && rnd(0, 3) != 0) return live[(size_t)rnd(0, (int)live.size() - 1)];
        return m.empty() ? 0 : rnd(0, (int)m.size() - 1);
    };
    auto holders = [&](int id) {
        int h = (t.setting == id) + m[(size_t)id].req_holds;
        for (int v : voices) h += v == id;
        return h;
    };
    for (int k = 0; k < steps; k++) {
        const std::string at = "step " + std::to_string(k) + ": ";
        Table::Recycled got; std::string thrown, want_throw;
        const int op = rnd(0, 7);
        try {
            if (op == 0) {
                if (n_live() >= 8) continue;
                const int id = t.add(k);
                if (id != (int)m.size()) return at + "add handed out id " + std::to_string(id) + ", not the next one";
                t.at(id).payload = 1000 + id;
                m.emplace_back();
            } else if (op == 1) { // a build ends
                const int id = any_id();
                if (m.empty() || !m[(size_t)id].live || m[(size_t)id].state != HELD_BUILDING) continue;
                const bool ok = rnd(0, 3) != 0;
                m[(size_t)id].state = ok ? HELD_READY : HELD_FAILED;
                got = t.finish(id, ok);
            } else if (op == 2) { // the creator's release, of anything
                const int id = any_id();
                if (m.empty() || !m[(size_t)id].live) want_throw = words.unknown;
                else if (!m[(size_t)id].creator) want_throw = words.released;
                else m[(size_t)id].creator = false;
                got = t.release_creator(id);
            } else if (op == 3 || op == 4) { // a setter: none, anything ever handed out, an id never handed out, a bad negative
                const int pick = rnd(0, 9), id = pick == 0 ? -1 : pick == 1 ? -7 : pick == 2 ? (int)m.size() + 3 : any_id();
                if (id >= 0 && (id >= (int)m.size() || !m[(size_t)id].live)) want_throw = words.unknown;
                else if (id >= 0 && m[(size_t)id].state == HELD_BUILDING) want_throw = words.building;
                else if (id >= 0 && m[(size_t)id].state == HELD_FAILED) want_throw = words.failed;
                else if (id < -1) want_throw = words.bad_id;
                int before[kVoices + 1] = {voices[0], voices[1], voices[2], t.setting};
                int& which = op == 3 ? voices[rnd(0, kVoices - 1)] : t.setting;
                try { got = t.swap_setting(which, id); }
                catch (...) {
                    if (before[0] != voices[0] || before[1] != voices[1] || before[2] != voices[2] || before[3] != t.setting) return at + "a refused setter changed a setting";
                    throw;
                }
                if (which != id) return at + "the setter did not store the id";
            } else if (op == 5) { // a request takes one
                const int id = any_id();
                if (m.empty() || !m[(size_t)id].live) continue;
                t.hold(id); m[(size_t)id].req_holds++; open_holds.push_back(id);
            } else if (op == 6) { // a request ends
                if (open_holds.empty()) continue;
                const size_t i = (size_t)rnd(0, (int)open_holds.size() - 1);
                const int id = open_holds[i];
                open_holds.erase(open_holds.begin() + (long)i);
                m[(size_t)id].req_holds--;
                got = t.unhold(id);
            } else { // an unhold of what is long gone, or was never there
                const int id = any_id();
                if (!m.empty() && m[(size_t)id].live) continue;
                got = t.unhold(m.empty() ? 5 : id);
            }
        } catch (const std::exception& ex) { thrown = ex.what(); }
        if (thrown != want_throw) return at + "threw \"" + thrown + "\" where \"" + want_throw + "\" was due";
        // every entry against the model, holders recomputed from scratch
        int died = -1;
        for (int id = 0; id < (int)m.size(); id++) {
            Model& x = m[(size_t)id];
            const int h = holders(id);
            const bool live = x.live && (x.creator || h > 0 || x.state == HELD_BUILDING);
            if (x.live && !live) { if (died >= 0) return at + "two ids died in one operation"; died = id; }
            x.live = live;
            Table::Entry* e = t.find(id);
            if ((e != nullptr) != live) return at + "id " + std::to_string(id) + (live ? " is missing from the table" : " is still in the table");
            if (e && (e->refs.creator != x.creator || e->refs.holders != h || e->refs.state != x.state || e->payload != 1000 + id))
                return at + "id " + std::to_string(id) + " holds creator " + std::to_string(e->refs.creator) + " holders " + std::to_string(e->refs.holders) +
                       " state " + std::to_string(e->refs.state) + ", the model creator " + std::to_string(x.creator) + " holders " + std::to_string(h) +
                       " state " + std::to_string(x.state);
        }
        if (t.live() != n_live()) return at + "the table's size differs from the model's";
        if (got.has_value() != (died >= 0)) return at + (got ? "a payload came back though no id died" : "an id died and no payload came back");
        if (got) {
            if (*got != 1000 + died) return at + "the payload of another id came back";
            if (++m[(size_t)died].handed_back != 1) return at + "a payload came back twice";
            (*n_recycled)++;
        }
    }
    for (const Model& x : m) if (x.handed_back != (x.live ? 0 : 1)) return "at the end: a payload was not handed back exactly once";
    return "";
}
}

int main() {
    std::unique_ptr<Table> t; int voices[kVoices] = {-1, -1, -1};
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "new") { // new noun
            std::string noun;
            std::cin >> noun;
            t.reset(new Table(noun.c_str()));
            for (int& v : voices) v = -1;
            printf("ok\n");
        } else if (cmd == "walk") { // walk noun seed steps -> "ok <payloads handed back>" or "seed <seed> <what went wrong>"
            std::string noun; unsigned seed; int steps; long long n = 0;
            std::cin >> noun >> seed >> steps;
            const std::string bad = walk(noun.c_str(), seed, steps, &n);
            if (bad.empty()) printf("ok %lld\n", n); else printf("seed %u %s\n", seed, bad.c_str());
        } else if (!t) {
            fprintf(stderr, "%s before new\n", cmd.c_str());
            return 2;
        } else if (cmd == "show") { // -> "engine <setting> voices <a> <b> <c> live <count> :" then " <id>=<creator>/<holders>/<state>/<n>/<payload>" per entry
            printf("engine %d voices %d %d %d live %d :", t->setting, voices[0], voices[1], voices[2], t->live());
            for (const auto& kv : t->entries())
                printf(" %d=%d/%d/%d/%d/%d", kv.first, kv.second.refs.creator ? 1 : 0, kv.second.refs.holders, kv.second.refs.state, kv.second.n, kv.second.payload);
            printf("\n");
        } else try {
            int id = 0, x = 0;
            if (cmd == "add") { // add n payload -> the id
                std::cin >> id >> x;
                const int got = t->add(id);
                t->at(got).payload = x;
                printf("%d\n", got);
            } else if (cmd == "at") { std::cin >> id; printf("%d\n", t->at(id).n); } // at id -> its n
            else if (cmd == "find") { std::cin >> id; printf("%d\n", t->find(id) ? 1 : 0); }
            else if (cmd == "hold") { std::cin >> id; t->hold(id); printf("ok\n"); }
            else if (cmd == "unhold") { std::cin >> id; answer(t->unhold(id)); }
            else if (cmd == "release") { std::cin >> id; answer(t->release_creator(id)); }
            else if (cmd == "finish") { std::cin >> id >> x; answer(t->finish(id, x != 0)); } // finish id ok
            else if (cmd == "voice") { std::cin >> x >> id; answer(t->swap_setting(voices[x], id)); } // voice v id
            else if (cmd == "engine") { std::cin >> id; answer(t->swap_setting(t->setting, id)); }
            else if (cmd == "refusal") { std::cin >> id; const char* why = t->set_refusal(id); printf("%s\n", why ? why : "ok"); }
            else {
                fprintf(stderr, "unknown command %s\n", cmd.c_str());
                return 2;
            }
        } catch (const std::exception& ex) { printf("throw %s\n", ex.what()); }
    }
    return 0;
}
