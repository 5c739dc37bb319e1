"""[EXT] decoding given frames, CPU half (include/q3tts_spec.h "decoding given frames"): the entry points are declared, exported, listed and
fail cleanly without an engine or a device; every refusal of q3tts_submit_decode is reached through the pure rule of csrc/sched_logic.h;
the seat rule of the decoder thread -- which chunks of the two queues share a codec pass -- is checked case by case and, with the low queue
empty, against the grouping loop the thread ran before decode-only requests existed; the admission arithmetic is checked over the engine
sizes in use.  The rules are built with plain g++ and the host sanitizers, like the other rule drivers.  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_submit_decode", "q3tts_group_submit_decode", "q3tts_engine_decode_width", "q3tts_engine_decode_stats")
SAMPLE_END, CODEC_EOS = 2160, 2150   # Q3_SAMPLE_END, Q3_CODEC_EOS


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_names_are_declared_exported_and_listed(q3):
    txt = _header("q3tts.h")
    tail = r"\s*const\s+int32_t\s*\*\s*codes\s*,\s*int32_t\s+n\s*,\s*int64_t\s*\*\s*req_id\s*\)\s*;"
    assert re.search(r"\bint\s+q3tts_submit_decode\s*\(\s*q3tts_engine\s*\*\s*\w+\s*," + tail, txt)
    assert re.search(r"\bint\s+q3tts_group_submit_decode\s*\(\s*q3tts_group\s*\*\s*\w+\s*,\s*int32_t\s+engine_index\s*," + tail, txt)
    assert re.search(r"\bint32_t\s+q3tts_engine_decode_width\s*\(\s*q3tts_engine\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_engine_decode_stats\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*requests\s*,"
                     r"\s*int64_t\s*\*\s*chunks\s*,\s*int64_t\s*\*\s*chunks_shared\s*\)\s*;", txt)
    for n in NEW:
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n) and getattr(q3.lib(), n).argtypes, n
    raw = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    doc = raw[raw.index("[EXT] decode given frames"):raw.index("int q3tts_submit_decode")]
    assert "no talker slot" in doc and "Refused" in doc and "load_codec = 0" in doc and "Q3TTS_REQ_DRAINING" in doc
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    sec = spec[spec.index("decoding given frames [EXT]"):]
    assert "D1" in sec and "D2" in sec and "D3" in sec and "decode_width" in sec and "Q3_CHUNK_CODES" in sec


def test_python_surface(q3):
    assert callable(q3.Engine.submit_decode) and callable(q3.Engine.decode_width) and callable(q3.Engine.decode_stats)
    assert callable(q3.group_submit_decode)


def test_entry_points_fail_cleanly_without_an_engine_or_a_device(q3):
    L = q3.lib()
    codes, rid = np.full((4, 16), 7, np.int32), C.c_int64(-5)
    assert L.q3tts_submit_decode(None, q3._p(codes), 4, C.byref(rid)) < 0 and L.q3tts_last_error() and rid.value == -5
    assert L.q3tts_group_submit_decode(None, -1, q3._p(codes), 4, C.byref(rid)) < 0 and L.q3tts_last_error() and rid.value == -5
    assert L.q3tts_engine_decode_width(None) < 0
    a = C.c_int64(-7)
    assert L.q3tts_engine_decode_stats(None, C.byref(a), None, None) < 0 and L.q3tts_last_error() and a.value == -7
    with pytest.raises(q3.Q3Error):
        q3.group_submit_decode(None, -1, codes)
    if q3.device_count() == 0:   # there is no engine to decode on without a device, and no other path to PCM
        with pytest.raises(q3.Q3Error, match="no HIP device"):
            q3.Engine(os.path.join(ROOT, "no_such_model"), "q8_0", max_batch=1, max_steps=8)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("decode_logic") / "decode_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "decode_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _refusal(driver, n=6, max_steps=16, have_codec=1, null_codes=0, at=-1, c0=5, res=7):
    return driver("refusal %d %d %d %d %d %d %d\n" % (n, max_steps, have_codec, null_codes, at, c0, res))[0]


def test_every_refusal_and_the_accepting_edges(driver):
    assert _refusal(driver) == "ok"
    assert _refusal(driver, n=1) == "ok"                                  # a tail alone
    assert _refusal(driver, n=16) == "ok"                                 # exactly max_steps: the staging region is full, not over
    assert "max_steps" in _refusal(driver, n=17)
    assert "n must be >= 1" in _refusal(driver, n=0)
    assert "n must be >= 1" in _refusal(driver, n=-3)
    assert "load_codec" in _refusal(driver, have_codec=0)
    assert "load_codec" in _refusal(driver, have_codec=0, n=0)            # whatever else is wrong, there is no codec
    assert "codes missing" in _refusal(driver, null_codes=1)
    for at in (0, 3, 5):                                                  # the first frame, one inside, the last
        for c0 in (0, 2047, 2048, SAMPLE_END - 1, CODEC_EOS - 1, CODEC_EOS + 1):   # codes past the codebook are clamped by the chunker, as emitted ones
            assert _refusal(driver, at=at, c0=c0) == "ok", (at, c0)
        assert "EOS" in _refusal(driver, at=at, c0=CODEC_EOS)
        assert "code_0" in _refusal(driver, at=at, c0=SAMPLE_END)
        assert "code_0" in _refusal(driver, at=at, c0=-1)
        assert "residual" in _refusal(driver, at=at, res=2048)
        assert "residual" in _refusal(driver, at=at, res=-1)
        assert _refusal(driver, at=at, res=2047) == "ok" and _refusal(driver, at=at, res=0) == "ok"
    assert "code_0" in _refusal(driver, n=1, at=0, c0=SAMPLE_END) and "EOS" in _refusal(driver, n=16, at=15, c0=CODEC_EOS)


def test_decode_width_and_admission(driver):
    """n_cs = max_batch + min(max_batch, 16) streams (Engine::Engine); half of the surplus, at least one"""
    for b, want in ((1, 1), (4, 2), (64, 8), (256, 8)):
        assert int(driver("width %d %d\n" % (b + min(b, 16), b))[0]) == want
    assert int(driver("width 2 2\n")[0]) == 1 and int(driver("width 5 2\n")[0]) == 1 and int(driver("width 6 2\n")[0]) == 2

    def admit(q, f, h, w):
        return int(driver("admit %d %d %d %d\n" % (q, f, h, w))[0])
    assert admit(5, 8, 0, 2) == 2        # the width limits
    assert admit(5, 1, 0, 2) == 1        # a free stream limits
    assert admit(1, 8, 0, 2) == 1        # the queue limits
    assert admit(5, 8, 2, 2) == 0        # width holders already
    assert admit(5, 8, 1, 2) == 1
    assert admit(5, 0, 0, 2) == 0        # the generating wave took every stream
    assert admit(0, 8, 0, 2) == 0


def _q(tasks):
    return "\n".join("%d %d %s" % t for t in tasks)


def _seat(driver, gmax, dry, live, low):
    line = driver("seat %d %d %d %d\n%s\n%s\n" % (gmax, dry, len(live), len(low), _q(live), _q(low)))[0]
    seats, dry = line.split("|")
    return seats.split(), int(dry)


def _drain(driver, gmax, live, low):
    out = driver("drain %d %d %d\n%s\n%s\n" % (gmax, len(live), len(low), _q(live), _q(low)))
    assert out[-1] == "end"
    return [ln.split("|")[0].split() for ln in out[:-1]]


def _old_passes(queue, gmax):
    """the decoder thread's loop before the low queue: the oldest task; if it is a chunk, the first pending task of every other request joins
    when it is a chunk of the same frame count, up to gmax"""
    q, out = list(queue), []
    while q:
        grp = [q.pop(0)]
        if grp[0][2] == "C" and gmax > 1:
            seen, i = [grp[0][0]], 0
            while i < len(q) and len(grp) < gmax:
                dup = q[i][0] in seen
                if not dup:
                    seen.append(q[i][0])
                if not dup and q[i][2] == "C" and q[i][1] == grp[0][1]:
                    grp.append(q.pop(i))
                else:
                    i += 1
        out.append(["L%d/%d%s" % t for t in grp])
    return out


def _recorded_queue(rng, n_req):
    """a live queue as the scheduler fills it: every request a reset, its chunks (4 frames, a shorter tail), a fence, interleaved in arrival order"""
    per = []
    for r in range(n_req):
        n = int(rng.integers(1, 14))
        per.append([(r, 0, "R")] + [(r, 4, "C")] * (n // 4) + ([(r, n % 4, "C")] if n % 4 else []) + [(r, 0, "F")])
    q = []
    while any(per):
        r = int(rng.integers(0, n_req))
        if per[r]:
            q.append(per[r].pop(0))
    return q


def test_an_empty_low_queue_gives_the_passes_of_before(driver):
    rng = np.random.default_rng(11)
    for case in range(40):
        q, gmax = _recorded_queue(rng, int(rng.integers(1, 7))), int(rng.choice([1, 2, 4, 16]))
        assert _drain(driver, gmax, q, []) == _old_passes(q, gmax), case


def test_free_seats_are_filled_in_queue_order_one_chunk_per_request(driver):
    live = [(1, 4, "C"), (2, 4, "C"), (1, 4, "C")]
    low = [(10, 4, "C"), (10, 4, "C"), (11, 4, "C"), (12, 4, "C"), (13, 4, "C")]
    seats, dry = _seat(driver, 4, 0, live, low)
    assert seats == ["L1/4C", "L2/4C", "D10/4C", "D11/4C"] and dry == 0   # the second chunks of 1 and 10 wait; 12 and 13 find no seat
    seats, dry = _seat(driver, 16, 0, live, low)
    assert seats == ["L1/4C", "L2/4C", "D10/4C", "D11/4C", "D12/4C", "D13/4C"]
    # the live chunks fill the pass: nothing of the low queue is seated, and the pass counts as one that left a decode-only chunk waiting
    seats, dry = _seat(driver, 2, 0, live, low)
    assert seats == ["L1/4C", "L2/4C"] and dry == 1
    seats, dry = _seat(driver, 2, 3, live, low)
    assert dry == 4


def test_a_differing_frame_count_is_not_seated(driver):
    live = [(1, 4, "C"), (2, 3, "C")]
    low = [(10, 3, "C"), (11, 4, "C"), (12, 1, "C")]
    seats, dry = _seat(driver, 8, 0, live, low)
    assert seats == ["L1/4C", "D11/4C"] and dry == 0                      # the 3-frame tails of 2 and 10, the 1-frame tail of 12 wait
    seats, dry = _seat(driver, 8, 0, [(2, 3, "C")], [(10, 3, "C"), (12, 1, "C")])
    assert seats == ["L2/3C", "D10/3C"]
    # only a request's first pending task counts: the 4-frame chunk behind 10's 3-frame one is not taken out of order
    seats, dry = _seat(driver, 8, 0, [(1, 4, "C")], [(10, 3, "C"), (10, 4, "C")])
    assert seats == ["L1/4C"] and dry == 1


def test_resets_and_fences_run_alone(driver):
    # of a generating request, at the head of the live queue, as before
    assert _seat(driver, 8, 0, [(1, 0, "R"), (2, 4, "C")], [])[0] == ["L1/0R"]
    assert _seat(driver, 8, 0, [(1, 0, "F"), (2, 4, "C")], [])[0] == ["L1/0F"]
    # of a decode-only request, as soon as it heads the request's tasks: at once, alone, the count of dry passes untouched
    seats, dry = _seat(driver, 8, 2, [(1, 4, "C")], [(10, 4, "C"), (11, 0, "R"), (11, 4, "C")])
    assert seats == ["D11/0R"] and dry == 2
    assert _seat(driver, 8, 0, [(1, 4, "C")], [(10, 4, "C"), (10, 0, "F"), (11, 0, "F")])[0] == ["D11/0F"]
    assert _seat(driver, 8, 0, [(1, 4, "C")], [(10, 4, "C"), (10, 0, "F")])[0] == ["L1/4C", "D10/4C"]   # 10's fence stays behind its chunk
    # a request's order holds through a whole drain: reset, chunks, fence
    passes = _drain(driver, 4, [(1, 0, "R"), (1, 4, "C"), (1, 2, "C"), (1, 0, "F")], [(10, 0, "R"), (10, 4, "C"), (10, 4, "C"), (10, 2, "C"), (10, 0, "F")])
    assert passes == [["D10/0R"], ["L1/0R"], ["L1/4C", "D10/4C"], ["L1/2C"], ["L1/0F"], ["D10/4C"], ["D10/2C"], ["D10/0F"]]


def test_a_waiting_decode_chunk_leads_the_fifth_pass(driver):
    gmax = 4
    live = [(r, 4, "C") for _ in range(12) for r in (1, 2, 3, 4)]          # gmax generating requests, a chunk each in every pass
    low = [(10, 4, "C"), (10, 4, "C"), (11, 4, "C")]
    passes = _drain(driver, gmax, live, low)
    full = ["L1/4C", "L2/4C", "L3/4C", "L4/4C"]
    assert passes[:4] == [full] * 4
    assert passes[4] == ["D10/4C", "L1/4C", "L2/4C", "L3/4C"]             # led by the oldest decode-only chunk; generating chunks take the other seats
    assert passes[5][0] == "L4/4C" and not any(s.startswith("D") for s in passes[5])   # the count starts again
    nxt = [i for i, p in enumerate(passes) if p[0].startswith("D")]
    assert nxt[1] - nxt[0] == 5                                           # and the next turn comes after four more dry passes
    # no chunk is lost or doubled
    flat = sorted(s for p in passes for s in p)
    assert flat == sorted(["L%d/4C" % t[0] for t in live] + ["D%d/4C" % t[0] for t in low])
    # a decode-only tail of another frame count waits the same way and then leads a pass of its own
    seats, dry = _seat(driver, gmax, 4, live, [(10, 2, "C")])
    assert seats == ["D10/2C"] and dry == 0
    # below the limit it waits
    seats, dry = _seat(driver, gmax, 3, live, [(10, 2, "C")])
    assert seats == full and dry == 4


def test_only_decode_chunks_form_groups_of_gmax(driver):
    low = [(r, 4, "C") for r in range(10, 16)] + [(r, 4, "C") for r in range(10, 16)] + [(r, 1, "C") for r in (10, 12)]
    passes = _drain(driver, 4, [], low)
    assert passes == [["D10/4C", "D11/4C", "D12/4C", "D13/4C"], ["D14/4C", "D15/4C", "D10/4C", "D11/4C"], ["D12/4C", "D13/4C", "D14/4C", "D15/4C"],
                      ["D10/1C", "D12/1C"]]


def test_gmax_one(driver):
    live = [(1, 4, "C"), (2, 4, "C")] * 3
    passes = _drain(driver, 1, live, [(10, 4, "C"), (10, 0, "F")])
    assert all(len(p) == 1 for p in passes)
    assert passes[:5] == [["L1/4C"], ["L2/4C"], ["L1/4C"], ["L2/4C"], ["D10/4C"]]   # its turn after four passes without a seat
    assert passes[5] == ["D10/0F"]                                        # the fence heads the request's tasks now
    assert passes[6:] == [["L1/4C"], ["L2/4C"]]


def _drain_e(driver, gmax, live, low):
    q = lambda tasks: "\n".join(" ".join(str(x) for x in t) for t in tasks)
    out = driver("epochs 1\ndrain %d %d %d\n%s\n%s\n" % (gmax, len(live), len(low), q(live), q(low)))
    assert out[-1] == "end"
    return [ln.split("|")[0].split() for ln in out[:-1]]


def test_a_pass_holds_the_generating_chunks_of_one_hand_over(driver):
    """the thread's passes are the same whether it forms them before or after the next hand-over has arrived: three requests hand over a
    chunk each in epochs 1 and 2, gmax 2.  Seen one hand-over at a time the passes are {1, 2}, {3}, {1', 2'}, {3'}; with both in the queue
    at once request 1's second chunk does not take the seat beside request 3's first"""
    e1, e2 = [(r, 4, "C", 1) for r in (1, 2, 3)], [(r, 4, "C", 2) for r in (1, 2, 3)]
    apart = _drain_e(driver, 2, e1, []) + _drain_e(driver, 2, e2, [])
    assert apart == [["L1/4C", "L2/4C"], ["L3/4C"]] * 2
    assert _drain_e(driver, 2, e1 + e2, []) == apart
    assert _drain(driver, 2, [t[:3] for t in e1 + e2], []) == [["L1/4C", "L2/4C"], ["L3/4C", "L1/4C"], ["L2/4C", "L3/4C"]]   # one epoch: seats by age alone
    # tails of another frame count and fences keep their places; the 1-frame tails of one hand-over share a pass
    live = [(1, 4, "C", 1), (2, 1, "C", 1), (2, 0, "F", 1), (3, 1, "C", 1), (3, 0, "F", 1), (1, 4, "C", 2), (4, 1, "C", 2)]
    assert _drain_e(driver, 4, live, []) == [["L1/4C"], ["L2/1C", "L3/1C"], ["L2/0F"], ["L3/0F"], ["L1/4C"], ["L4/1C"]]
    # decode-only chunks carry no epoch: they take the seats left; a decode-only lead binds the pass to the first generating chunk's epoch
    assert _drain_e(driver, 4, e1[:1] + e2[1:2], [(10, 4, "C", 0), (11, 4, "C", 0)]) == [["L1/4C", "D10/4C", "D11/4C"], ["L2/4C"]]
    out = driver("epochs 1\nseat 4 4 3 1\n1 4 C 1\n2 4 C 2\n3 4 C 1\n10 4 C 0\n")[0]
    assert out.split("|")[0].split() == ["D10/4C", "L1/4C", "L3/4C"]
