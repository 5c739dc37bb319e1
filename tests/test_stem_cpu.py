"""[EXT] prompt stems, CPU half (include/q3tts_spec.h "prompt stems"): the entry points are declared, exported, listed and fail cleanly without an
engine or a device; every refusal of q3tts_stem_create, what a setter refuses, which stem applies, the take rule, the prefill packer with
skipped rows, the admission row counts and the holder table are reached through the pure rules of csrc/sched_logic.h, built with plain g++
and the host sanitizers like the other rule drivers.  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("q3tts_stem_create", "q3tts_voice_stem_create", "q3tts_stem_poll", "q3tts_stem_wait", "q3tts_stem_release", "q3tts_voice_set_stem",
          "q3tts_engine_set_stem", "q3tts_request_stem", "q3tts_engine_stem_stats")
GROUP = ("q3tts_group_stem_create", "q3tts_group_voice_stem_create", "q3tts_group_stem_wait", "q3tts_group_stem_release",
         "q3tts_group_voice_set_stem", "q3tts_group_set_stem", "q3tts_group_request_stem", "q3tts_group_stem_stats")
BUILDING, READY, FAILED = 0, 1, -1


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_names_are_declared_exported_and_listed(q3):
    txt = _header("q3tts.h")
    for n in ENGINE + GROUP + ("q3tts_op_kv_stem",):
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n) and getattr(q3.lib(), n).argtypes, n
    assert re.search(r"\bint\s+q3tts_stem_create\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*const\s+float\s*\*\s*rows\s*,\s*int32_t\s+n_rows\s*,"
                     r"\s*int32_t\s*\*\s*stem_id\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_request_stem\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*int64_t\s+req_id\s*,\s*int32_t\s*\*\s*stem_id\s*,"
                     r"\s*int32_t\s*\*\s*rows_reused\s*\)\s*;", txt)
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    sec = spec[spec.index("prompt stems [EXT]"):]
    for word in ("takes", "memcmp", "n_prompt > n", "S1", "S2", "READY", "mismatch"):
        assert word in sec, word
    stripped = _header("q3tts_spec.h")
    assert re.search(r"#define\s+Q3TTS_MAX_STEMS\s+64\b", stripped)
    for name, val in (("BUILDING", "0"), ("READY", "1"), ("FAILED", "-1")):
        assert re.search(r"#define\s+Q3TTS_STEM_%s\s+%s\b" % (name, re.escape(val)), stripped), name
    assert (q3.MAX_STEMS, q3.STEM_BUILDING, q3.STEM_READY, q3.STEM_FAILED) == (64, BUILDING, READY, FAILED)
    assert [f for f, _ in q3.StemStats._fields_] == ["built", "restores", "rows_not_prefilled", "pages_copied", "mismatches", "device_bytes"]
    m = re.search(r"typedef\s+struct\s+q3tts_stem_stats\s*\{([^}]*)\}", txt)
    assert m and [w.strip() for w in m.group(1).replace("int64_t", "").strip(" ;").split(",")] == [f for f, _ in q3.StemStats._fields_]


def test_python_surface(q3):
    for n in ("stem_create", "voice_stem_create", "stem_poll", "stem_wait", "stem_release", "voice_set_stem", "set_stem", "request_stem",
              "stem_stats", "stem_voice"):
        assert callable(getattr(q3.Engine, n)), n
    for n in ("group_stem_create", "group_voice_stem_create", "group_stem_wait", "group_stem_release", "group_voice_set_stem", "group_set_stem",
              "group_request_stem", "group_stem_stats", "op_kv_stem"):
        assert callable(getattr(q3, n)), n


def test_entry_points_fail_cleanly_without_an_engine_or_a_device(q3):
    L = q3.lib()
    rows, sid, st, n = np.ones((3, 2048), np.float32), C.c_int32(-5), C.c_int32(-9), C.c_int32(-8)
    for fn in (L.q3tts_stem_create, L.q3tts_group_stem_create):
        assert fn(None, q3._p(rows), 3, C.byref(sid)) < 0 and L.q3tts_last_error() and sid.value == -5
    for fn in (L.q3tts_voice_stem_create, L.q3tts_group_voice_stem_create):
        assert fn(None, 0, 2055, None, 0, C.byref(sid)) < 0 and L.q3tts_last_error() and sid.value == -5
    assert L.q3tts_stem_poll(None, 0, C.byref(st), None) < 0 and L.q3tts_last_error() and st.value == -9
    for fn in (L.q3tts_stem_wait, L.q3tts_group_stem_wait):
        assert fn(None, 0, 0.0) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_stem_release, L.q3tts_group_stem_release, L.q3tts_engine_set_stem, L.q3tts_group_set_stem):
        assert fn(None, 0) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_voice_set_stem, L.q3tts_group_voice_set_stem):
        assert fn(None, 0, 0) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_request_stem, L.q3tts_group_request_stem):
        assert fn(None, 1, C.byref(sid), C.byref(n)) < 0 and L.q3tts_last_error() and (sid.value, n.value) == (-5, -8)
    s = q3.StemStats(built=-7)
    for fn in (L.q3tts_engine_stem_stats, L.q3tts_group_stem_stats):
        assert fn(None, C.byref(s)) < 0 and L.q3tts_last_error() and s.built == -7
    with pytest.raises(q3.Q3Error):
        q3.group_stem_create(None, rows)
    with pytest.raises(q3.Q3Error):
        q3.group_set_stem(None, None)


def test_kernel_surface_refuses_before_it_touches_a_device(q3):
    """every precondition of q3tts_op_kv_stem is checked before anything is uploaded or launched, so the refusals need no GPU"""
    k = np.zeros((4, 1, 1, 8192), np.uint16)
    st = np.zeros((2, 1, 1, 8192), np.uint16)
    pt = np.array([[0, 1], [2, 3]], np.int32)

    def run(jobs, save=False, table=pt, store=st):
        return q3.op_kv_stem(k, k, table, store, store, jobs, save)
    for jobs, save, why in (([], False, "n_jobs"), ([(0, 0, [0])], False, "n_pages"), ([(0, 3, [0])], False, "n_pages"),
                            ([(1, 2, [0])], False, "store range"), ([(-1, 1, [0])], False, "store range"), ([(0, 1, [])], False, "n_dst"),
                            ([(0, 1, [0, 1])], True, "n_dst"), ([(0, 1, [2])], False, "slot out of range"), ([(0, 1, [-1])], False, "slot out of range"),
                            ([(0, 1, [0, 0])], False, "coincide"), ([(0, 1, [0]), (1, 1, [0])], False, "coincide"),
                            ([(0, 2, [0]), (1, 1, [1])], True, "overlap")):
        with pytest.raises(q3.Q3Error, match=why):
            run(jobs, save)
    with pytest.raises(q3.Q3Error, match="page table entry"):
        run([(0, 1, [1])], table=np.array([[0, 1], [4, 3]], np.int32))
    with pytest.raises(q3.Q3Error, match="caches and stores"):
        run([(0, 1, [0])], store=np.zeros((2, 1, 2, 8192), np.uint16))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("stem_logic") / "stem_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "stem_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr + r.stdout
        return r.stdout.splitlines()
    return run


def _refusal(driver, n=10, max_prompt=256, live=0, ggml=0, null_rows=0):
    return driver("refusal %d %d %d %d %d\n" % (n, max_prompt, live, ggml, null_rows))[0]


def test_every_refusal_and_the_accepting_edges(driver):
    assert _refusal(driver) == "ok"
    assert _refusal(driver, n=1) == "ok" and _refusal(driver, n=255) == "ok"
    assert "below max_prompt" in _refusal(driver, n=256) and "below max_prompt" in _refusal(driver, n=1000)
    assert "n_rows must be >= 1" in _refusal(driver, n=0) and "n_rows must be >= 1" in _refusal(driver, n=-4)
    assert "rows missing" in _refusal(driver, null_rows=1)
    assert _refusal(driver, live=63) == "ok"
    assert "Q3TTS_MAX_STEMS" in _refusal(driver, live=64) and "Q3TTS_MAX_STEMS" in _refusal(driver, live=300)
    assert "Q3_SPEC=ggml" in _refusal(driver, ggml=1)
    assert "Q3_SPEC=ggml" in _refusal(driver, ggml=1, null_rows=1, n=0, live=64)   # the mode comes first: nothing else is looked at
    assert "below max_prompt" in _refusal(driver, n=256, live=64)                  # a bad count is reported before the table is full


def test_setters_take_ready_stems_only(driver):
    assert driver("set 1 %d\n" % READY)[0] == "ok"
    assert "building" in driver("set 1 %d\n" % BUILDING)[0]
    assert "failed" in driver("set 1 %d\n" % FAILED)[0]
    for st in (BUILDING, READY, FAILED):
        assert "unknown stem" in driver("set 0 %d\n" % st)[0]


def test_which_stem_applies(driver):
    def of(asked, eng):
        return int(driver("of %d %d\n" % (asked, eng))[0])
    assert of(-2, 5) == 5 and of(-2, -1) == -1          # a raw-prompt form: the engine-level setting
    assert of(3, 5) == 3 and of(-1, 5) == -1            # a text form: its voice's, never the engine's


def _takes(driver, state=READY, n=3, n_prompt=5, score=0, drow=-1, dcol=0, negzero=0):
    return int(driver("takes %d %d %d %d %d %d %d\n" % (state, n, n_prompt, score, drow, dcol, negzero))[0])


def test_the_take_rule(driver):
    assert _takes(driver) == 1
    assert _takes(driver, n_prompt=3) == 0                         # n_prompt == n: the request would have no row of its own
    assert _takes(driver, n_prompt=2) == 0
    assert _takes(driver, n_prompt=4) == 1                         # n_prompt == n + 1
    assert _takes(driver, n=1, n_prompt=2) == 1
    assert _takes(driver, drow=2, dcol=2047) == 0                  # one differing float, the last of the last stem row
    assert _takes(driver, drow=2, dcol=0) == 0 and _takes(driver, drow=0, dcol=0) == 0 and _takes(driver, drow=1, dcol=1000) == 0
    assert _takes(driver, drow=3, dcol=0) == 1 and _takes(driver, drow=4, dcol=2047) == 1   # the request's own rows are its own
    assert _takes(driver, drow=1, dcol=7, negzero=1) == 0          # bytes, not values: -0 is not +0
    assert _takes(driver, state=BUILDING) == 0 and _takes(driver, state=FAILED) == 0
    assert _takes(driver, score=1) == 0                            # a score request never takes a stem
    assert driver("takes_null\n")[0] == "0 0"


def test_packer_with_skips_is_the_plain_packing_with_the_skipped_entries_removed(driver):
    tokens = skipped = chunks = 0
    for seed in (1, 2, 3, 4):
        out = driver("packer %d 60\n" % seed)[0].split()
        assert out[0] == "ok", out
        tokens += int(out[1]); skipped += int(out[2]); chunks += int(out[3])
    assert tokens > 10000 and skipped > 2000 and chunks > 400       # the batches did skip rows and did span chunks
    assert driver("score_runs 7 80\n")[0] == "ok"                  # a score request beside skipping wave-mates keeps its head rows


def test_admission_row_counts(driver):
    def rows(n_prompt, n_skip, n_prefix):
        return int(driver("rows %d %d %d\n" % (n_prompt, n_skip, n_prefix))[0])
    assert rows(330, 0, 0) == 330 and rows(330, 300, 0) == 30 and rows(330, 300, 12) == 42 and rows(301, 300, 0) == 1

    def take(free_slots, free_codec, limit, entries, max_rows=4096):
        return int(driver("take %d %d %d %d %d %s\n" % (free_slots, free_codec, limit, max_rows, len(entries),
                                                         " ".join("%d %d %d" % e for e in entries)))[0])
    plain = [(330, 0, 0)] * 20
    stemmed = [(rows(330, 300, 0), 0, 0)] * 20
    assert take(32, 0, 1, plain) == 12                  # 4096 rows of staging: 12 x 330 fit, the 13th does not
    assert take(32, 0, 1, stemmed) == 20                # behind a 300-row stem all 20 fit: 600 rows
    assert take(32, 0, 0, plain) == 20
    assert take(32, 0, 1, [(5000, 0, 0), (30, 0, 0)]) == 1   # the first entry is always taken; admission_take itself is unchanged
    assert take(3, 0, 1, [(30, 0, 9), (30, 0, 9), (30, 0, 9), (30, 0, 9)]) == 0   # a set of four in three slots: none


def test_store_size(driver):
    assert driver("store 1 28 8\n")[0] == "1 %d" % (2 * 1 * 28 * 8 * 8192 * 2)
    assert driver("store 64 28 8\n")[0].split()[0] == "1" and driver("store 65 28 8\n")[0].split()[0] == "2"
    assert driver("store 300 28 8\n")[0] == "5 %d" % (2 * 5 * 28 * 8 * 8192 * 2)
    assert driver("store 200 2 2\n")[0] == "4 %d" % (2 * 4 * 2 * 2 * 8192 * 2)


def test_holder_table(driver):
    assert driver("fresh\n")[0] == "1 0 %d 0" % BUILDING      # its creator holds it, it is building, it is not recyclable

    def rec(creator, holders, state):
        return int(driver("recyclable %d %d %d\n" % (creator, holders, state))[0])
    table = [
        (1, 0, BUILDING, 0), (1, 0, READY, 0), (1, 3, READY, 0), (1, 0, FAILED, 0),       # the creator has not released it
        (0, 1, READY, 0), (0, 2, READY, 0), (0, 1, FAILED, 0),                            # a voice, the engine or a request still holds it
        (0, 0, BUILDING, 0), (0, 1, BUILDING, 0),                                         # released while it builds: the wave still writes its pages
        (0, 0, READY, 1), (0, 0, FAILED, 1),                                              # nobody left, the build has ended
    ]
    for creator, holders, state, want in table:
        assert rec(creator, holders, state) == want, (creator, holders, state)
