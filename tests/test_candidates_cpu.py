"""[EXT] candidate sets, CPU half (include/q3tts_spec.h "candidate sets"): the entry points are declared, exported, listed and fail cleanly
without an engine or a device; every refusal of q3tts_submit_candidates that needs no engine is reached through the pure rule of
csrc/sched_logic.h, and the admission rule -- how many queue entries the next wave takes -- is checked over a table and, for queues without
a set, against the loop the scheduler ran before sets existed.  The rules are built with plain g++ and the host sanitizers, like the other
rule drivers.  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_submit_candidates", "q3tts_group_submit_candidates", "q3tts_engine_candidate_stats", "q3tts_op_kv_fork")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_names_are_declared_exported_and_listed(q3):
    txt = _header("q3tts.h")
    tail = (r"\s*const\s+q3tts_request\s*\*\s*r\s*,\s*int32_t\s+want_pcm\s*,\s*const\s+q3tts_gen_options\s*\*\s*opts\s*,"
            r"\s*const\s+int32_t\s*\*\s*trail_ids\s*,\s*int32_t\s+n_trail\s*,\s*const\s+uint64_t\s*\*\s*seeds\s*,\s*int32_t\s+n\s*,"
            r"\s*int64_t\s*\*\s*req_ids\s*\)\s*;")
    assert re.search(r"\bint\s+q3tts_submit_candidates\s*\(\s*q3tts_engine\s*\*\s*\w+\s*," + tail, txt)
    assert re.search(r"\bint\s+q3tts_group_submit_candidates\s*\(\s*q3tts_group\s*\*\s*\w+\s*,\s*int32_t\s+engine_index\s*," + tail, txt)
    assert re.search(r"\bint\s+q3tts_engine_candidate_stats\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*int64_t\s*\*\s*sets\s*,"
                     r"\s*int64_t\s*\*\s*prefill_rows_saved\s*,\s*int64_t\s*\*\s*pages_copied\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_op_kv_fork\s*\(\s*uint16_t\s*\*\s*k_cache\s*,\s*uint16_t\s*\*\s*v_cache\s*,\s*int32_t\s+n_pages\s*,"
                     r"\s*int32_t\s+n_layer\s*,\s*int32_t\s+n_kv\s*,\s*const\s+int32_t\s*\*\s*page_table\s*,\s*int32_t\s+n_seq\s*,"
                     r"\s*int32_t\s+max_pages\s*,\s*int32_t\s+src_seq\s*,\s*const\s+int32_t\s*\*\s*dst_seqs\s*,\s*int32_t\s+n_dst\s*,"
                     r"\s*int32_t\s+n_positions\s*\)\s*;", txt)
    for n in NEW:
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n) and getattr(q3.lib(), n).argtypes, n
    raw = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    doc = raw[raw.index("[EXT] candidate sets"):raw.index("int q3tts_submit_candidates")]
    assert "No resumed prefix and no open trail" in doc and "admitted whole" in doc
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    sec = spec[spec.index("candidate sets [EXT]"):]
    assert "seeds[i]" in sec and "whole pages" in sec and "Q3_PRED_SEED_XOR" in sec


def test_python_surface(q3):
    assert callable(q3.Engine.submit_candidates) and callable(q3.Engine.candidate_stats)
    assert callable(q3.group_submit_candidates) and callable(q3.op_kv_fork)


def test_entry_points_fail_cleanly_without_an_engine_or_a_device(q3):
    L = q3.lib()
    prompt, seeds, ids = np.zeros((3, 2048), np.float32), np.arange(2, dtype=np.uint64), np.full(2, -5, np.int64)
    r = q3.Request()
    r.prompt, r.n_prompt, r.max_steps = prompt.ctypes.data, 3, 4
    assert L.q3tts_submit_candidates(None, C.byref(r), 0, None, None, 0, q3._p(seeds), 2, q3._p(ids)) < 0 and L.q3tts_last_error()
    assert L.q3tts_group_submit_candidates(None, -1, C.byref(r), 0, None, None, 0, q3._p(seeds), 2, q3._p(ids)) < 0 and L.q3tts_last_error()
    assert np.all(ids == -5)
    a = C.c_int64(-7)
    assert L.q3tts_engine_candidate_stats(None, C.byref(a), None, None) < 0 and L.q3tts_last_error() and a.value == -7
    # the kernel's test surface: NULL buffers and every refusal come before the device is looked for, and leave the buffers alone
    rng = np.random.default_rng(1)
    k, v = rng.integers(0, 65536, (4, 1, 1, 8192)).astype(np.uint16), rng.integers(0, 65536, (4, 1, 1, 8192)).astype(np.uint16)
    k0, v0 = k.copy(), v.copy()
    pt, dst = np.array([[0, 1], [2, 3]], np.int32), np.array([1], np.int32)

    def fork(kc=k, vc=v, table=pt, n_seq=2, src=0, d=dst, n_dst=1, n_pos=65):
        return L.q3tts_op_kv_fork(q3._p(kc), q3._p(vc), 4, 1, 1, q3._p(table), n_seq, 2, src, q3._p(d), n_dst, n_pos)
    for bad in (dict(kc=None), dict(vc=None), dict(table=None), dict(d=None), dict(n_dst=0), dict(n_pos=0), dict(n_pos=129), dict(src=2), dict(src=-1),
                dict(d=np.array([2], np.int32)), dict(d=np.array([0], np.int32)), dict(d=np.array([1, 1], np.int32), n_dst=2),
                dict(table=np.array([[0, 1], [2, 4]], np.int32)), dict(table=np.array([[0, 1], [2, -1]], np.int32)),
                dict(table=np.array([[0, 1], [2, 1]], np.int32)), dict(table=np.array([[0, 0], [2, 3]], np.int32))):
        assert fork(**bad) < 0 and L.q3tts_last_error() and b"no HIP device" not in L.q3tts_last_error(), bad
    if q3.device_count() == 0:
        assert fork() < 0 and b"no HIP device" in L.q3tts_last_error()
        with pytest.raises(q3.Q3Error, match="no HIP device"):
            q3.op_kv_fork(k, v, pt, 0, [1], 65)
    assert np.array_equal(k, k0) and np.array_equal(v, v0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("candidates_logic") / "candidates_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "candidates_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _refusal(driver, n=4, max_batch=8, null_seeds=0, null_ids=0, null_trail=0, n_trail=0, max_prompt=32, ggml=0):
    return driver("refusal %d %d %d %d %d %d %d %d\n" % (n, max_batch, null_seeds, null_ids, null_trail, n_trail, max_prompt, ggml))[0]


def test_every_refusal(driver):
    assert _refusal(driver) == "ok"
    assert _refusal(driver, n=1) == "ok"                                 # a set of one is a plain submission
    assert _refusal(driver, n=8) == "ok"                                 # exactly max_batch
    assert "n must be >= 1" in _refusal(driver, n=0)
    assert "n must be >= 1" in _refusal(driver, n=-2)
    assert "max_batch" in _refusal(driver, n=9)
    assert "seeds missing" in _refusal(driver, null_seeds=1)
    assert "req_ids missing" in _refusal(driver, null_ids=1)
    assert "n_trail" in _refusal(driver, n_trail=-1)
    assert "n_trail" in _refusal(driver, n_trail=33)
    assert _refusal(driver, n_trail=32) == "ok"
    assert "trailing ids missing" in _refusal(driver, n_trail=2, null_trail=1)
    assert _refusal(driver, n_trail=0, null_trail=1) == "ok"
    assert "Q3_SPEC=ggml" in _refusal(driver, ggml=1)
    assert "Q3_SPEC=ggml" in _refusal(driver, ggml=1, n=1)


def _take(driver, free_slots, free_codec, limit, q):
    return int(driver("take %d %d %d %d\n%s\n" % (free_slots, free_codec, limit, len(q), "\n".join("%d %d %d" % e for e in q)))[0])


def _old_loop(free_slots, free_codec, limit, q):
    """the admission loop before sets: one slot each, a codec stream with PCM, the 4096 rows of an asynchronous wave"""
    take = rows = 0
    for n, pcm, _ in q:
        if free_slots == 0 or (pcm and free_codec == 0) or (limit and take > 0 and rows + n > 4096):
            break
        take, rows, free_slots, free_codec = take + 1, rows + n, free_slots - 1, free_codec - pcm
    return take


def test_admission_table(driver):
    P, S = (10, 0, 0), lambda rows, k, sid, pcm=0: [(rows, pcm, sid)] * k   # a plain request; a set of k members
    # a set at the head with too few slots takes nothing, and nothing behind it is taken
    assert _take(driver, 2, 8, 0, S(10, 3, 1) + [P]) == 0
    assert _take(driver, 2, 8, 1, S(10, 3, 1) + [P, P]) == 0
    # ... or too few codec streams
    assert _take(driver, 4, 2, 0, S(10, 3, 1, pcm=1) + [P]) == 0
    assert _take(driver, 4, 3, 0, S(10, 3, 1, pcm=1) + [P]) == 4
    assert _take(driver, 4, 0, 0, S(10, 3, 1) + [P]) == 4                 # codes only: no stream needed
    # a set that fits exactly is taken whole
    assert _take(driver, 3, 8, 0, S(10, 3, 1)) == 3
    assert _take(driver, 3, 8, 0, S(10, 3, 1) + [P]) == 3
    # a set behind plain requests: the plain ones go, the set waits whole
    assert _take(driver, 4, 8, 0, [P, P] + S(10, 3, 1) + [P]) == 2
    assert _take(driver, 5, 8, 0, [P, P] + S(10, 3, 1) + [P]) == 5
    assert _take(driver, 6, 8, 0, [P, P] + S(10, 3, 1) + [P]) == 6
    # two sets: ids tell them apart, each is whole or absent
    assert _take(driver, 5, 8, 0, S(10, 3, 1) + S(10, 3, 2)) == 3
    assert _take(driver, 6, 8, 0, S(10, 3, 1) + S(10, 3, 2)) == 6
    assert _take(driver, 6, 4, 0, S(10, 3, 1, pcm=1) + S(10, 3, 2, pcm=1)) == 3
    # the 4096 rows of an asynchronous wave: a set's rows count once
    assert _take(driver, 8, 8, 1, S(1000, 4, 1) + [(3096, 0, 0)]) == 5
    assert _take(driver, 8, 8, 1, S(1000, 4, 1) + [(3097, 0, 0)]) == 4
    assert _take(driver, 8, 8, 1, [(3097, 0, 0)] + S(1000, 4, 1)) == 1
    assert _take(driver, 8, 8, 1, [(3096, 0, 0)] + S(1000, 4, 1)) == 5
    assert _take(driver, 8, 8, 0, [(3097, 0, 0)] + S(1000, 4, 1)) == 5   # no limit on an in-line wave
    assert _take(driver, 8, 8, 1, S(5000, 4, 1) + [P]) == 4               # the wave's first entry is never refused for its rows
    # a set with cancelled members: those left the queue, the rest is the set
    assert _take(driver, 2, 8, 0, S(10, 2, 1) + [P]) == 2
    assert _take(driver, 1, 8, 0, S(10, 1, 1) + [P]) == 1
    # nothing free, nothing queued
    assert _take(driver, 0, 8, 0, [P]) == 0 and _take(driver, 4, 8, 0, []) == 0


def test_queues_without_a_set_are_taken_as_before(driver):
    rng = np.random.default_rng(5)
    cases = []
    for _ in range(300):
        q = [(int(rng.integers(1, 2500)), int(rng.integers(0, 2)), 0) for _ in range(int(rng.integers(0, 9)))]
        cases.append((int(rng.integers(0, 7)), int(rng.integers(0, 5)), int(rng.integers(0, 2)), q))
    got = driver("".join("take %d %d %d %d\n%s\n" % (s, c, l, len(q), "\n".join("%d %d %d" % e for e in q)) for s, c, l, q in cases))
    assert [int(g) for g in got] == [_old_loop(*c) for c in cases]
