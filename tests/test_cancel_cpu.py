"""[EXT] request cancellation, CPU half: q3tts_cancel / q3tts_group_cancel and Q3TTS_REQ_CANCELLED are declared, exported and listed, fail
cleanly without an engine, the Python wrapper carries them, and the pure rule of csrc/sched_logic.h -- which action a cancel takes in which
request state -- holds over the full table, built with plain g++.  No GPU is used (an unknown id on a live engine: tests/test_gpu_cancel.py)."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUEUED, RUNNING, DRAINING, DONE, CANCELLED, FAILED = 0, 1, 2, 3, 4, -1


def test_names_are_declared_exported_and_listed(q3):
    raw = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"^#define\s+Q3TTS_REQ_CANCELLED\s+4\b", txt, flags=re.M)
    assert re.search(r"\bint\s+q3tts_cancel\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_group_cancel\s*\(\s*q3tts_group\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*\)\s*;", txt)
    for n in ("q3tts_cancel", "q3tts_group_cancel"):
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n), n
    # the struct layouts did not change: the state simply takes the new value
    assert [f for f, _ in q3.ReqStatus._fields_] == ["state", "n_frames", "n_pcm", "queue_ms", "prefill_ms", "first_chunk_ms", "total_ms"]


def test_cancel_fails_cleanly_without_an_engine(q3):
    L = q3.lib()
    for fn in (L.q3tts_cancel, L.q3tts_group_cancel):
        for rid in (1, 0, -3, 987654321):
            assert fn(None, rid) < 0
            assert L.q3tts_last_error()


def test_python_surface(q3):
    assert callable(q3.Engine.cancel)
    assert q3.REQ_CANCELLED == 4
    assert (q3.REQ_QUEUED, q3.REQ_RUNNING, q3.REQ_DRAINING, q3.REQ_DONE, q3.REQ_FAILED) == (0, 1, 2, 3, -1)
    assert q3.lib().q3tts_cancel.argtypes and q3.lib().q3tts_group_cancel.argtypes


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("cancel_logic") / "cancel_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "cancel_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_state_values(driver):
    assert driver("states\n") == ["0 1 2 3 4 -1"]
    assert driver("".join("ended %d\n" % s for s in (QUEUED, RUNNING, DRAINING, DONE, CANCELLED, FAILED))) == ["0", "0", "0", "1", "1", "1"]


def action_ref(state, in_wave, live, want_pcm):
    """the contract of include/q3tts.h, state by state"""
    if state in (DONE, CANCELLED, FAILED):
        return "nothing"                      # the call returns 1
    if state == QUEUED:
        return "at_once"                      # leaves the queue in the caller's thread; it owns no slot, no pages, no stream
    if state == DRAINING:
        return "purge"                        # its slot is gone already; the queued fence ends it
    if live:
        return "retire_fence" if want_pcm else "retire"
    return "at_activate" if in_wave else "nothing"


def test_cancel_action_full_table(driver):
    rows = list(itertools.product((QUEUED, RUNNING, DRAINING, DONE, CANCELLED, FAILED), (0, 1), (0, 1), (0, 1)))
    out = driver("".join("action %d %d %d %d\n" % r for r in rows))
    assert len(out) == len(rows) == 48
    for r, got in zip(rows, out):
        assert got == action_ref(*r), r
    table = dict(zip(rows, out))
    # the rows the engine can reach, spelt out
    assert table[(QUEUED, 0, 0, 0)] == table[(QUEUED, 0, 0, 1)] == "at_once"
    assert table[(RUNNING, 1, 0, 0)] == table[(RUNNING, 1, 0, 1)] == "at_activate"
    assert table[(RUNNING, 0, 1, 0)] == "retire" and table[(RUNNING, 0, 1, 1)] == "retire_fence"
    assert table[(DRAINING, 0, 0, 1)] == "purge"
    assert {table[(s, 0, 0, p)] for s in (DONE, CANCELLED, FAILED) for p in (0, 1)} == {"nothing"}


def test_end_states(driver):
    # a slot given back: codes-only requests end right there, PCM requests drain behind a fence; a cancelled one never reads DONE
    assert driver("retired 0 0\nretired 0 1\nretired 1 0\nretired 1 1\n") == [str(DONE), str(CANCELLED), str(DRAINING), str(DRAINING)]
    assert driver("fenced 0\nfenced 1\n") == [str(DONE), str(CANCELLED)]
