"""The decoder thread's queue bookkeeping (CodecQueue, csrc/sched_logic.h) without a GPU: 200 seeded random sequences of 300 operations --
pushes of generating and decode-only requests, hand-overs, purges, steps, completions -- each followed by a comparison with a shadow: the
pending count, no step during a hand-over, what a purge removes, each request's reset / chunks / fence order, one epoch per step, and the
seats of seat_chunks called on the same heads.  tests/host/codec_queue_logic_main.cpp checks all of it itself, as a stand-alone program
under the host sanitizers; here its counts are held against the run's shape."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("codec_queue_logic") / "codec_queue_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-o", exe, os.path.join(ROOT, "tests", "host", "codec_queue_logic_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (l.split() for l in r.stdout.splitlines())}


def test_every_sequence_ran_to_its_end(counts):
    assert counts["sequences"] == 200 and counts["ops"] == 200 * 300
    assert counts["pushes"] + counts["takes"] + counts["pops"] + counts["purges"] <= counts["ops"]


def test_every_kind_of_operation_occurred(counts):
    assert counts["pushes"] > 0 and counts["steps"] > 0 and counts["pops"] > 0 and counts["handovers"] > 0 and counts["nested"] > 0
    assert counts["held_takes"] > 0                          # a take during a hand-over, which gave nothing
    assert counts["purges"] >= 1 and counts["chunks_purged"] >= 1
    assert counts["tasks_left"] >= counts["steps"]


def test_the_passes_that_matter_occurred(counts):
    assert counts["multi_seat"] >= 1                         # a pass of more than one chunk
    assert counts["shared"] >= 1                             # generating and decode-only chunks in one pass
    assert counts["decode_turns"] >= 1                       # a decode-only chunk led while generating tasks waited (SEAT_DRY_MAX)
