"""[EXT] the one record of a stream's output settings (OutSpec, csrc/sched_logic.h) without a GPU: its submit rule returns the very pointer the
chain of the volume's, the pitch's and the rate's rules returned, its kind is the expression the codec's pass tail classified a stream with,
and its delivered counts give, chunk for chunk, the bytes the decoder thread staged in three different ways.  The routing of a pass's streams
behind the output conv (out_route) says which stages run, what each is handed per stream and where each stream's copy comes from as the
pass tail's own expressions said it.  tests/host/out_spec_logic_main.cpp restates them all and checks the grids itself, as a stand-alone
program under the host sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("out_spec_logic") / "out_spec_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "out_spec_logic_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(l.split() for l in r.stdout.splitlines())


def test_the_submit_rule_and_the_kind_over_the_grid(lines):
    """6 rates x 6 pitches x 5 volumes x 16 formats, each at 3 lengths, 2 staging capacities, with and without a codec"""
    assert int(lines["refusals"]) == 6 * 6 * 5 * 16 * 3 * 2 * 2


def test_the_counts_add_up_over_whole_frame_chunks(lines):
    """16 formats x 9 (rate, pitch) pairs x 8 random chunkings of up to 64 frames"""
    assert int(lines["counts"]) == 16 * 9 * 8


def test_the_routing_is_what_the_pass_tail_worked_out(lines):
    """at T = 1920 and 3 x 1920: each of the 6 x 6 x 5 x 16 x 2 single streams, 20000 drawn groups of 2 and of 4, a null out and the
    all-native group at G = 1, 2, 4; then the two refusals"""
    assert int(lines["routes"]) == 2 * (6 * 6 * 5 * 16 * 2 + 2 * 20000 + 3 * 2)
