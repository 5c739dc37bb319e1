"""[EXT] output formats / speaking rate / pitch: the three output stages give the bytes they gave before their shared code was factored out.

tests/golden/output_stage_digests.json was recorded by scripts/output_stage_digest.py on an MI355X against the build of commit 8c500c2
("Test the engine at every step width up to 256 slots against narrow runs"), the last one in which k_tsm_stretch, k_tsm_pitch and
k_pcm_convert each carried their own copy of the frame step, the upload ring and the int16 packing.  One SHA-1 per case over every byte
q3tts_op_pcm_convert, q3tts_op_tsm and q3tts_op_pitch return: the outputs and traces with their guards, the counts, the history stores.  The
other GPU tests of these kernels judge them against float64 with bounds; this one holds a change that is meant to compute nothing new to
the same bits.  A digest that differs means the kernels or their launchers changed what they compute: the fixture is not re-recorded for that."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "output_stage_digests.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def digests(gpu):
    spec = importlib.util.spec_from_file_location("output_stage_digest", os.path.join(ROOT, "scripts", "output_stage_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return dict(mod.cases(gpu))


def test_the_cases_are_the_recorded_ones(digests):
    assert sorted(digests) == sorted(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_bytes_are_those_of_the_recorded_build(digests, name):
    assert digests[name] == GOLDEN[name]
