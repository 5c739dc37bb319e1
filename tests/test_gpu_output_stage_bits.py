"""[EXT] output formats / speaking rate / pitch: the three output stages give the bytes they gave before their shared code was factored out.

tests/golden/output_stage_digests.json was recorded by scripts/output_stage_digest.py on an MI355X against the build of commit 8c500c2
("Test the engine at every step width up to 256 slots against narrow runs"), the last one in which k_tsm_stretch, k_tsm_pitch and
k_pcm_convert each carried their own copy of the frame step, the upload ring and the int16 packing.  One SHA-1 per case over every byte
q3tts_op_pcm_convert, q3tts_op_tsm and q3tts_op_pitch return: the outputs and traces with their guards, the counts, the history stores.  The
other GPU tests of these kernels judge them against float64 with bounds; this one holds a change that is meant to compute nothing new to
the same bits.  A digest that differs means the kernels or their launchers changed what they compute: the fixture is not re-recorded for that.

tests/golden/output_stage_volume_digests.json is the same for q3tts_op_volume (volume_cases of the script), recorded against the build of commit
87dfdfc ("Volume: gain with a look-ahead limiter on the device, any output stage"), the last one in which the four entry points' Python
wrappers each carried their own prelude and postlude."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "output_stage_digests.json")) as f:
    GOLDEN = json.load(f)
with open(os.path.join(ROOT, "tests", "golden", "output_stage_volume_digests.json")) as f:
    GOLDEN_VOLUME = json.load(f)


@pytest.fixture(scope="module")
def script():
    spec = importlib.util.spec_from_file_location("output_stage_digest", os.path.join(ROOT, "scripts", "output_stage_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def digests(gpu, script):
    return dict(script.cases(gpu))


def test_the_cases_are_the_recorded_ones(digests):
    assert sorted(digests) == sorted(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_bytes_are_those_of_the_recorded_build(digests, name):
    assert digests[name] == GOLDEN[name]


def test_the_volume_stage_gives_the_bytes_of_the_recorded_build(gpu, script):
    assert dict(script.volume_cases(gpu)) == GOLDEN_VOLUME
