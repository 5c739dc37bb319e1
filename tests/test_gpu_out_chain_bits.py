"""[EXT] output formats / speaking rate / pitch / volume / loudness through the engine: requests are given the bytes they were given before
what sits between the codec decoder and the stage launchers -- routing, lazy making of the stages, resets, the flush, the converter history
of a primed stream -- became one OutChain (csrc/out_chain.h).

tests/golden/out_chain_digests.json was recorded by scripts/out_chain_digest.py on an MI355X against the build of commit f7fa361 ("Voice
intake: reference audio at any rate and format, on the device"), the last one in which CodecDecoder::Impl held the five stages itself.  One
SHA-1 per case over every request's codes, delivered bytes, delivered sample count and loudness rows; the stage counters the script prints
are not part of it.  tests/test_gpu_output_stage_bits.py holds the launchers to their recorded bytes; this one holds the path above them.  A
digest that differs means the chain changed what a request is given: the fixture is not re-recorded for that."""
import importlib.util
import json
import os

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "out_chain_digests.json")) as f:
    GOLDEN = json.load(f)


@pytest.fixture(scope="module")
def digests(gpu, synth_tool):
    spec = importlib.util.spec_from_file_location("out_chain_digest", os.path.join(ROOT, "scripts", "out_chain_digest.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    got = {}
    for name, digest, counters in mod.cases(gpu, mod.model()):
        print("%s  %s  %s" % (digest, name, json.dumps(counters, sort_keys=True)))
        got[name] = digest
    return got


def test_the_cases_are_the_recorded_ones(digests):
    assert sorted(digests) == sorted(GOLDEN)


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_requests_are_given_what_the_recorded_build_gave_them(digests, name):
    assert digests[name] == GOLDEN[name]
