"""The ONNX executor (csrc/onnx_exec.hip) bit for bit: every case of the product, row and zoo tables of tests/onnx_cases.py gives the outputs
(SHA-256 over dtype, shape and bytes) and the launch count recorded in tests/golden/onnx_exec_digests.json, on both kernel families, and
the set of executable operator names is the recorded one.  The fixture was written by scripts/onnx_exec_digest.py --golden on an MI355X with
the library of the commit before the executor became a table of handlers (two recordings, equal); no kernel of the executor uses atomics, so
the bits do not depend on scheduling."""
import json
import os
import subprocess
import sys

import pytest

import onnx_cases as OC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "onnx_exec_digests.json")) as f:
        return json.load(f)


def _compare(got, want):
    assert sorted(got) == sorted(want)                                    # every case, nothing left out
    bad = ["%s: %s launches %d (recorded %s launches %d)" % (k, got[k]["sha256"][:12], got[k]["launches"], want[k]["sha256"][:12], want[k]["launches"])
           for k in sorted(want) if (got[k]["sha256"], got[k]["launches"]) != (want[k]["sha256"], want[k]["launches"])]
    assert not bad, bad


def test_every_case_keeps_its_bits_and_launches(gpu, tmp_path, golden):
    assert len(golden["default"]) == len(OC.product_cases()) + len(OC.row_cases()) + len(OC.zoo_cases())
    _compare(OC.digest_cases(gpu, tmp_path), golden["default"])


def test_every_case_keeps_its_bits_on_the_naive_kernels(gpu, tmp_path, golden):
    """Q3_ONNX_NAIVE is read once when the library loads, so one fresh child process runs every case with it set (scripts/onnx_exec_digest.py
    --naive).  Nothing else uses the GPU while the child runs."""
    out = str(tmp_path / "naive.json")
    env = dict(os.environ, Q3_ONNX_NAIVE="1")
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "onnx_exec_digest.py"), "--naive", "--out", out], env=env, capture_output=True, text=True, timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("the Q3_ONNX_NAIVE child ran into its time limit: nothing further runs on this GPU", returncode=1)
    if r.returncode < 0:
        pytest.exit("the Q3_ONNX_NAIVE child died of signal %d: nothing further runs on this GPU\n%s" % (-r.returncode, r.stderr[-2000:]), returncode=1)
    assert r.returncode == 0, r.stderr[-3000:]
    with open(out) as f:
        _compare(json.load(f), golden["naive"])


def test_the_supported_set_is_pinned(gpu, golden):
    """the 103 names the four hand-kept lists held (33 unary, 19 binary, 11 reduce, 40 other) are executable, each occurs in a case of the
    fixture, and the names that were not executable still are not"""
    assert len(OC.UNARY_OPS) == 33 and len(OC.BINARY_OPS) == 19 and len(OC.REDUCE_OPS + ("ArgMax", "ArgMin")) == 11 and len(OC.OTHER_OPS) == 40
    assert len(set(OC.EXECUTABLE_OPS)) == 103
    assert [op for op in OC.EXECUTABLE_OPS if not gpu.onnx_op_executable(op)] == []
    assert [op for op in OC.NOT_EXECUTABLE_OPS if gpu.onnx_op_executable(op)] == []
    for mode in ("default", "naive"):
        seen = set()
        for case in golden[mode].values():
            seen.update(case["ops"])
        assert sorted(set(OC.EXECUTABLE_OPS) - seen) == [], mode
        assert sorted(seen - set(OC.EXECUTABLE_OPS)) == [], mode
