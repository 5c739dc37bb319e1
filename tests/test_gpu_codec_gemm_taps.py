"""The tap-reusing main loop of k_conv_gemm_h3 (csrc/codec.hip), forced through q3tts_op_codec_gemm as H3 / H3_EPL, against the float64 reference
of tests/codec_gemm_ref.py element by element with the bar of tests/test_gpu_codec_gemm.py: tiles inside a segment, aligned to it and crossing
one or two segment boundaries, both sides of the halo-span limit, 2 and 3 taps, pre-split operands, three epilogues, an A buffer that ends with
the last tile's last row, NaN in every row no output reads, and the same list with the loop switched off in a child process.  (-m gpu)"""
import os
import subprocess
import sys

import pytest

import codec_gemm_taps_cases as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_tap_loop_matches_float64(gpu, case):
    p = T.check_case(gpu, case)
    form, M, N, cin, taps, dil, segT, skip, a_split = case
    if segT == 48 and skip > (taps - 1) * dil:   # two boundaries per tile, segments further apart than the taps reach
        assert T.expects_tap_reuse(case) and p.unused_in_halo >= 1, "no poisoned row inside a halo: %d" % p.unused_in_halo


def test_span_limit_has_a_case_on_each_side(gpu):
    spans = {T.halo_span(c[1], c[4], c[5], c[6], c[7]) for c in T.CASES}
    assert T.HALO_ROWS in spans and T.HALO_ROWS + 1 in spans
    assert 236 in spans   # a 128-row tile over two 64-row segments at dil = 9
    at, over = (next(c for c in T.CASES if T.halo_span(c[1], c[4], c[5], c[6], c[7]) == s) for s in (T.HALO_ROWS, T.HALO_ROWS + 1))
    assert T.Problem(at, 0).query(gpu) is True and T.Problem(over, 0).query(gpu) is False


def test_poisoned_rows_inside_halos_are_counted(gpu):
    """how many rows the loop stages although no output may use them, per two-segment case (reported by -s; at least one each)"""
    for c in T.CASES:
        if c[6] == 48 and c[7] > (c[4] - 1) * c[5]:
            p = T.Problem(c, 0)
            print("%s: %d rows no output reads, %d of them inside a halo" % (T.case_id(c), p.unused, p.unused_in_halo))
            assert p.unused_in_halo >= 1


@pytest.mark.parametrize("case", T.EPI_CASES, ids=T.case_id)
def test_tap_loop_epilogues(gpu, case):
    assert T.expects_tap_reuse(case)
    T.check_epilogues(gpu, case)


def test_same_cases_with_the_loop_switched_off(gpu):
    """Q3_CODEC_H3_TAPS is read once per process, so the tap-major loop runs the list in one fresh child"""
    env = dict(os.environ, Q3_CODEC_H3_TAPS="0")
    r = subprocess.run([sys.executable, os.path.abspath(T.__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "0 failed, tap reuse off" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
