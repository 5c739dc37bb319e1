"""[EXT] token log-probabilities, CPU half: the entry points are declared, exported, listed and fail cleanly without an engine or a device;
the frame-variant key keeps its value without the new bit and is distinct with it; and q3_expf -- the one transcendental the kernel shares
with the spec -- is measured against float64, because the tolerance of tests/test_gpu_logprobs.py assumes it is good to a few ulp.
No GPU is used."""
import ctypes as C
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_engine_set_logprobs", "q3tts_fetch_logprobs", "q3tts_group_set_logprobs", "q3tts_group_fetch_logprobs", "q3tts_op_logprob_rows")


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_names_are_declared_exported_and_listed(q3):
    txt = _header("q3tts.h")
    assert re.search(r"^#define\s+Q3TTS_LOGPROB_COLS\s+17\b", txt, flags=re.M)
    assert re.search(r"^#define\s+Q3TTS_LOGPROB_NONE\s+1\.0f\b", txt, flags=re.M)
    spec = _header("q3tts_spec.h")
    assert re.search(r"^#define\s+Q3_LOGPROB_COLS\s+17\b", spec, flags=re.M) and re.search(r"^#define\s+Q3_LOGPROB_NONE\s+1\.0f\b", spec, flags=re.M)
    assert re.search(r"\bint\s+q3tts_engine_set_logprobs\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_group_set_logprobs\s*\(\s*q3tts_group\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*\)\s*;", txt)
    for who, first in (("q3tts_fetch_logprobs", "q3tts_engine"), ("q3tts_group_fetch_logprobs", "q3tts_group")):
        assert re.search(r"\bint\s+%s\s*\(\s*%s\s*\*\s*\w+\s*,\s*int64_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*int32_t\s+\w+\s*,"
                         r"\s*int32_t\s*\*\s*\w+\s*\)\s*;" % (who, first), txt), who
    assert re.search(r"\bint\s+q3tts_op_logprob_rows\s*\(\s*const\s+float\s*\*\s*\w+\s*,\s*int32_t\s+B\s*,\s*int32_t\s+n\s*,\s*int32_t\s+stride\s*,"
                     r"\s*const\s+int32_t\s*\*\s*\w+\s*,\s*int32_t\s+\w+\s*,\s*float\s*\*\s*\w+\s*,\s*float\s*\*\s*\w+\s*\)\s*;", txt)
    for n in NEW:
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n), n
    # no struct changed: the request, status and options layouts are the ones the earlier features left
    assert [f for f, _ in q3.ReqStatus._fields_] == ["state", "n_frames", "n_pcm", "queue_ms", "prefill_ms", "first_chunk_ms", "total_ms"]
    assert [f for f, _ in q3.GenOptions._fields_] == ["repetition_penalty", "predictor_temperature", "predictor_top_k", "predictor_top_p"]


def test_the_spec_states_what_is_pinned():
    raw = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    sec = raw[raw.index("token log-probabilities [EXT]"):]
    sec = sec[:sec.index("#define Q3_LOGPROB_COLS")]
    assert "NOT a bit-exact spec item" in sec and "1e-5 * max(1, |lp64|)" in sec and "Q3_LOGPROB_NONE" in sec


def test_python_surface(q3):
    assert callable(q3.Engine.set_logprobs) and callable(q3.Engine.fetch_logprobs) and callable(q3.op_logprob_rows)
    assert callable(q3.group_set_logprobs) and callable(q3.group_fetch_logprobs)
    assert (q3.LOGPROB_COLS, q3.LOGPROB_NONE) == (17, 1.0)
    L = q3.lib()
    assert all(getattr(L, n).argtypes for n in NEW)


def test_entry_points_fail_cleanly_without_an_engine_or_a_device(q3):
    L = q3.lib()
    out, got = np.zeros(17 * 4, np.float32), C.c_int32(-5)
    for fn in (L.q3tts_engine_set_logprobs, L.q3tts_group_set_logprobs):
        for on in (1, 0):
            assert fn(None, on) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_fetch_logprobs, L.q3tts_group_fetch_logprobs):
        for rid in (1, 0, -3, 987654321):
            assert fn(None, rid, q3._p(out), 0, 4, C.byref(got)) < 0 and L.q3tts_last_error()
    assert got.value == -5 and not out.any()                             # nothing was written
    lg, ch, o = np.zeros((2, 8), np.float32), np.zeros(2, np.int32), np.full(2, 7.0, np.float32)
    if q3.device_count() == 0:
        assert L.q3tts_op_logprob_rows(q3._p(lg), 2, 8, 8, q3._p(ch), -1, q3._p(o), None) < 0
        assert b"no HIP device" in L.q3tts_last_error()                  # no CPU fallback
    # bad arguments are refused before anything is launched, with or without a device
    for args in ((None, 2, 8, 8, q3._p(ch), -1, q3._p(o), None), (q3._p(lg), 2, 8, 8, None, -1, q3._p(o), None), (q3._p(lg), 2, 8, 8, q3._p(ch), -1, None, None),
                 (q3._p(lg), 0, 8, 8, q3._p(ch), -1, q3._p(o), None), (q3._p(lg), 2, 9, 8, q3._p(ch), -1, q3._p(o), None),
                 (q3._p(lg), 2, 8, 8, q3._p(ch), 8, q3._p(o), q3._p(o)), (q3._p(lg), 2, 8, 8, q3._p(ch), 3, q3._p(o), None)):
        assert L.q3tts_op_logprob_rows(*args) < 0 and L.q3tts_last_error()
    assert np.all(o == 7.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("logprob_logic") / "logprob_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "logprob_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_variant_key_keeps_its_values_and_the_new_bit_is_distinct(driver):
    combos = [(w,) + f for w in (1, 2, 4, 64, 512) for f in itertools.product((0, 1), repeat=5)]
    off = [int(x) for x in driver("".join("key %d %d %d %d %d %d 0\n" % c for c in combos))]
    on = [int(x) for x in driver("".join("key %d %d %d %d %d %d 1\n" % c for c in combos))]
    assert off == [w * 32 + gate * 16 + trail * 8 + pred * 4 + pen * 2 + sampled for (w, sampled, pen, pred, trail, gate) in combos]
    assert len(set(off + on)) == 2 * len(combos)                         # no graph with the bit shares a cache entry with one without
    assert min(on) > max(off)


def test_variant_bit_comes_from_live_recording_slots_only(driver):
    cases = {"nobody records": ([(1, 0), (1, 0)], 0), "a live slot records": ([(1, 0), (1, 1), (0, 0)], 1),
             "only a slot that is not live records": ([(1, 0), (0, 1)], 0), "no live slot": ([(0, 1), (0, 1)], 0)}
    for name, (slots, want) in cases.items():
        out = driver("variant %d\n" % len(slots) + "".join("%d %d\n" % s for s in slots))
        assert [int(x) for x in out[0].split()] == [0, 0, 0, 0, 0, want], name


def test_q3_expf_is_good_to_a_few_ulp(driver):
    """The tolerance 1e-5 * max(1, |lp|) budgets "a few ulp" for q3_expf.  Measured against double exp: on [-87, 0] in f32 ulps of the result
    (0.997 at x = -5.874 when this was written; above 4 the tolerance would have to be widened by the excess).  On [-88, -87) q3_expf
    returns 0 by definition (q3tts_spec.h) -- a relative error of 1 that no ulp count describes; what reaches the log-probability there is
    the ABSOLUTE error of a term of a sum that is >= 1 (the maximum's own term is exactly 1): below e^-87 = 1.65e-38 a term, 6.8e-35 over
    4096 terms, thirty orders of magnitude under the tolerance.  So the tolerance stays as it is."""
    out = driver("expf 2000000\n")
    worst_ulp, at = (float(x) for x in out[0].split())
    worst_abs = float(out[1])
    print("q3_expf: worst %.4f ulp on [-87, 0] at x = %.9g; worst absolute error on [-88, -87): %.4g" % (worst_ulp, at, worst_abs))
    assert worst_ulp <= 4.0
    assert worst_abs <= 1.7e-38
    assert 4096 * worst_abs < 1e-30
