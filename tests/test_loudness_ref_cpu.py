"""[EXT] loudness without a GPU (include/q3tts_spec.h "loudness"): the K-weighting tables against BS.1770's printed ones and against the
formulas at 24 kHz, the segmented restatement against the plain sequential recurrence, its independence of the chunking and its exact
scaling by powers of two, the 997 Hz sine against the filter's frequency response, the gate case by case, the gain helper, the
declarations and the calls that need no engine, and the host half (csrc/loudness.h) through a plain g++ driver under the host sanitizers,
bit for bit against the numpy restatement."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import loudness_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("q3tts_engine_set_loudness", "q3tts_fetch_loudness", "q3tts_request_loudness", "q3tts_request_metered", "q3tts_engine_loudness_stats",
         "q3tts_group_set_loudness", "q3tts_group_fetch_loudness", "q3tts_group_request_loudness", "q3tts_group_request_metered",
         "q3tts_loudness_tables", "q3tts_loudness_gate", "q3tts_loudness_gain_db10", "q3tts_op_loudness")
N = 6 * R.FRAME   # 11520 samples, 4 whole blocks and most of a fifth

# What bounds the distance between the two float64 evaluation orders.  The high-pass poles sit at radius 0.99 next to z = 1, so a rounding
# of the state (2^-53 relative) is amplified by about 1 / (1 - r)^2 = 1e4 before it decays; where the block energy is small against the
# state -- a DC offset, which the filter removes -- by more.  1e-10 is that with two decades to spare; what the four listed signals really
# differ by is measured below, written into profiles/loudness_f64.md, and eight times it bounds the signals that are not in the list.
F64_CEILING = 1e-10


def ulps(a, b):
    return int(np.abs(R.bits(a).astype(np.int64) - R.bits(b).astype(np.int64)).max())


# A block 50 LU under the absolute gate (-120 LUFS over 400 ms) can change no result of the meter.  The decayed tail behind an impulse lies
# far below that, is rounding residue of the states in both orders, and is compared against this energy instead of its own.
E_FLOOR = 2400.0 * 10.0 ** ((-120.0 + 0.691) / 10.0)


def rel_rows(a, b, floor=0.0):
    """the largest relative block-energy difference of two row sets; floor: the least energy a difference is measured against"""
    assert a.shape == b.shape and a.shape[0] > 0 and np.array_equal(a[:, 1], b[:, 1])
    return float((np.abs(a[:, 0] - b[:, 0]) / np.maximum(b[:, 0], floor)).max())


@pytest.fixture(scope="module")
def tab(q3):
    coef, M = q3.loudness_tables()
    coef.setflags(write=False); M.setflags(write=False)
    return coef, M


LISTED = {"noise": lambda: R.noise(N), "sine 997": lambda: R.sine(N), "dc + 20 Hz": lambda: R.dc_hum(N), "noise 1e-4": lambda: R.noise(N, 1e-4, 11)}
OTHERS = {"noise seed 3": lambda: R.noise(N, 0.5, 3), "square": lambda: R.square(N), "impulse 2399": lambda: R.impulse(N, 2399),
          "sine 60": lambda: R.sine(N, 60.0, 0.7), "dc + noise": lambda: (np.float32(0.5) + R.noise(N, 0.1, 5)).astype(np.float32)}


@pytest.fixture(scope="module")
def measured(tab):
    """the relative block-energy difference segmented - sequential of every listed signal, computed once"""
    coef, M = tab
    out = {}
    for name in sorted(LISTED):
        x = LISTED[name]()
        out[name] = rel_rows(R.segmented(x, coef, M)[0], R.sequential_rows(x, coef))
    return out


# -------------------------------------------------------- the tables --------------------------------------------------------
def test_48k_formulas_give_the_table_printed_in_bs1770():
    c = R.coefs(48000)
    got = (c[0], c[1], c[2], c[3], c[4], c[8], c[9])
    for g, w in zip(got, R.BS1770_48K):
        assert abs(g - w) <= 0.5e-14 + 1e-15, (g, w)                        # its 14 decimals
    assert (c[5], c[6], c[7]) == (1.0, -2.0, 1.0)


def test_24k_tables_are_the_formulas_values(tab):
    coef, M = tab
    got = np.array([coef[0], coef[1], coef[2], coef[3], coef[4], coef[8], coef[9]])
    assert ulps(got, np.array(R.K24)) <= 2
    assert ulps(coef, R.coefs()) <= 2 and tuple(coef[5:8]) == (1.0, -2.0, 1.0)
    assert np.array_equal(R.bits(M), R.bits(R.matrix(coef)))                # M is A^96 of the library's own coefficients, bit for bit
    assert np.abs(np.linalg.eigvals(M)).max() < 1.0


# -------------------------------------------------------- the restatement --------------------------------------------------------
def test_restatement_against_the_sequential_recurrence_on_the_listed_signals(measured):
    for name, v in sorted(measured.items()):
        print("%-12s segmented vs sequential, largest relative block-energy difference: %.3g" % (name, v))
    print("largest: %.3g, bound for other inputs: %.3g" % (max(measured.values()), 8 * max(measured.values())))
    assert 0.0 < max(measured.values()) <= F64_CEILING
    assert max(measured, key=measured.get) == "dc + 20 Hz"                   # the filter removes the offset: small energy against a large state


@pytest.mark.parametrize("name", sorted(OTHERS))
def test_restatement_on_inputs_not_in_the_list(tab, measured, name):
    coef, M = tab
    x = OTHERS[name]()
    got = rel_rows(R.segmented(x, coef, M)[0], R.sequential_rows(x, coef), E_FLOOR)
    print("%-12s %.3g of a bound of %.3g" % (name, got, 8 * max(measured.values())))
    assert got <= 8 * max(measured.values())


def test_schedule_independence_of_the_restatement(tab):
    coef, M = tab
    x = R.noise(5 * R.FRAME)
    rows, state = R.segmented(x, coef, M)
    assert rows.shape == (4, 2)
    for sched in ((1, 1, 1, 1, 1), (4, 1), (2, 3), (1, 4)):
        r, s = R.segmented(x, coef, M, [k * R.FRAME for k in sched])
        assert np.array_equal(R.bits(r), R.bits(rows)) and np.array_equal(R.bits(s), R.bits(state)), sched
    assert state[4] == 0.0 and state[5] == 0.0                              # 5 frames end exactly on a block edge


@pytest.mark.parametrize("k", (-20, -3, 1, 7))
def test_scaling_by_a_power_of_two_scales_the_energies_exactly(tab, k):
    coef, M = tab
    x = R.noise(N, 0.01)
    rows, state = R.segmented(x, coef, M)
    r2, s2 = R.segmented((x * np.float32(2.0 ** k)).astype(np.float32), coef, M)
    assert np.array_equal(R.bits(r2[:, 0]), R.bits(rows[:, 0] * 4.0 ** k)) and np.array_equal(R.bits(r2[:, 1]), R.bits(rows[:, 1] * 2.0 ** k))
    assert np.array_equal(R.bits(s2[:4]), R.bits(state[:4] * 2.0 ** k)) and s2[4] == state[4] * 4.0 ** k


def test_full_scale_997_hz_sine_meets_the_frequency_response(tab):
    coef, M = tab
    rows, _ = R.segmented(R.sine(N), coef, M)
    first = R.gate(rows[:4])["momentary_max_lufs"]
    want = -0.691 + 10.0 * math.log10(0.5) + R.response_db(coef, 997.0)
    print("first 400 ms block of a full-scale 997 Hz sine: %.4f LUFS, from the response: %.4f" % (first, want))
    assert abs(want - -2.9844) < 1e-3                                        # the issue's figure
    assert abs(first - want) <= 0.01                                         # the gap is the high-pass start transient
    assert rows[0, 1] == np.abs(R.sine(N)[:R.BLOCK]).max()


# -------------------------------------------------------- the gate --------------------------------------------------------
def energy_of(l):
    """the 100 ms block energy whose 400 ms blocks, made of four such, measure l LUFS"""
    return 2400.0 * 10.0 ** ((l + 0.691) / 10.0)


def check_gate(q3, rows):
    got, want = q3.loudness_gate(rows), R.gate(rows)
    for k in ("integrated_lufs", "momentary_max_lufs", "peak_dbfs"):
        assert got[k] == want[k] or abs(got[k] - want[k]) <= 1e-12, (k, got, want)
    assert (got["n_blocks"], got["n_gated"]) == (want["n_blocks"], want["n_gated"])
    return got


@pytest.mark.parametrize("n", (0, 1, 3))
def test_gate_fewer_than_four_rows(q3, n):
    g = check_gate(q3, np.array([[energy_of(-20.0), 0.5]] * n).reshape(-1, 2))
    assert g["integrated_lufs"] == -math.inf and g["momentary_max_lufs"] == -math.inf and (g["n_blocks"], g["n_gated"]) == (n, 0)
    assert g["peak_dbfs"] == (-math.inf if n == 0 else 20.0 * math.log10(0.5))


def test_gate_all_silent(q3):
    g = check_gate(q3, np.zeros((12, 2)))
    assert g["integrated_lufs"] == -math.inf and g["momentary_max_lufs"] == -math.inf and g["peak_dbfs"] == -math.inf and g["n_gated"] == 0
    g = check_gate(q3, np.array([[energy_of(-75.0), 1e-4]] * 12))              # audible to the meter, under the absolute gate
    assert g["integrated_lufs"] == -math.inf and abs(g["momentary_max_lufs"] - -75.0) < 1e-9 and g["n_gated"] == 0


def test_gate_steady_signal(q3):
    g = check_gate(q3, np.array([[energy_of(-23.0), 0.1]] * 10))
    assert abs(g["integrated_lufs"] - -23.0) < 1e-9 and abs(g["momentary_max_lufs"] - -23.0) < 1e-9 and g["n_gated"] == 7
    assert abs(g["peak_dbfs"] - -20.0) < 1e-12


@pytest.mark.parametrize("quiet,kept", [(-69.0, False), (-71.0, False), (-45.0, False), (-25.0, True)])
def test_gate_one_loud_stretch_among_quiet_blocks(q3, quiet, kept):
    """eight loud 100 ms blocks (-20) among quiet ones: quiet 400 ms blocks under the absolute gate (-71), over it but under the relative
    gate (-69 and -45: the threshold lies between -36.2, were only the five all-loud blocks to count, and -30), or past both (-25)"""
    rows = np.array([[energy_of(quiet), 0.01]] * 8 + [[energy_of(-20.0), 0.3]] * 8 + [[energy_of(quiet), 0.01]] * 8)
    g = check_gate(q3, rows)
    assert abs(g["momentary_max_lufs"] - -20.0) < 1e-9
    n_loud_only = 5                                                          # the 400 ms blocks made of loud 100 ms blocks alone
    if kept:
        assert g["n_gated"] == 21 and g["integrated_lufs"] < -20.5
    else:
        assert n_loud_only <= g["n_gated"] < 21 and -21.5 < g["integrated_lufs"] <= -20.0 + 1e-9


def test_gate_exact_thresholds(q3):
    """a block exactly at -70 is not past the absolute gate (the comparison is strict); nor is one exactly at the relative threshold"""
    e70 = 2400.0 * 10.0 ** ((-70.0 + 0.691) / 10.0)
    z = (((e70 + e70) + e70) + e70) / 9600.0
    l = -0.691 + 10.0 * math.log10(z)
    g = check_gate(q3, np.array([[e70, 0.001]] * 4))
    assert g["n_gated"] == (1 if l > -70.0 else 0)                           # whichever side the rounding lands on, both agree
    lo, hi = np.nextafter(e70, 0.0), e70 * (1 + 1e-9)
    assert check_gate(q3, np.array([[lo * (1 - 1e-9), 0.001]] * 4))["n_gated"] == 0 and check_gate(q3, np.array([[hi, 0.001]] * 4))["n_gated"] == 1
    # relative: twelve loud rows, then twelve at level x.  The threshold depends on x; the restatement finds the x at which the all-quiet
    # blocks sit on it, and a hundredth of a LU to either side decides whether those nine blocks count
    def rows_at(x):
        return np.array([[energy_of(-20.0), 0.1]] * 12 + [[energy_of(x), 0.1]] * 12)

    def margin(x):
        e = rows_at(x)[:, 0]
        z = [(((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / 9600.0 for j in range(21)]
        return R.lufs(z[-1]) - (R.lufs(sum(z) / 21.0) - 10.0)
    lo, hi = -45.0, -25.0
    assert margin(lo) < 0.0 < margin(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if margin(mid) < 0.0 else (lo, mid)
    assert check_gate(q3, rows_at(hi + 0.01))["n_gated"] == 21 and check_gate(q3, rows_at(lo - 0.01))["n_gated"] == 12


# -------------------------------------------------------- the gain helper --------------------------------------------------------
def test_gain_helper_rounding_clamps_and_non_finite_inputs(q3):
    f = q3.loudness_gain_db10
    assert f(-23.0, -16.0) == 70 and f(-16.0, -23.0) == -70 and f(-20.0, -20.0) == 0
    assert f(-20.04, -16.0) == 40 and f(-20.06, -16.0) == 41 and f(-16.0, -20.06) == -41 and f(-16.0, -20.04) == -40
    assert f(-60.0, -16.0) == R.VOL_MAX and f(-36.0, -16.0) == 200 and f(-36.1, -16.0) == 200 and f(-35.9, -16.0) == 199
    assert f(0.0, -50.0) == R.VOL_MIN and f(-10.0, -50.0) == -400 and f(-10.1, -50.0) == -399
    for bad in (math.inf, -math.inf, math.nan):
        assert f(bad, -16.0) == 0 and f(-16.0, bad) == 0


# -------------------------------------------------------- declarations, no engine --------------------------------------------------------
def test_declarations_and_constants(q3):
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in q3.SYMBOLS and hasattr(q3.lib(), name), name
    for name, val in (("Q3_LOUD_SEG", 96), ("Q3_LOUD_BLOCK", 2400), ("Q3_LOUD_STATE", 6)):
        assert "#define %s %d" % (name, val) in spec, name
    assert (q3.LOUD_SEG, q3.LOUD_BLOCK, q3.LOUD_STATE) == (R.SEG, R.BLOCK, R.STATE)
    assert R.FRAME % R.SEG == 0 and R.BLOCK % R.SEG == 0 and C.sizeof(q3.Loudness) == 32
    assert "typedef struct { double integrated_lufs, momentary_max_lufs, peak_dbfs; int32_t n_blocks, n_gated; } q3tts_loudness;" in hdr


def test_calls_without_an_engine_fail_cleanly(q3):
    L = q3.lib()
    v, a, b, o = C.c_int32(77), C.c_int64(5), C.c_int64(6), q3.Loudness(1.0, 2.0, 3.0, 4, 5)
    buf = np.full(4, 7.0)
    assert L.q3tts_engine_set_loudness(None, 1) < 0 and b"null" in L.q3tts_last_error()
    assert L.q3tts_request_metered(None, 1, C.byref(v)) < 0 and v.value == 77
    assert L.q3tts_fetch_loudness(None, 1, buf.ctypes.data, 0, 2, C.byref(a)) < 0 and a.value == 5 and np.all(buf == 7.0)
    assert L.q3tts_request_loudness(None, 1, C.byref(o)) < 0 and (o.integrated_lufs, o.n_gated) == (1.0, 5)
    assert L.q3tts_engine_loudness_stats(None, C.byref(a), C.byref(b)) < 0 and (a.value, b.value) == (5, 6)
    assert L.q3tts_group_set_loudness(None, 1) < 0 and L.q3tts_group_request_metered(None, 1, C.byref(v)) < 0 and v.value == 77
    assert L.q3tts_group_fetch_loudness(None, 1, buf.ctypes.data, 0, 2, C.byref(a)) < 0 and L.q3tts_group_request_loudness(None, 1, C.byref(o)) < 0
    assert L.q3tts_loudness_tables(None, None) < 0 and L.q3tts_loudness_gate(None, 4, C.byref(o)) < 0 and L.q3tts_loudness_gate(buf.ctypes.data, 2, None) < 0
    assert L.q3tts_loudness_gate(buf.ctypes.data, -1, C.byref(o)) < 0 and o.n_blocks == 4


# -------------------------------------------------------- the host half under the sanitizers --------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("loudness_logic") / "loudness_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "loudness_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def doubles(line):
    return np.array([int(t, 16) for t in line.split()], np.uint64).view(np.float64)


def hexd(v):
    return "%016x" % int(np.array([v], np.float64).view(np.uint64)[0])


def test_host_tables_under_the_sanitizers(driver, tab):
    coef, M = tab
    t = doubles(driver("tables\n")[0])
    assert np.array_equal(R.bits(t[:10]), R.bits(coef)) and np.array_equal(R.bits(t[10:]), R.bits(M.reshape(-1)))
    c48 = doubles(driver("coefs 48000\n")[0])
    assert ulps(c48, R.coefs(48000)) <= 2
    for g, w in zip((c48[0], c48[1], c48[2], c48[3], c48[4], c48[8], c48[9]), R.BS1770_48K):
        assert abs(g - w) <= 0.5e-14 + 1e-15


@pytest.mark.parametrize("sched", [(6,), (1, 1, 1, 1, 1, 1), (4, 2), (1, 5)])
def test_host_segmented_evaluation_is_the_restatement_bit_for_bit(driver, tab, sched):
    coef, M = tab
    x = R.noise(N)
    x[95] = -0.0
    x[2400] = 1.0
    text = "run 0 %d %s\n%s\n" % (len(sched), " ".join(str(k * R.FRAME) for k in sched), " ".join("%08x" % b for b in x.view(np.uint32)))
    out = driver(text)
    rows, state = R.segmented(x, coef, M, [k * R.FRAME for k in sched])
    assert np.array_equal(R.bits(doubles(out[0])), R.bits(rows.reshape(-1))) and np.array_equal(R.bits(doubles(out[1])), R.bits(state))
    assert rows.shape == (4, 2)


def test_host_gate_and_gain_under_the_sanitizers(driver, q3):
    rows = np.array([[energy_of(-40.0), 0.01]] * 6 + [[energy_of(-18.0), 0.4]] * 9 + [[0.0, 0.0]] * 5)
    for r in (rows, rows[:3], rows[:0], np.zeros((8, 2))):
        out = driver("gate %d %s\n" % (r.shape[0], " ".join(hexd(v) for v in r.reshape(-1))))[0].split()
        got, want = doubles(" ".join(out[:3])), q3.loudness_gate(r)
        assert np.array_equal(R.bits(got), R.bits(np.array([want["integrated_lufs"], want["momentary_max_lufs"], want["peak_dbfs"]])))
        assert (int(out[3]), int(out[4])) == (want["n_blocks"], want["n_gated"])
    for a, b in ((-23.0, -16.0), (-20.06, -16.0), (-60.0, -16.0), (0.0, -50.0), (math.nan, -16.0), (-16.0, math.inf)):
        assert int(driver("gain %s %s\n" % (hexd(a), hexd(b)))[0]) == q3.loudness_gain_db10(a, b)
    assert driver("blocks 0 1920\nblocks 1920 1920\nblocks 0 9600\nblocks 7680 1920\nblocks 0 17280\n") == ["0", "1", "4", "1", "7"]


def test_launch_check(driver):
    ok = "launch 3 3 7680 6 0  5 1 0  0 0 0  2 1 3840\n"
    assert driver(ok)[0] == "ok" and driver(ok.replace("7680", "1920"))[0] == "ok"
    for bad in ("7681", "0", "960", "-1920", "2400"):
        assert "1920" in driver(ok.replace("7680", bad))[0], bad
    assert "long" in driver(ok.replace("7680", str(1920 * 10000)))[0]
    assert "group" in driver("launch 0 3 1920 6 0\n")[0] and "group" in driver(ok.replace("launch 3 3", "launch 3 2"))[0]
    assert "group" in driver("launch -1 3 1920 6 0\n")[0]
    for nulls in (1, 2, 3):
        assert "null" in driver(ok.replace("7680 6 0", "7680 6 %d" % nulls))[0]
    assert "once" in driver(ok.replace(" 2 1 3840", " 5 1 3840"))[0] and "once" in driver(ok.replace(" 0 0 0 ", " 5 0 0 "))[0]
    assert "stream out of range" in driver(ok.replace(" 2 1 3840", " 6 1 3840"))[0] and "stream out of range" in driver(ok.replace(" 5 1 0", " -1 1 0"))[0]
    assert "position" in driver(ok.replace(" 2 1 3840", " 2 1 2400"))[0] and "position" in driver(ok.replace(" 2 1 3840", " 2 1 -1920"))[0]
    assert driver(ok.replace(" 0 0 0 ", " 0 0 77 "))[0] == "ok"               # an unmetered stream's position is not looked at


def test_the_shared_launch_checks_come_in_the_order_each_stage_stated_them(driver):
    """group size, chunk, then stream by stream slot, once, own argument -- 5000 inputs with any number of them failing at once (tests/host/stage_preamble.h)"""
    assert driver("preamble\n") == ["preamble 5000"]


def test_submit_rule(driver):
    assert driver("submit 1\n") == ["ok"] and "codec" in driver("submit 0\n")[0]
