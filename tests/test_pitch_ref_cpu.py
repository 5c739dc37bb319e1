"""[EXT] pitch without a GPU: the counts against their closed forms and the library's, the reach proof by brute force over every allowed pair,
the library's 151 tap tables against the numpy restatement bit for bit, the identity at pitch 100, that the GPU tests' signals leave no frame
undecided in float64 at the pairs those tests use, stage 2 alone on a tone, and the host rules (csrc/sched_logic.h, csrc/pitch.h) through a
plain g++ driver under the host sanitizers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pitch_ref as R
import tsm_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = (50, 51, 80, 99, 100, 101, 125, 199, 200)
NS = (0, 1, 1199, 1200, 1920, 7680, 46080)


def closed(Rt, P, N, final):
    """the closed forms of q3tts_spec.h "pitch": (frames, delivered samples)"""
    L, M, _, _ = R.plan(P)
    f = -(-P * N // (480 * Rt)) if final else (0 if N < 1200 else (P * (N - 1199) - 1) // (480 * Rt) + 1)
    return f, -(-480 * f * L // M)


@pytest.mark.parametrize("Rt", VALUES)
def test_counts_match_the_closed_forms(q3, Rt):
    for P in VALUES:
        for N in NS:
            for final in (False, True):
                got = q3.pitch_samples(Rt, P, N, final)
                if not R.pair_ok(Rt, P):
                    assert got < 0, (Rt, P)
                    continue
                f, n = closed(Rt, P, N, final)
                assert R.n_frames(Rt, P, N, final) == f == q3.pitch_frames(Rt, P, N, final), (Rt, P, N, final)
                assert R.n_samples(Rt, P, N, final) == n == got, (Rt, P, N, final)
                if P == 100:
                    assert f * 480 == q3.tsm_samples(Rt, N, final)   # stage 1 at pitch 100 is the speaking rate's


def test_values_and_pairs_out_of_range_have_no_count(q3):
    for Rt, P in ((49, 100), (100, 49), (201, 200), (100, 201), (50, 101), (200, 99), (99, 199), (101, 50), (0, 0), (-100, 100)):
        assert not R.pair_ok(Rt, P)
        assert q3.pitch_samples(Rt, P, 1920, False) < 0 and q3.pitch_samples(Rt, P, 1920, True) < 0, (Rt, P)
    assert q3.pitch_samples(100, 107, -1, False) < 0
    for Rt, P in ((50, 100), (100, 50), (100, 200), (200, 100), (50, 50), (200, 200), (100, 199), (77, 131)):
        assert R.pair_ok(Rt, P) and q3.pitch_samples(Rt, P, 0, True) == 0


def test_reach_of_every_allowed_pair_stays_inside_the_window():
    """q3tts_spec.h "pitch", reach: with d at either extreme the template and the candidates of frame k stay inside [a_k - 720, a_k + 1200)"""
    pairs = [(Rt, P) for Rt in range(50, 201) for P in range(50, 201) if R.pair_ok(Rt, P)]
    assert len(pairs) > 15000
    k = np.arange(1, 400, dtype=np.int64)
    worst_lo, worst_hi = 0, 0
    for Rt, P in pairs:
        a1, a0 = (k * 480 * Rt) // P, ((k - 1) * 480 * Rt) // P
        step = a1 - a0
        assert step.min() >= 240 and step.max() <= 960, (Rt, P)
        lo = (a0 - 240 + 480 - a1).min()           # t_k - a_k at d = -240
        hi = (a0 + 240 + 480 + 480 - a1).max()     # t_k + 480 - a_k at d = +240
        assert lo >= -720 and hi <= 1200, (Rt, P, lo, hi)
        worst_lo, worst_hi = min(worst_lo, lo), max(worst_hi, hi)
    assert worst_lo == -720 and 240 + 960 <= 1200   # the bound is met (tempo 2), and a candidate's two windows end at a_k + 1200
    assert R.reach(200, 100)[0] == -720 and R.reach(50, 100)[1] <= 1200 and R.reach(100, 199)[0] >= -720


@pytest.mark.parametrize("lo", range(50, 201, 19))
def test_tables_equal_the_numpy_restatement_bit_for_bit(q3, lo):
    for P in range(lo, min(lo + 19, 201)):
        pl = q3.pitch_plan(P)
        assert (pl["L"], pl["M"], pl["n_taps"], pl["taps_per_output"]) == R.plan(P)
        assert 2 * R.Z * max(pl["L"], pl["M"]) // pl["L"] <= R.ZHIST and 33 <= pl["taps_per_output"] <= 65
        lib = q3.pitch_filter(P)
        assert lib.dtype == np.float32 and np.array_equal(lib.view(np.uint32), R.table(P).view(np.uint32)), P


def test_table_sizes_and_the_two_shared_with_the_output_formats(q3):
    sizes = [q3.pitch_plan(P)["n_taps"] for P in range(50, 201)]
    assert sum(sizes) == 366999 and max(sizes) == 6369 == q3.pitch_plan(199)["n_taps"]
    assert np.array_equal(q3.pitch_filter(50).view(np.uint32), q3.pcm_out_filter(48000).view(np.uint32))   # L / M = 2 / 1
    assert np.array_equal(q3.pitch_filter(200).view(np.uint32), q3.pcm_out_filter(12000).view(np.uint32))  # L / M = 1 / 2
    L = q3.lib()
    for P in (49, 201, 0, -100):
        assert L.q3tts_pitch_plan(P, None, None, None, None) < 0 and L.q3tts_pitch_filter(P, None, 0) < 0
    h = np.zeros(64, np.float32)
    assert L.q3tts_pitch_filter(50, h.ctypes.data, 64) < 0 and not h.any()   # 65 taps do not fit


def test_pitch_100_is_the_speaking_rate():
    x = T.speech_like(4, 3)
    for Rt in (80, 125):
        z, d, bz = R.stretch(x, Rt, 100, final=True)
        y, d0, b0 = T.stretch(x, Rt, final=True)
        assert np.array_equal(z, y) and np.array_equal(d, d0) and np.array_equal(bz, b0)
        assert all(R.a_of(Rt, 100, k) == T.a_of(Rt, k) for k in range(50))


@pytest.mark.parametrize("kind", ("speech", "noise"))
def test_the_gpu_tests_signals_have_no_undecided_frame(kind):
    x = T.speech_like(12) if kind == "speech" else T.noise(9)
    for Rt, P in R.GPU_PAIRS:
        z, d, _ = R.stretch(x, Rt, P)
        res = R.decisions(x, Rt, P, d)
        assert 17 <= len(res) <= 92
        assert all(ok for ok, dec, ref in res) and all(ref == dk for (ok, dec, ref), dk in zip(res, d))
        assert sum(not dec for ok, dec, ref in res) == 0, (kind, Rt, P)


@pytest.mark.parametrize("P", (50, 89, 107, 137, 199, 200))
def test_stage_two_alone_moves_a_tone(P):
    """a 1 kHz sine through the resampler (f32 taps, float64 sums) is the delayed sine at 1000 P / 100 Hz within 1.2e-5 of full scale times
    its amplitude 0.5 (the stop band is below -90 dB and the pass band ripple below 4e-5)"""
    L, M, N, _ = R.plan(P)
    z = 0.5 * np.sin(2 * np.pi * 1000.0 * np.arange(4800) / 24000.0)
    y, _ = R.resample(z, P)
    n = np.arange(y.size)
    ideal = 0.5 * np.sin(2 * np.pi * 1000.0 * (n * M / L - R.Z * max(L, M) / L) / 24000.0)
    skip = 2 * R.ZHIST * L // M + 2                 # samples whose taps reach below z[0]
    assert np.abs(y - ideal)[skip:].max() <= 1.2e-5


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("pitch_logic") / "pitch_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "pitch_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_counts_plans_and_tables_under_the_sanitizers(driver, q3):
    cases = [(a, b, n, f) for a in VALUES for b in VALUES for n in NS for f in (0, 1)]
    out = driver("".join("samples %d %d %d %d\n" % c for c in cases))
    for (a, b, n, f), line in zip(cases, out):
        want = list(closed(a, b, n, bool(f))) if R.pair_ok(a, b) else [-1, -1]
        assert [int(v) for v in line.split()] == want, (a, b, n, f)
    assert driver("samples 100 107 -5 0\n") == ["-1 -1"]
    assert driver("pitch 50\npitch 200\npitch 100\n") == ["ok"] * 3 and all("range" in s for s in driver("pitch 49\npitch 201\npitch 0\n"))
    assert driver("pair 50 100\npair 100 50\npair 200 100\npair 100 200\npair 77 131\n") == ["ok"] * 5
    assert all("1/2, 2" in s for s in driver("pair 50 101\npair 200 99\npair 101 50\n"))
    assert "rate" in driver("pair 49 60\n")[0] and "pitch" in driver("pair 100 201\n")[0]
    for P in (50, 51, 100, 137, 199, 200):
        assert tuple(int(v) for v in driver("plan %d\n" % P)[0].split()) == R.plan(P)
        bits = np.array([int(v, 16) for v in driver("filter %d\n" % P)[0].split()], np.uint32)
        assert np.array_equal(bits, q3.pitch_filter(P).view(np.uint32))
    assert driver("plan 49\nplan 201\n") == ["none"] * 2 and driver("filter 201\n") == [""]
    floats, taps, off200, end = (int(v) for v in driver("tables\n")[0].split())
    assert taps == 366999 and floats % 4 == 0 and off200 % 4 == 0 and end <= floats < taps + 4 * 151


def test_launch_check(driver):
    ok = "launch 3 3 7680 0 6  5 100 50 1  0 125 100 0  2 150 75 0\n"
    assert driver(ok)[0] == "ok"
    assert driver(ok.replace("7680 0", "7680 1"))[0] == "ok" and driver(ok.replace("7680 0", "0 1"))[0] == "ok"   # a flush, with or without input
    for bad in ("7681", "0", "960", "-1920"):
        assert "1920" in driver(ok.replace("7680", bad))[0], bad
    assert "long" in driver(ok.replace("7680", str(1920 * 10000)))[0]
    assert "group" in driver("launch 0 3 1920 0 6\n")[0] and "group" in driver(ok.replace("launch 3 3", "launch 3 2"))[0]
    assert "once" in driver(ok.replace(" 2 150 75 0", " 5 150 75 0"))[0]
    assert "range" in driver(ok.replace(" 2 150 75 0", " 6 150 75 0"))[0] and "range" in driver(ok.replace(" 5 100 50 1", " -1 100 50 1"))[0]
    assert "pitch out of range" in driver(ok.replace(" 5 100 50 1", " 5 100 49 1"))[0] and "pitch out of range" in driver(ok.replace(" 2 150 75 0", " 2 150 201 0"))[0]
    assert "rate out of range" in driver(ok.replace(" 0 125 100 0", " 0 201 100 0"))[0]
    assert "1/2, 2" in driver(ok.replace(" 2 150 75 0", " 2 151 75 0"))[0] and "1/2, 2" in driver(ok.replace(" 5 100 50 1", " 5 50 101 1"))[0]
    assert "encoding" in driver(ok.replace(" 5 100 50 1", " 5 100 50 2"))[0] and "encoding" in driver(ok.replace(" 2 150 75 0", " 2 150 75 -1"))[0]


def test_the_shared_launch_checks_come_in_the_order_each_stage_stated_them(driver):
    """group size, chunk, then stream by stream slot, once, own argument -- 5000 inputs with any number of them failing at once (tests/host/stage_preamble.h)"""
    assert driver("preamble\n") == ["preamble 5000"]


def test_submit_rule(driver):
    cap = 24 * 1920 * 4                                                  # an engine of max_steps 24
    assert driver("submit 100 100 16000 1 24 %d 1\n" % cap)[0] == "ok"   # both off: any format, any length
    assert driver("submit 100 107 24000 0 23 %d 1\n" % cap)[0] == "ok" and driver("submit 125 80 24000 1 24 %d 1\n" % cap)[0] == "ok"
    # the flushed last hop ends past the native length (103 hops of z make 46206 samples, 24 frames are 46080): f32 at rate 100 needs a frame to spare
    assert "staging" in driver("submit 100 107 24000 0 24 %d 1\n" % cap)[0] and driver("submit 100 107 24000 1 24 %d 1\n" % cap)[0] == "ok"
    assert "24000" in driver("submit 100 107 16000 1 8 %d 1\n" % cap)[0] and "24000" in driver("submit 125 80 48000 1 8 %d 1\n" % cap)[0]
    assert "encoding" in driver("submit 100 80 24000 2 8 %d 1\n" % cap)[0]
    assert "range" in driver("submit 100 49 24000 0 8 %d 1\n" % cap)[0] and "range" in driver("submit 201 200 24000 0 8 %d 1\n" % cap)[0]
    assert "1/2, 2" in driver("submit 50 101 24000 0 8 %d 1\n" % cap)[0] and "1/2, 2" in driver("submit 200 99 24000 0 8 %d 1\n" % cap)[0]
    assert "codec" in driver("submit 100 80 24000 0 8 %d 0\n" % cap)[0]
    # the duration is the rate's: f32 at rate 50 fits up to half the engine's max_steps whatever the pitch, s16 up to all of it
    assert driver("submit 50 50 24000 0 11 %d 1\n" % cap)[0] == "ok" and "staging" in driver("submit 50 50 24000 0 24 %d 1\n" % cap)[0]
    assert driver("submit 50 50 24000 1 23 %d 1\n" % cap)[0] == "ok"
    # a rate alone keeps the speaking rate's rule
    assert driver("submit 50 100 24000 0 12 %d 1\n" % cap)[0] == "ok" and "staging" in driver("submit 50 100 24000 0 13 %d 1\n" % cap)[0]
    for Rt, P in ((50, 50), (50, 100), (77, 131), (100, 199), (100, 50), (200, 199)):
        for ms in (1, 7, 12, 13, 24):
            fits = closed(Rt, P, ms * 1920, True)[1] * 4 <= cap
            assert (driver("submit %d %d 24000 0 %d %d 1\n" % (Rt, P, ms, cap))[0] == "ok") == fits, (Rt, P, ms)
