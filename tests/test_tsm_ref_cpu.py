"""[EXT] speaking rate without a GPU: the counts against their closed forms and the library's, the three facts the definition states (rate
100 is the identity, a periodic input continues in phase, silence chooses offset 0), the library's window tables against numpy's, the host
rules (csrc/sched_logic.h, csrc/tsm.h) through a plain g++ driver under the host sanitizers, and that the GPU tests' signals leave no frame
undecided in float64."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import tsm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PCTS = (50, 80, 100, 125, 160, 200)


@pytest.mark.parametrize("pct", PCTS)
def test_counts_match_the_closed_forms(q3, pct):
    for n in (1, 2, 4, 8):
        N = n * 1920
        stream = R.n_samples(pct, N, False)
        assert stream == 480 * ((100 * (N - 1199) - 1) // (480 * pct) + 1) == q3.tsm_samples(pct, N, False)
        final = R.n_samples(pct, N, True)
        assert final == 480 * -(-100 * N // (480 * pct)) == q3.tsm_samples(pct, N, True)
        assert final >= stream
        # a frame is available only when everything it may read has been seen
        k = stream // 480 - 1
        assert R.a_of(pct, k) + R.LOOK <= N < R.a_of(pct, k + 1) + R.LOOK
    assert q3.tsm_samples(pct, 0, False) == 0 == q3.tsm_samples(pct, 0, True) and q3.tsm_samples(pct, 1199, False) == 0
    assert q3.tsm_samples(pct, 1200, False) == 480 and q3.tsm_samples(pct, 1, True) == 480


def test_count_examples():
    assert [R.n_samples(p, 1920, False) for p in PCTS] == [1920, 960, 960, 960, 480, 480]
    assert R.n_samples(80, 1920, True) == 2400


def test_rates_out_of_range_have_no_count(q3):
    for pct in (49, 201, 0, -100):
        assert q3.tsm_samples(pct, 1920, False) < 0 and q3.tsm_samples(pct, 1920, True) < 0
    assert q3.tsm_samples(100, -1, False) < 0


def test_reach_of_a_frame_stays_inside_the_history():
    for pct in range(R.MIN, R.MAX + 1):
        for k in range(1, 40):
            a, a1 = R.a_of(pct, k), R.a_of(pct, k - 1)
            t_lo, t_hi = max(a1 - R.SEARCH, 0) + R.HOP, a1 + R.SEARCH + R.HOP
            assert t_lo >= a - (R.HIST - R.LOOK) and t_hi + R.HOP <= a + R.LOOK and a + R.SEARCH + R.WIN <= a + R.LOOK


def test_rate_100_is_the_identity():
    x = R.speech_like(4, 3)
    y, d, bound = R.stretch(x, 100)
    assert np.all(d == 0) and y.size == R.n_samples(100, x.size, False)
    assert np.all(np.abs(y - x[: y.size].astype(np.float64)) <= 2.0 ** -23 * np.abs(x[: y.size]) + 2.0 ** -149)


@pytest.mark.parametrize("P", (96, 75, 201))
@pytest.mark.parametrize("pct", (50, 75, 125, 150, 200))
def test_a_periodic_input_continues_in_phase(P, pct):
    tab, x = R.periodic(P, 6, 11 + P)
    y, d, bound = R.stretch(x, pct)
    xp = np.concatenate([x.astype(np.float64), np.zeros(4000)])
    p_prev = -R.HOP
    for k, dk in enumerate(d):       # every chosen candidate matches its template exactly
        a, t = R.a_of(pct, k), p_prev + R.HOP
        assert np.array_equal(xp[a + dk: a + dk + R.HOP], xp[t: t + R.HOP]), (k, dk)
        p_prev = a + dk
    want = tab[np.arange(y.size) % P].astype(np.float64)
    assert np.all(np.abs(y - want) <= 2.0 ** -23 * np.abs(want) + 2.0 ** -149)


def test_silence_chooses_offset_zero():
    for pct in (50, 125, 200):
        y, d, bound = R.stretch(np.zeros(4 * 1920, np.float32), pct, final=True)
        assert np.all(d == 0) and np.all(y == 0) and y.size == R.n_samples(pct, 4 * 1920, True)


def test_teacher_forcing_reproduces_the_free_run_and_flush_appends_zeros():
    x = R.noise(3, 5)
    y, d, _ = R.stretch(x, 80, final=True)
    y2, d2, _ = R.stretch(x, 80, final=True, deltas=d)
    assert np.array_equal(y, y2) and np.array_equal(d, d2)
    ys, ds, _ = R.stretch(x, 80)                                   # the streamed part is the head of the flushed whole
    assert np.array_equal(ys, y[: ys.size]) and np.array_equal(ds, d[: ds.size])
    yz, dz, _ = R.stretch(np.concatenate([x, np.zeros(1920, np.float32)]), 80)
    assert yz.size >= y.size and np.array_equal(yz[: y.size], y)   # a flushed tail is the stream with zeros appended


def test_library_windows_equal_numpys(q3):
    w, w2 = q3.tsm_windows()
    rw, rw2 = R.windows()
    for a, b in ((w, rw), (w2, rw2)):
        ulps = np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))
        assert a.dtype == np.float32 and a.shape == (480,) and ulps.max() <= 1, ulps.max()
    assert np.abs(w.astype(np.float64) + w2.astype(np.float64) - 1.0).max() <= 2.0 ** -24
    assert w[0] == 0.0 and w2[0] == 1.0 and np.all(np.diff(w) > 0) and np.all(np.diff(w2) < 0)


@pytest.mark.parametrize("kind", ("speech", "noise"))
def test_the_gpu_tests_signals_have_no_undecided_frame(kind):
    x = R.speech_like(12) if kind == "speech" else R.noise(9)
    for pct in (50, 80, 125, 160, 200):
        y, d, _ = R.stretch(x, pct)
        res = R.decisions(x, pct, d)
        assert all(ok for ok, dec, ref in res) and all(ref == dk for (ok, dec, ref), dk in zip(res, d))
        assert sum(not dec for ok, dec, ref in res) == 0, (kind, pct)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("tsm_logic") / "tsm_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "tsm_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_counts_and_tables_under_the_sanitizers(driver, q3):
    cases = [(p, n, f) for p in (50, 51, 80, 99, 100, 125, 160, 199, 200) for n in (0, 1, 1199, 1200, 1920, 3840, 7680, 15360, 46080) for f in (0, 1)]
    out = driver("".join("samples %d %d %d\n" % c for c in cases))
    for (p, n, f), line in zip(cases, out):
        assert [int(v) for v in line.split()] == [R.n_frames(p, n, bool(f)), R.n_samples(p, n, bool(f))], (p, n, f)
    assert driver("samples 49 1920 0\nsamples 201 1920 1\nsamples 100 -5 0\n") == ["-1 -1"] * 3
    assert driver("rate 50\nrate 200\nrate 100\n") == ["ok"] * 3
    assert all("range" in s for s in driver("rate 49\nrate 201\nrate 0\nrate -50\n"))
    bits = np.array([int(v, 16) for v in driver("windows\n")[0].split()], np.uint32)
    w, w2 = q3.tsm_windows()
    assert np.array_equal(bits[:480], w.view(np.uint32)) and np.array_equal(bits[480:], w2.view(np.uint32))
    assert driver("order\n")[0] == "ok"


def test_launch_check(driver):
    ok = "launch 3 3 7680 0 6  5 50 1  0 100 0  2 200 0\n"
    assert driver(ok)[0] == "ok"
    assert driver(ok.replace("7680 0", "7680 1"))[0] == "ok" and driver(ok.replace("7680 0", "0 1"))[0] == "ok"   # a flush, with or without input
    for bad in ("7681", "0", "960", "-1920"):
        assert "1920" in driver(ok.replace("7680", bad))[0], bad
    assert "long" in driver(ok.replace("7680", str(1920 * 10000)))[0]
    assert "group" in driver("launch 0 3 1920 0 6\n")[0] and "group" in driver(ok.replace("launch 3 3", "launch 3 2"))[0]
    assert "once" in driver(ok.replace(" 2 200 0", " 5 200 0"))[0]
    assert "range" in driver(ok.replace(" 2 200 0", " 6 200 0"))[0] and "range" in driver(ok.replace(" 5 50 1", " -1 50 1"))[0]
    assert "rate" in driver(ok.replace(" 5 50 1", " 5 49 1"))[0] and "rate" in driver(ok.replace(" 2 200 0", " 2 201 0"))[0]
    assert "encoding" in driver(ok.replace(" 5 50 1", " 5 50 2"))[0] and "encoding" in driver(ok.replace(" 2 200 0", " 2 200 -1"))[0]


def test_the_shared_launch_checks_come_in_the_order_each_stage_stated_them(driver):
    """group size, chunk, then stream by stream slot, once, own argument -- 5000 inputs with any number of them failing at once (tests/host/stage_preamble.h)"""
    assert driver("preamble\n") == ["preamble 5000"]


def test_submit_rule(driver):
    cap = 24 * 1920 * 4                                             # an engine of max_steps 24
    assert driver("submit 100 16000 1 24 %d 1\n" % cap)[0] == "ok"   # 100 is off: any format, any length
    assert driver("submit 125 24000 0 24 %d 1\n" % cap)[0] == "ok" and driver("submit 200 24000 1 24 %d 1\n" % cap)[0] == "ok"
    assert "24000" in driver("submit 125 16000 1 8 %d 1\n" % cap)[0] and "24000" in driver("submit 80 48000 1 8 %d 1\n" % cap)[0]
    assert "encoding" in driver("submit 80 24000 2 8 %d 1\n" % cap)[0]
    assert "range" in driver("submit 49 24000 0 8 %d 1\n" % cap)[0] and "range" in driver("submit 201 24000 0 8 %d 1\n" % cap)[0]
    assert "codec" in driver("submit 80 24000 0 8 %d 0\n" % cap)[0]
    # slowing down makes more samples than native: f32 at 50 fits up to half the engine's max_steps, s16 up to all of it
    assert driver("submit 50 24000 0 12 %d 1\n" % cap)[0] == "ok" and "staging" in driver("submit 50 24000 0 13 %d 1\n" % cap)[0]
    assert driver("submit 50 24000 1 24 %d 1\n" % cap)[0] == "ok"
    for pct in range(50, 201, 7):
        for ms in (1, 7, 24):
            fits = R.n_samples(pct, ms * 1920, True) * 4 <= cap
            assert (driver("submit %d 24000 0 %d %d 1\n" % (pct, ms, cap))[0] == "ok") == fits, (pct, ms)
