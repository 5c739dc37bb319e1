"""[EXT] volume without a GPU: the four facts the definition rests on (include/q3tts_spec.h "volume") on its numpy restatement at float64 and
f32, q3tts_volume_gain against numpy over every volume, the fixed tree against the plain window sum, that the f32 twin stays inside the
error bounds on the GPU tests' signals, the declarations and the calls that need no engine, and the host rules (csrc/sched_logic.h,
csrc/volume.h) through a plain g++ driver under the host sanitizers."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import volume_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("q3tts_engine_set_volume", "q3tts_request_volume", "q3tts_engine_volume_stats", "q3tts_group_set_volume", "q3tts_group_request_volume",
         "q3tts_volume_gain", "q3tts_op_volume")


@pytest.fixture(scope="module")
def speech():
    x = R.speech_like(9)
    x.setflags(write=False)
    return x


# -------------------------------------------------------- the four facts --------------------------------------------------------
@pytest.mark.parametrize("db10,sig", [(-60, "speech"), (-400, "speech"), (-1, "speech"), (60, "quiet")])
def test_fact_1_where_nothing_exceeds_one_the_output_is_the_delayed_product(speech, db10, sig):
    x = speech if sig == "speech" else R.quiet(9)
    v = R.scaled(x, db10)
    assert np.abs(v).max() <= 1.0 and np.abs(v).max() > 0.0
    want = np.concatenate([np.zeros(R.DELAY, np.float32), v[:-R.DELAY]])
    y32, g32 = R.volume32(v)
    y64, g64, _ = R.volume64(v)
    assert np.all(g32 == 1.0) and np.all(g64 == 1.0)                       # 128 ones sum exactly
    assert np.array_equal(y32.view(np.uint32), want.view(np.uint32)) and np.array_equal(y64, want.astype(np.float64))


@pytest.mark.parametrize("db10", (120, 200))
def test_fact_2_the_limited_product_never_exceeds_one_but_for_rounding(speech, db10):
    v = R.scaled(speech, db10)
    y, g, p = R.volume64(v)
    assert np.abs(v).max() > 2.0 and g.min() < 0.5                         # the limiter is at work
    assert np.abs(p).max() <= 1.0 + 1e-14 and np.abs(y).max() <= 1.0
    assert np.all(g > 0.0) and np.all(g <= 1.0)


def test_fact_3_the_output_depends_on_the_stream_alone(speech):
    """a prefix of the stream gives a prefix of the output: nothing later than sample n reaches y[n]"""
    v = R.scaled(speech, 120)
    y, g = R.volume32(v)
    for cut in (1, 126, 127, 128, 637, 638, 1920, 3 * 1920 + 5):
        yc, gc = R.volume32(v[:cut])
        assert np.array_equal(yc.view(np.uint32), y[:cut].view(np.uint32)) and np.array_equal(gc.view(np.uint32), g[:cut].view(np.uint32)), cut


def test_fact_4_the_impulse():
    x = np.zeros(3 * R.FRAME, np.float32)
    x[1000] = 1.0
    v = R.scaled(x, 200)
    assert R.gain(200) == np.float32(10.0) and v[1000] == np.float32(10.0)
    for y, g in (R.volume64(v)[:2], R.volume32(v)):
        below = np.nonzero(g < 1.0)[0]
        assert below[0] == 1000 and below[-1] == 1638 and below.size == 639     # g < 1 exactly on [1000, 1638]
        tenth = 0.1 if g.dtype == np.float64 else float(np.float32(0.1))
        assert np.all(np.abs(g[1127:1512].astype(np.float64) - tenth) <= 8 * R.U * 0.1)   # g = 0.1 on [1127, 1511]
        assert np.all(g[1000:1127] > g[1001:1128]) and np.all(g[1511:1638] < g[1512:1639])   # the ramps around it
        assert abs(float(y[1127]) - 1.0) <= float(R.y_bound(1.0))
        assert np.count_nonzero(y) == 1


# -------------------------------------------------------- the gain, the tree, the bound --------------------------------------------------------
def test_the_gain_of_every_volume(q3):
    got = np.array([q3.volume_gain(d) for d in range(R.VOL_MIN, R.VOL_MAX + 1)], np.float32)
    want = np.array([R.gain(d) for d in range(R.VOL_MIN, R.VOL_MAX + 1)], np.float32)
    assert got.size == 601 and got.dtype == np.float32
    assert np.all(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1)   # within 1 f32 ulp of numpy
    assert q3.volume_gain(0) == np.float32(1.0) and q3.volume_gain(200) == np.float32(10.0)
    assert q3.volume_gain(-400) == np.float32(0.01) and np.all(np.diff(got) > 0)
    for bad in (-401, 201, 1000, -(2 ** 31)):
        assert np.isnan(q3.volume_gain(bad))


@pytest.mark.parametrize("db10", (120, 200))
def test_tree_and_plain_window_sums_agree_in_float64(speech, db10):
    v = R.scaled(speech, db10)
    _, g_tree, _ = R.volume64(v, tree=True)
    _, g_plain, _ = R.volume64(v, tree=False)
    assert np.abs(g_tree - g_plain).max() <= 128 * 2.0 ** -53


SIGNALS = {"speech +12": lambda: R.scaled(R.speech_like(9), 120), "speech +20": lambda: R.scaled(R.speech_like(9), 200),
           "speech -6": lambda: R.scaled(R.speech_like(9), -60), "quiet +6": lambda: R.scaled(R.quiet(9), 60)}


@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_the_f32_twin_stays_inside_the_bound_on_the_gpu_tests_signals(name):
    v = SIGNALS[name]()
    y64, g64, _ = R.volume64(v)
    y32, g32 = R.volume32(v)
    ey = np.abs(y32.astype(np.float64) - y64) / R.y_bound(y64)
    eg = np.abs(g32.astype(np.float64) - g64) / R.g_bound(g64)
    print("%s: limited share %.3f, y error %.3f of its bound, g error %.3f of its bound" % (name, R.limited_share(v), ey.max(), eg.max()))
    assert ey.max() <= 1.0 and eg.max() <= 1.0


def test_the_speech_like_signal_engages_the_limiter_as_described():
    x = R.speech_like(9)
    assert x.size == 9 * 1920 and 0.85 <= np.abs(x).max() <= 1.0
    s12, s20 = R.limited_share(R.scaled(x, 120)), R.limited_share(R.scaled(x, 200))
    print("limited share: +12 dB %.3f, +20 dB %.3f" % (s12, s20))
    assert 0.4 <= s12 <= 0.7 and 0.65 <= s20 <= 0.9 and s12 < s20          # partly limited, partly passed through, at both


# -------------------------------------------------------- declarations, no engine --------------------------------------------------------
def test_declarations_and_constants(q3):
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in q3.SYMBOLS and hasattr(q3.lib(), name), name
    for name, val in (("Q3_VOL_MIN", -400), ("Q3_VOL_MAX", 200), ("Q3_VOL_LOOK", 128), ("Q3_VOL_HOLD", 512), ("Q3_VOL_DELAY", 127), ("Q3_VOL_HIST", 638)):
        assert "#define %s %d" % (name, val) in spec, name
    assert (q3.VOL_MIN, q3.VOL_MAX, q3.VOL_LOOK, q3.VOL_HOLD, q3.VOL_DELAY, q3.VOL_HIST) == (R.VOL_MIN, R.VOL_MAX, R.LOOK, R.HOLD, R.DELAY, R.HIST)
    assert R.HIST == R.HOLD - 1 + R.DELAY and R.DELAY == R.LOOK - 1


def test_calls_without_an_engine_fail_cleanly(q3):
    L = q3.lib()
    v, a, b = C.c_int32(77), C.c_int64(5), C.c_int64(6)
    assert L.q3tts_engine_set_volume(None, 60) < 0 and b"null" in L.q3tts_last_error()
    assert L.q3tts_request_volume(None, 1, C.byref(v)) < 0 and v.value == 77
    assert L.q3tts_engine_volume_stats(None, C.byref(a), C.byref(b)) < 0 and (a.value, b.value) == (5, 6)
    assert L.q3tts_group_set_volume(None, 60) < 0 and L.q3tts_group_request_volume(None, 1, C.byref(v)) < 0 and v.value == 77


# -------------------------------------------------------- the host rules under the sanitizers --------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("volume_logic") / "volume_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "volume_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_range_and_gain_under_the_sanitizers(driver, q3):
    vals = list(range(R.VOL_MIN, R.VOL_MAX + 1))
    bits = np.array([int(s, 16) for s in driver("".join("gain %d\n" % d for d in vals))], np.uint32)
    assert np.array_equal(bits, np.array([q3.volume_gain(d) for d in vals], np.float32).view(np.uint32))
    assert all(np.isnan(np.array([int(s, 16)], np.uint32).view(np.float32)[0]) for s in driver("gain -401\ngain 201\n"))
    assert driver("volume -400\nvolume 0\nvolume 200\n") == ["ok"] * 3
    assert all("volume out of range" in s for s in driver("volume -401\nvolume 201\nvolume 100000\n"))


def test_launch_check(driver):
    ok = "launch 3 3 7680 6 0  5 120  0 0  2 -60\n"
    assert driver(ok)[0] == "ok" and driver(ok.replace("7680", "1920"))[0] == "ok"
    for bad in ("7681", "0", "960", "-1920"):
        assert "1920" in driver(ok.replace("7680", bad))[0], bad
    assert "long" in driver(ok.replace("7680", str(1920 * 10000)))[0]
    assert "group" in driver("launch 0 3 1920 6 0\n")[0] and "group" in driver(ok.replace("launch 3 3", "launch 3 2"))[0]
    assert "group" in driver("launch -1 3 1920 6 0\n")[0]
    assert "null" in driver(ok.replace("7680 6 0", "7680 6 1"))[0]
    assert "once" in driver(ok.replace(" 2 -60", " 5 -60"))[0] and "once" in driver(ok.replace(" 0 0 ", " 5 0 "))[0]
    assert "stream out of range" in driver(ok.replace(" 2 -60", " 6 -60"))[0] and "stream out of range" in driver(ok.replace(" 5 120", " -1 120"))[0]
    assert "volume out of range" in driver(ok.replace(" 5 120", " 5 201"))[0] and "volume out of range" in driver(ok.replace(" 2 -60", " 2 -401"))[0]
    assert driver(ok.replace(" 5 120", " 5 200").replace(" 2 -60", " 2 -400"))[0] == "ok"


def test_the_shared_launch_checks_come_in_the_order_each_stage_stated_them(driver):
    """group size, chunk, then stream by stream slot, once, own argument -- 5000 inputs with any number of them failing at once (tests/host/stage_preamble.h)"""
    assert driver("preamble\n") == ["preamble 5000"]


def test_submit_rule(driver):
    assert driver("submit 0 1\nsubmit 120 1\nsubmit -400 1\nsubmit 200 1\n") == ["ok"] * 4
    assert all("volume out of range" in s for s in driver("submit 201 1\nsubmit -401 1\n"))
    assert all("codec" in s for s in driver("submit 60 0\nsubmit 0 0\nsubmit 201 0\n"))
