"""[EXT] output formats without a GPU: the library's plan and filter table against tests/pcm_out_ref.py, the filter's properties asserted on the
library's own table, the reference's two forms against each other and on tones, and the host rules (csrc/sched_logic.h, csrc/pcm_out.h)
through a plain g++ driver under the host sanitizers, like the other rule drivers."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pcm_out_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NON_NATIVE = [r for r in R.RATES if r != R.NATIVE]


@pytest.mark.parametrize("rate", R.RATES)
def test_plan_and_table_match_the_reference(q3, rate):
    assert q3.pcm_out_plan(rate) == R.plan(rate)
    lib, ref = q3.pcm_out_filter(rate), R.table(rate).astype(np.float32)
    assert lib.shape == ref.shape
    # two double-precision libms may round a tap differently: one f32 ulp, nothing larger
    ulps = np.abs(lib.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert np.all(np.sign(lib) == np.sign(ref)) and (ulps.size == 0 or ulps.max() <= 1), ulps.max()
    assert q3.pcm_out_samples(rate, 1920) == 1920 * R.plan(rate)[0] // R.plan(rate)[1] == R.n_out(rate, 1920)
    assert (1920 * R.plan(rate)[0]) % R.plan(rate)[1] == 0   # a frame is a whole number of output samples


def test_unknown_rates_and_small_buffers_are_refused(q3):
    L = q3.lib()
    for rate in (0, 11025, 24001, -8000, 96000):
        assert L.q3tts_pcm_out_plan(rate, None, None, None, None) < 0 and L.q3tts_last_error()
        assert L.q3tts_pcm_out_samples(rate, 1920) < 0 and L.q3tts_pcm_out_filter(rate, None, 0) < 0
    assert L.q3tts_pcm_out_plan(8000, None, None, None, None) == 0
    h = np.zeros(96, np.float32)
    assert L.q3tts_pcm_out_filter(8000, h.ctypes.data, 96) < 0 and not h.any()   # 97 taps do not fit
    assert L.q3tts_pcm_out_filter(24000, None, 0) == 0
    assert L.q3tts_pcm_out_samples(8000, -1) < 0
    assert L.q3tts_pcm_format_check(None) < 0
    for rate in R.RATES + (11025,):
        for enc in (0, 1, 2, -1):
            assert q3.pcm_format_ok(rate, enc) == R.allowed(rate, enc), (rate, enc)


@pytest.mark.parametrize("rate", NON_NATIVE)
def test_filter_properties_of_the_library_table(q3, rate):
    L, M, N, taps = R.plan(rate)
    h = q3.pcm_out_filter(rate)
    rows = R.phase_rows(h, L)
    assert max(len(r) for r in rows) == taps and 33 <= taps <= 97
    assert max(abs(r.sum() - 1.0) for r in rows) <= 1e-4          # per-phase DC gain (measured <= 3.1e-5)
    assert max(np.abs(r).sum() for r in rows) <= 2.0              # per-phase sum |h| (measured <= 1.962)
    nyq = min(rate, R.NATIVE) / 2.0
    pb = R.response_db(h, L, np.linspace(0.0, 0.8 * nyq, 801))
    assert pb.max() <= 0.001 and pb.min() >= -0.4                 # measured +0.0003 / -0.3752 dB
    sb = R.response_db(h, L, np.linspace(1.1 * nyq, R.NATIVE * L / 2.0, 4001))
    assert sb.max() <= -85.0                                      # measured <= -90.1 dB
    assert h.size == N and np.array_equal(h, h[::-1])             # linear phase: the delay is exactly Z F / L native samples
    assert R.delay_native(rate) == {8000: 48, 12000: 32, 16000: 24, 32000: 16, 44100: 16, 48000: 16}.get(rate, 16 * 160 / 147)


def _signal(n_frames, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.0, n_frames * R.FRAME).astype(np.float32)


@pytest.mark.parametrize("rate", R.RATES)
def test_streaming_form_equals_the_whole_signal_form(rate):
    x = _signal(9, rate)
    whole, wb = R.convert(x, rate)
    assert whole.size == R.n_out(rate, x.size)
    for sched in ([9], [4, 4, 1], [1] * 9):
        y, b = R.stream_convert(x, rate, sched)
        assert np.array_equal(y, whole) and np.array_equal(b, wb), sched
    s = R.Stream(rate)   # a reset makes the stream a fresh one
    s.push(x[: 2 * R.FRAME])
    s.reset()
    assert np.array_equal(s.push(x[: R.FRAME])[0], whole[: R.n_out(rate, R.FRAME)])


def test_a_given_table_replaces_the_reference_table(q3):
    x = _signal(2, 5)
    for rate in (16000, 44100):
        own = R.convert(x, rate)[0]
        assert np.array_equal(R.convert(x, rate, R.table(rate).astype(np.float32))[0], own)
        assert np.allclose(R.convert(x, rate, q3.pcm_out_filter(rate))[0], own, atol=1e-6, rtol=0)
        assert not np.array_equal(R.convert(x, rate, np.zeros(R.plan(rate)[2], np.float32))[0], own)


def test_tones_pass_delayed_and_alias_tones_vanish():
    n = np.arange(4 * R.FRAME)
    # 1 kHz to 16 kHz: the tone delayed by 24 native samples, i.e. 16 output samples
    y, _ = R.convert(np.sin(2 * np.pi * 1000.0 * n / 24000.0).astype(np.float32), 16000)
    m = np.arange(y.size)
    want = np.sin(2 * np.pi * 1000.0 * (m / 16000.0 - R.delay_native(16000) / 24000.0))
    err = np.abs(y - want)[200:].max()
    print("1 kHz -> 16 kHz: max error %.3g" % err)
    assert err <= 2e-5                                            # measured 1.0e-5
    # 7 kHz lies above the 4 kHz Nyquist frequency of 8 kHz: -85 dB at the least
    y, _ = R.convert(np.sin(2 * np.pi * 7000.0 * n / 24000.0).astype(np.float32), 8000)
    left = np.abs(y)[200:].max()
    print("7 kHz -> 8 kHz: max residue %.3g" % left)
    assert left <= 5.6e-5                                         # measured 4.3e-7


def test_quantiser_rounds_the_f32_product_to_even():
    y = np.array([0.0, 1.0, -1.0, 0.5, -0.5, 1.5 / 32767.0, 2.5 / 32767.0, 1e-9], np.float32)
    q = R.s16_of(y)
    assert q.dtype == np.int16 and list(q[:5]) == [0, 32767, -32767, 16384, -16384] and q[7] == 0
    assert list(q[5:7]) == [int(np.rint(np.float32(y[5]) * np.float32(32767.0))), int(np.rint(np.float32(y[6]) * np.float32(32767.0)))]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("pcm_out_logic") / "pcm_out_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "pcm_out_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_rules_over_every_format(driver):
    cases = [(r, e, n) for r in R.RATES + (11025, 0) for e in (0, 1, 2) for n in (0, 1, 4, 24, 512)]
    out = driver("".join("rule %d %d 1 0 %d\n" % c for c in cases))
    assert len(out) == len(cases)
    for (rate, enc, n), line in zip(cases, out):
        why, nums = [s.strip() for s in line.split("|")]
        samples, nbytes = [int(v) for v in nums.split()]
        assert (why == "ok") == R.allowed(rate, enc), (rate, enc, line)
        if rate in R.RATES:
            assert samples == R.n_out(rate, n * R.FRAME)
            assert nbytes == samples * (2 if enc == 1 else 4)
            if R.allowed(rate, enc):
                assert nbytes <= 4 * n * R.FRAME                 # the native staging region serves every format
                assert (nbytes == 4 * n * R.FRAME) == ((rate, enc) in ((24000, 0), (48000, 1)) or n == 0)
        else:
            assert samples == -1 and nbytes == -1 and "rate" in why
    assert "encoding" in driver("rule 16000 2 1 0 1\n")[0] and "24000" in driver("rule 32000 0 1 0 1\n")[0]
    assert driver("rule 0 0 1 1 1\n")[0].startswith("ok")        # NULL is the native format
    assert "codec" in driver("rule 16000 1 0 0 1\n")[0] and "codec" in driver("rule 0 0 0 1 1\n")[0]


def test_host_table_builder_under_the_sanitizers(driver, q3):
    for rate in R.RATES:
        L, M, N, taps = R.plan(rate)
        assert driver("plan %d\n" % rate)[0] == "%d %d %d %d %d" % (L, M, N, taps, -(-taps // 4) * 4)
        bits = np.array([int(w, 16) for w in driver("filter %d\n" % rate)[0].split()], np.uint32)
        assert np.array_equal(bits, q3.pcm_out_filter(rate).view(np.uint32))
        assert driver("phases %d\n" % rate)[0] == "ok"
    assert driver("plan 11025\n")[0] == "unknown" and driver("filter 11025\n")[0] == ""


def test_launch_check(driver):
    ok = "launch 3 3 7680 6  5 8000 1  0 24000 0  2 48000 1\n"
    assert driver(ok)[0] == "ok"
    assert "frames" in driver(ok.replace("7680", "7681"))[0] and "frames" in driver(ok.replace("7680", "0"))[0]
    assert "frames" in driver(ok.replace("7680", "960"))[0]
    assert "group" in driver("launch 0 3 1920 6\n")[0] and "group" in driver(ok.replace("launch 3 3", "launch 3 2"))[0]
    assert "once" in driver(ok.replace(" 2 48000 1", " 5 48000 1"))[0]
    assert "range" in driver(ok.replace(" 2 48000 1", " 6 48000 1"))[0] and "range" in driver(ok.replace(" 5 8000 1", " -1 8000 1"))[0]
    assert "24000 Hz only" in driver(ok.replace("48000 1", "48000 0"))[0]
    assert "rate" in driver(ok.replace("8000 1", "11025 1"))[0] and "encoding" in driver(ok.replace("8000 1", "8000 2"))[0]
    assert "long" in driver(ok.replace("7680", str(1920 * 7700)))[0]


def test_the_shared_launch_checks_come_in_the_order_each_stage_stated_them(driver):
    """group size, chunk, then stream by stream slot, once, own argument -- 5000 inputs with any number of them failing at once (tests/host/stage_preamble.h)"""
    assert driver("preamble\n") == ["preamble 5000"]
