"""[EXT] reference audio intake without a GPU: the library's plan, sample count and filter table against tests/intake_ref.py, the restatement
against scipy's polyphase resampler and on tones, the clip check case by case, and the host rules of csrc/intake.h -- the WAV header reader
above all -- through a plain g++ driver under the host sanitizers, like the other rule drivers."""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import intake_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NON_NATIVE = [r for r in R.RATES if r != R.NATIVE]
# the attenuation intake_ref gives an 18 kHz tone in a 48 kHz clip (it would alias to 6 kHz): recorded in profiles/intake_cost.md
ALIAS_18K_DB = 108.5


@pytest.mark.parametrize("rate", R.RATES)
def test_plan_count_and_table_match_the_restatement(q3, rate):
    L, M, N, taps = R.plan(rate)
    assert q3.intake_plan(rate) == (L, M, N, taps) and L * rate == M * R.NATIVE and max(L, M) <= R.MAX_F
    lib, ref = q3.intake_filter(rate), R.table(rate).astype(np.float32)
    assert lib.shape == ref.shape == (N,)
    # two double-precision libms may round a tap differently: one f32 ulp, nothing larger
    ulps = np.abs(lib.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert np.all(np.sign(lib) == np.sign(ref)) and (ulps.size == 0 or ulps.max() <= 1), ulps.max()
    for n in (1, 2, M, M + 1, 1000, 44100, 1234567):
        assert q3.intake_samples(rate, n) == R.n_out(rate, n) == -(-n * R.NATIVE // rate)
    tile = q3.intake_tile(rate)
    assert tile in (64, 128, 256, 512, 1024)
    if N:   # table, a full tile's window and the tile fit the kernel's 64 KB
        stride = -(-taps // 4) * 4
        assert L * stride + (-(-(tile - 1) * M // L) + stride + 1 + 3) // 4 * 4 + tile <= 16384 - 16
        assert L * stride <= 320 * 36


def test_rates_outside_the_rule_are_refused(q3):
    L = q3.lib()
    for rate in (0, -8000, 7999, 192001, 24001, 44101, 11024, 191400 + 1):
        assert not R.accepted(rate)
        assert L.q3tts_intake_plan(rate, None, None, None, None) < 0 and L.q3tts_last_error()
        assert L.q3tts_intake_samples(rate, 100) < 0 and L.q3tts_intake_filter(rate, None, 0) < 0 and L.q3tts_intake_tile(rate) < 0
    for rate in (191400, 9600, 37800, 24000 * 319 // 320):   # unusual rates inside the rule
        assert R.accepted(rate) and q3.intake_plan(rate) == R.plan(rate) and q3.intake_tile(rate) >= 64
    assert L.q3tts_intake_plan(8000, None, None, None, None) == 0
    h = np.zeros(96, np.float32)
    assert L.q3tts_intake_filter(8000, h.ctypes.data, 96) < 0 and not h.any()   # 97 taps do not fit
    assert L.q3tts_intake_filter(24000, None, 0) == 0 and L.q3tts_intake_samples(8000, -1) < 0


@pytest.mark.parametrize("rate", NON_NATIVE)
def test_restatement_equals_scipy_resample_poly(rate):
    from scipy import signal
    L, M, N, taps = R.plan(rate)
    rng = np.random.default_rng(rate)
    h32 = R.table(rate).astype(np.float32)
    for n in (1, 7, 2 * M + 1, 4001):
        x = rng.uniform(-1.0, 1.0, n).astype(np.float32)
        y, bound = R.resample(x, rate)
        want = signal.resample_poly(x.astype(np.float64), L, M, window=h32.astype(np.float64) / L)
        assert y.size == want.size == R.n_out(rate, n) == -(-n * L // M)
        assert np.abs(y - want).max() <= 1e-12
        assert np.all(bound >= 0) and bound.max() <= (taps + 2) * 2.0 ** -24 * 2.2   # per-phase sum |h| stays below 2


@pytest.mark.parametrize("rate", R.RATES)
def test_a_1_khz_tone_comes_out_as_the_24_khz_tone(rate):
    """zero phase: no delay to subtract.  This pins the definition, not the kernel"""
    n = rate * 50 // 1000                                                 # 50 ms
    x = np.sin(2 * np.pi * 1000.0 * np.arange(n) / rate).astype(np.float32)
    y, _ = R.resample(x, rate)
    assert y.size == 1200
    want = np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / 24000.0)
    err = np.abs(y - want)[240:-240].max()                                # 10 ms in from both ends
    print("1 kHz at %d Hz: max error %.3g" % (rate, err))
    assert err <= 1e-4                                                    # the issue's cap; 2.2e-5 at worst, at 11025 Hz


def test_an_18_khz_tone_in_a_48_khz_clip_vanishes():
    n = 4800
    x = np.sin(2 * np.pi * 18000.0 * np.arange(n) / 48000.0).astype(np.float32)
    y, _ = R.resample(x, 48000)
    att = -20 * np.log10(np.abs(y)[240:-240].max())
    print("18 kHz in 48 kHz: attenuation %.1f dB" % att)
    assert att >= ALIAS_18K_DB - 6.0


def test_decode_and_downmix_are_the_spec_arithmetic():
    assert list(R.decode(np.array([0, 128, 255], np.uint8), R.U8, 1)[:, 0]) == [-1.0, 0.0, 127 / 128]
    assert list(R.decode(np.array([-32768, 0, 32767], np.int16), R.S16, 1)[:, 0]) == [-1.0, 0.0, 32767 / 32768]
    assert list(R.decode(R.pack_s24([-(1 << 23), -1, 0, (1 << 23) - 1]), R.S24, 1)[:, 0]) == [-1.0, -1 / 8388608, 0.0, 8388607 / 8388608]
    s32 = R.decode(np.array([-(1 << 31), 1, (1 << 31) - 1], np.int32), R.S32, 1)[:, 0]
    assert s32.dtype == np.float32 and list(s32) == [-1.0, np.float32(2.0 ** -31), 1.0]   # 2^31 - 1 rounds to 2^31 as an f32
    f = np.array([0.25, -3.0, 1e-30], np.float32)
    assert np.array_equal(R.decode(f, R.F32, 1)[:, 0].view(np.uint32), f.view(np.uint32))
    x = np.array([[0.1, 0.2, 0.4]], np.float32)
    assert R.downmix(x, R.FIRST)[0] == x[0, 0]
    assert R.downmix(x, R.MEAN)[0] == np.float32(np.float32(np.float32(x[0, 0] + x[0, 1]) + x[0, 2]) / np.float32(3.0))
    for fmt in (R.U8, R.S16, R.S24, R.F32):   # encode is decode's inverse on the grid of every format an f32 holds exactly
        raw = R.random_raw(np.random.default_rng(fmt), fmt, 64, 2)
        assert np.array_equal(np.asarray(R.encode(R.decode(raw, fmt, 2), fmt)).view(np.uint8), raw.view(np.uint8))


CLIP_CASES = [(r, c, f, m, n) for r in (8000, 44100, 192000, 7999, 24001, 200000) for c in (0, 1, 8, 9) for f in (-1, 0, 4, 5) for m in (-1, 0, 1, 2)
              for n in (0, 1, 100)] + [(r, 1, 1, 0, n) for r in R.RATES for n in (-5, R.MAX_OUT * r // 24000, R.MAX_OUT * r // 24000 + 1, 1 << 40)]


def test_clip_check_case_by_case(q3):
    data = np.zeros(1, np.uint8)
    for rate, ch, fmt, mix, n in CLIP_CASES:
        c = q3.IntakeClip(data.ctypes.data, n, rate, ch, fmt, mix)
        ok = q3.lib().q3tts_intake_check(q3.C.byref(c)) == 0
        why = R.why_not(rate, ch, fmt, mix, n)
        assert ok == (why is None), (rate, ch, fmt, mix, n)
        if why:
            assert why in q3.lib().q3tts_last_error().decode(), (why, q3.lib().q3tts_last_error())
    assert q3.lib().q3tts_intake_check(None) < 0
    c = q3.IntakeClip(None, 10, 48000, 2, 1, 0)
    assert q3.lib().q3tts_intake_check(q3.C.byref(c)) < 0 and "null" in q3.lib().q3tts_last_error().decode()
    assert q3.intake_why_not((np.zeros(8, np.int16), 48000, 2, R.S16, R.MEAN)) is None


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("intake_logic") / "intake_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "intake_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def test_host_plan_and_table_builder_under_the_sanitizers(driver, q3):
    for rate in R.RATES:
        L, M, N, taps = R.plan(rate)
        stride = -(-taps // 4) * 4
        nums = [int(v) for v in driver("plan %d\n" % rate)[0].split()]
        assert nums[:6] == [L, M, N, taps, stride, R.Z * max(L, M) if N else 0] and nums[6] == q3.intake_tile(rate) and nums[7] <= 16384 - 16
        bits = np.array([int(w, 16) for w in driver("filter %d\n" % rate)[0].split()], np.uint32)
        assert np.array_equal(bits, q3.intake_filter(rate).view(np.uint32))
        assert driver("phases %d\n" % rate)[0] == "ok"
        assert [int(driver("samples %d %d\n" % (rate, n))[0]) for n in (0, 1, 999)] == [0, R.n_out(rate, 1), R.n_out(rate, 999)]
    # every ratio the rule admits gets a tile that fits: all L, M <= 320 with a rate in range
    rates = sorted({g * M for g in range(75, 24001) if 24000 % g == 0 for M in range(1, 321) if R.accepted(g * M)})
    assert len(rates) > 1000 and 191400 in rates
    tiles = {}
    for rate, line in zip(rates, driver("".join("plan %d\n" % r for r in rates))):
        nums = [int(v) for v in line.split()]
        assert tuple(nums[:4]) == R.plan(rate) and nums[6] >= 64 and nums[7] <= 16384 - 16, (rate, line)
        tiles[nums[6]] = tiles.get(nums[6], 0) + 1
    assert tiles[1024] > 500 and tiles.get(512, 0) > 0   # most ratios take a full tile; those with a long window beside a large table a smaller one
    assert driver("plan 24001\n")[0].startswith("refused") and driver("plan 7999\n")[0].startswith("refused")
    assert driver("samples 24001 5\n")[0] == "-1" and driver("filter 24001\n")[0] == ""


def test_host_clip_check_under_the_sanitizers(driver):
    out = driver("".join("clip %d %d %d %d %d 1\n" % c for c in CLIP_CASES))
    assert len(out) == len(CLIP_CASES)
    for c, line in zip(CLIP_CASES, out):
        why = R.why_not(*c)
        assert (line == "ok") == (why is None) and (why is None or why in line), (c, line)
    assert "null" in driver("clip 48000 2 1 0 10 0\n")[0] and "null" in driver("clip 48000 2 1 0 10 -1\n")[0]


def _probe(driver, data):
    return driver("wav %s\n" % (bytes(data).hex() or "-"))[0]


def test_wav_probe_reads_every_well_formed_file(driver, q3):
    rng = np.random.default_rng(5)
    for fmt in R.FORMATS:
        for ch, rate, n in ((1, 24000, 10), (2, 44100, 7), (3, 48000, 5), (8, 192000, 3)):
            raw = R.random_raw(rng, fmt, n, ch)
            bits = 8 * R.SAMPLE_BYTES[fmt]
            for kw, off in (({}, 44), ({"extensible": True}, 68), ({"junk": b"abc"}, 56), ({"junk": b"abcd", "extensible": True}, 80)):
                data = R.wav_bytes(raw, fmt, ch, rate, **kw)
                want = "ok %d %d %d %d %d %d" % (fmt, ch, rate, bits, off, n)
                assert _probe(driver, data) == want, (fmt, ch, kw)
                assert data[off: off + raw.size] == bytes(raw)
                w = q3.wav_probe(data)   # and the library's entry point agrees
                assert (w["sample_format"], w["channels"], w["sample_rate"], w["bits"], w["data_offset"], w["n_frames"]) == (fmt, ch, rate, bits, off, n)
    # a data chunk that claims more than the file holds is cut to the file, whole frames only, as the engine's two readers do
    raw = R.random_raw(rng, R.S16, 9, 2)
    assert _probe(driver, R.wav_bytes(raw, R.S16, 2, 48000, declared_len=1 << 20)) == "ok 1 2 48000 16 44 9"
    assert _probe(driver, R.wav_bytes(raw, R.S16, 2, 48000, declared_len=0xFFFFFFFF)[:-3]) == "ok 1 2 48000 16 44 8"
    assert _probe(driver, R.wav_bytes(raw, R.S16, 2, 48000, declared_len=8)) == "ok 1 2 48000 16 44 2"   # and a shorter claim is believed
    assert _probe(driver, R.wav_bytes(raw[:0], R.S16, 2, 48000)) == "ok 1 2 48000 16 44 0"               # no frames: the clip check's business


def _fmt(tag=1, ch=2, rate=48000, bits=16, align=None, length=None, extra=b""):
    align = ch * bits // 8 if align is None else align
    body = struct.pack("<HHIIHH", tag, ch, rate, rate * align & 0xFFFFFFFF, align, bits) + extra
    return b"fmt " + struct.pack("<I", len(body) if length is None else length) + body


def _file(*chunks):
    body = b"".join(chunks)
    return b"RIFF" + struct.pack("<I", 4 + len(body)) + b"WAVE" + body


DATA = b"data" + struct.pack("<I", 8) + bytes(8)
EXT_TAIL = struct.pack("<HHI", 22, 16, 0)
GUID_TAIL = bytes.fromhex("000000001000800000aa00389b71")
MALFORMED = {
    "empty": (b"", "RIFF"),
    "eleven bytes": (b"RIFF\x04\0\0\0WAV", "RIFF"),
    "RIFX": (b"RIFX" + _file(_fmt(), DATA)[4:], "RIFF"),
    "not WAVE": (_file(_fmt(), DATA).replace(b"WAVE", b"AVI "), "RIFF"),
    "header only": (_file(), "no fmt"),
    "data before fmt": (_file(DATA, _fmt()), "before fmt"),
    "no data chunk": (_file(_fmt()), "no data"),
    "fmt of 14 bytes": (_file(_fmt()[:8 + 14].replace(struct.pack("<I", 16), struct.pack("<I", 14)), DATA), "shorter than 16"),
    "fmt claims 16, file ends after 10": (_file(_fmt())[: 12 + 8 + 10], "shorter than 16"),
    "fmt length past the end": (_file(_fmt(length=0xFFFFFFF0))[: 12 + 8 + 12], "shorter than 16"),
    "other chunk's length past the end": (_file(_fmt(), b"LIST" + struct.pack("<I", 1 << 30) + b"abcd", DATA), "no data"),
    "zero channels": (_file(_fmt(ch=0), DATA), "zero channels"),
    "12 bit": (_file(_fmt(bits=12, align=4), DATA), "sample width"),
    "64 bit float": (_file(_fmt(tag=3, bits=64), DATA), "sample width"),
    "16 bit float": (_file(_fmt(tag=3, bits=16), DATA), "sample width"),
    "block align contradicts": (_file(_fmt(ch=2, bits=16, align=2), DATA), "block align"),
    "zero rate": (_file(_fmt(rate=0), DATA), "sample rate"),
    "ADPCM": (_file(_fmt(tag=2), DATA), "format tag"),
    "A-law": (_file(_fmt(tag=6, bits=8), DATA), "format tag"),
    "mu-law": (_file(_fmt(tag=7, bits=8), DATA), "format tag"),
    "extensible of 24 bytes": (_file(_fmt(tag=0xFFFE, extra=EXT_TAIL), DATA), "shorter than 40"),
    "extensible sub-format 2": (_file(_fmt(tag=0xFFFE, extra=EXT_TAIL + struct.pack("<H", 2) + GUID_TAIL), DATA), "format tag"),
    "two fmt chunks": (_file(_fmt(), _fmt(), DATA), "second fmt"),
}


@pytest.mark.parametrize("name", sorted(MALFORMED))
def test_wav_probe_refuses_a_malformed_header(driver, q3, name):
    data, word = MALFORMED[name]
    line = _probe(driver, data)
    assert line.startswith("error: ") and word in line, line
    with pytest.raises(q3.Q3Error, match="WAV error"):
        q3.wav_probe(data)


def test_wav_probe_truncated_at_every_header_byte(driver):
    """a well-formed file cut anywhere in front of its first sample is an error text, never a read past the buffer"""
    for kw, hdr in (({}, 44), ({"extensible": True}, 68), ({"junk": b"xyz"}, 56)):
        data = R.wav_bytes(np.arange(8, dtype=np.int16), R.S16, 2, 44100, **kw)
        out = driver("".join("wav %s\n" % (data[:cut].hex() or "-") for cut in range(hdr)))
        assert len(out) == hdr and all(line.startswith("error: ") for line in out), [l for l in out if not l.startswith("error: ")]
        assert _probe(driver, data[:hdr]) == "ok 1 2 44100 16 %d 0" % hdr
