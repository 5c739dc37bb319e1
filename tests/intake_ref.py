"""The reference audio intake of include/q3tts_spec.h ("reference audio intake") restated in float64 numpy: the yardstick of
tests/test_intake_ref_cpu.py and tests/test_gpu_intake.py.  TEST INFRASTRUCTURE ONLY.

plan / table build the ratios and the prototype from the spec's formulas with numpy's own sinc and kaiser.  decode and downmix are the spec's
f32 arithmetic (they are exact or correctly rounded operations, so numpy's f32 is the definition itself).  resample sums the exact float64
products of f32 factors in ascending k over its own table or a given f32 one, and returns with every output sample the running-error bound
of an f32 fma chain over the same terms, gamma_n * sum |h_k x_k| with n = taps + 2 and u = 2^-24, as tests/pcm_out_ref.py does.  The helpers
below it make raw clips and WAV files of every sample format for the tests."""
import math
import struct

import numpy as np

RATES = (8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000)
NATIVE, Z, BETA = 24000, 16, 9.0
U8, S16, S24, S32, F32 = 0, 1, 2, 3, 4
FORMATS = (U8, S16, S24, S32, F32)
SAMPLE_BYTES = (1, 2, 3, 4, 4)
FIRST, MEAN = 0, 1
MAX_F, MAX_CH, MAX_OUT, MAX_CLIPS = 320, 8, 2880000, 64
U = 2.0 ** -24


def accepted(rate):
    if not 8000 <= rate <= 192000:
        return False
    g = math.gcd(rate, NATIVE)
    return max(NATIVE // g, rate // g) <= MAX_F


def plan(rate):
    """(L, M, N, taps): 24000 / rate = L / M, N prototype taps, at most `taps` terms per output sample; 24000 has no filter"""
    assert accepted(rate)
    g = math.gcd(rate, NATIVE)
    L, M = NATIVE // g, rate // g
    if rate == NATIVE:
        return 1, 1, 0, 0
    N = 2 * Z * max(L, M) + 1
    return L, M, N, -(-N // L)


def table(rate):
    """the prototype in float64 (round with .astype(np.float32) for h32)"""
    L, M, N, _ = plan(rate)
    if N == 0:
        return np.zeros(0)
    F = max(L, M)
    fc = 0.9 / (2 * F)
    i = np.arange(N, dtype=np.float64)
    return L * 2 * fc * np.sinc(2 * fc * (i - Z * F)) * np.kaiser(N, BETA)


def n_out(rate, n):
    L, M, _, _ = plan(rate)
    return -(-n * L // M)


def why_not(rate, channels, fmt, mix, n):
    """the spec's "accepted" rule: None, or which part refuses"""
    if not accepted(rate):
        return "rate"
    if not 1 <= channels <= MAX_CH:
        return "channel"
    if fmt not in FORMATS:
        return "format"
    if mix not in (FIRST, MEAN):
        return "downmix"
    if n < 1:
        return "empty"
    if n_out(rate, n) > MAX_OUT:
        return "120 s"
    return None


def decode(raw, fmt, channels):
    """raw interleaved bytes -> f32 [n][channels]"""
    b = np.frombuffer(bytes(raw), np.uint8) if isinstance(raw, (bytes, bytearray)) else np.ascontiguousarray(raw).reshape(-1).view(np.uint8)
    n = b.size // (SAMPLE_BYTES[fmt] * channels)
    b = b[: n * SAMPLE_BYTES[fmt] * channels]
    if fmt == U8:
        x = (b.astype(np.int32) - 128).astype(np.float32) / np.float32(128.0)
    elif fmt == S16:
        x = b.view("<i2").astype(np.float32) / np.float32(32768.0)
    elif fmt == S24:
        t = b.reshape(-1, 3).astype(np.int32)
        v = t[:, 0] | (t[:, 1] << 8) | (t[:, 2].astype(np.int8).astype(np.int32) << 16)
        x = v.astype(np.float32) / np.float32(8388608.0)
    elif fmt == S32:
        x = b.view("<i4").astype(np.float32) / np.float32(2147483648.0)
    else:
        x = b.view("<f4").copy()
    return x.reshape(n, channels)


def downmix(x, mix):
    """f32 [n][C] -> f32 [n]"""
    x = np.asarray(x, np.float32)
    if mix == FIRST:
        return x[:, 0].copy()
    acc = x[:, 0].copy()
    for c in range(1, x.shape[1]):
        acc = (acc + x[:, c]).astype(np.float32)
    return (acc / np.float32(x.shape[1])).astype(np.float32)


def _gamma(n):
    return n * U / (1.0 - n * U)


def resample(x, rate, h32=None, m0=0, count=None):
    """outputs m0 .. m0 + count - 1 (default: all) of the mono f32 clip x at `rate`: (y, bound), y in float64; |f32 result - y| <= bound for
    an f32 fma chain over the same terms.  24000: x itself and a bound of zero"""
    x = np.asarray(x, np.float32).astype(np.float64)
    L, M, N, taps = plan(rate)
    total = n_out(rate, x.size)
    count = total - m0 if count is None else count
    assert 0 <= m0 and m0 + count <= total
    if N == 0:
        return x[m0: m0 + count].copy(), np.zeros(count)
    h = (table(rate).astype(np.float32) if h32 is None else np.asarray(h32, np.float32)).astype(np.float64)
    assert h.size == N
    c = Z * max(L, M)
    t = np.arange(m0, m0 + count, dtype=np.int64) * M + c
    p, j = t % L, t // L
    y = np.zeros(count)
    s = np.zeros(count)
    for k in range(taps):
        idx, i = p + k * L, j - k
        hk = np.where(idx < N, h[np.minimum(idx, N - 1)], 0.0)
        xi = np.where((i >= 0) & (i < x.size), x[np.clip(i, 0, x.size - 1)], 0.0)
        term = hk * xi
        y = y + term
        s = s + np.abs(term)
    return y, _gamma(taps + 2) * s


def intake(raw, rate, channels, fmt, mix, h32=None, m0=0, count=None):
    """the whole definition: decode, downmix, resample"""
    return resample(downmix(decode(raw, fmt, channels), mix), rate, h32, m0, count)


# ---- clips and files for the tests ----
def random_raw(rng, fmt, n, channels):
    """n frames of full-scale noise in sample format fmt, as a uint8 array"""
    k = n * channels
    if fmt == U8:
        return rng.integers(0, 256, k, dtype=np.uint8)
    if fmt == S16:
        return rng.integers(-32768, 32768, k, dtype=np.int16).view(np.uint8)
    if fmt == S24:
        return pack_s24(rng.integers(-(1 << 23), 1 << 23, k, dtype=np.int32))
    if fmt == S32:
        return rng.integers(-(1 << 31), 1 << 31, k, dtype=np.int64).astype(np.int32).view(np.uint8)
    return rng.uniform(-1.0, 1.0, k).astype(np.float32).view(np.uint8)


def pack_s24(v):
    v = np.asarray(v, np.int32)
    out = np.empty((v.size, 3), np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = v & 255, (v >> 8) & 255, (v >> 16) & 255
    return out.reshape(-1)


def encode(x, fmt):
    """f32 samples in [-1, 1) -> raw bytes of sample format fmt (u8 and the integer formats quantise)"""
    x = np.asarray(x, np.float64).reshape(-1)
    if fmt == U8:
        return np.clip(np.rint(x * 128.0) + 128, 0, 255).astype(np.uint8)
    if fmt == S16:
        return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16).view(np.uint8)
    if fmt == S24:
        return pack_s24(np.clip(np.rint(x * 8388608.0), -(1 << 23), (1 << 23) - 1).astype(np.int32))
    if fmt == S32:
        return np.clip(np.rint(x * 2147483648.0), -(1 << 31), (1 << 31) - 1).astype(np.int64).astype(np.int32).view(np.uint8)
    return x.astype(np.float32).view(np.uint8)


def wav_bytes(raw, fmt, channels, rate, extensible=False, junk=None, declared_len=None):
    """a RIFF/WAVE file around raw sample bytes; junk: the body of a chunk put between fmt and data (odd lengths are padded)"""
    raw = bytes(np.ascontiguousarray(raw).reshape(-1).view(np.uint8))
    bits = 8 * SAMPLE_BYTES[fmt]
    tag = 3 if fmt == F32 else 1
    align = channels * bits // 8
    body = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, channels, rate, rate * align, align, bits)
    if extensible:
        body += struct.pack("<HHIH", 22, bits, 0, tag) + bytes.fromhex("000000001000800000aa00389b71")
    chunks = b"fmt " + struct.pack("<I", len(body)) + body
    if junk is not None:
        chunks += b"LIST" + struct.pack("<I", len(junk)) + junk + (b"\0" if len(junk) & 1 else b"")
    chunks += b"data" + struct.pack("<I", len(raw) if declared_len is None else declared_len) + raw + (b"\0" if len(raw) & 1 else b"")
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks
