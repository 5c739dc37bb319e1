"""The output formats of include/q3tts_spec.h ("output formats") restated in float64 numpy: the yardstick of tests/test_gpu_pcm_out.py and
tests/test_gpu_pcm_out_engine.py.  TEST INFRASTRUCTURE ONLY.

plan / table build the ratios and the prototype filter from the spec's formulas with numpy's own sinc and kaiser.  convert is the whole-signal
form (output sample n from the global index arithmetic t = n M), Stream the stateful form (chunk-local indices and 96 samples of history, as a
converter that sees one chunk at a time must work); tests/test_pcm_out_ref_cpu.py holds the two against each other.  Both take their own table
or a given f32 one, sum the exact float64 products of f32 factors in ascending k, and return with every output sample the running-error bound
of an f32 fma chain over the same terms, gamma_n * sum |h_k x_k| with n = taps + 2 and u = 2^-24: `taps` fmas for the sum, and two to spare,
one of which covers the f32 rounding of y * 32767 in front of the int16 conversion (|y| <= sum |h_k x_k|)."""
import math

import numpy as np

RATES = (8000, 12000, 16000, 22050, 24000, 32000, 44100, 48000)
NATIVE, FRAME, Z, BETA, HIST = 24000, 1920, 16, 9.0, 96
F32, S16 = 0, 1
U = 2.0 ** -24


def plan(rate):
    """(L, M, N, taps): rate = 24000 L / M, N prototype taps, at most `taps` terms per output sample; 24000 has no filter"""
    assert rate in RATES
    g = math.gcd(rate, NATIVE)
    L, M = rate // g, NATIVE // g
    if rate == NATIVE:
        return 1, 1, 0, 0
    N = 2 * Z * max(L, M) + 1
    return L, M, N, -(-N // L)


def allowed(rate, enc):
    return rate in RATES and enc in (F32, S16) and (enc == S16 or rate <= NATIVE)


def table(rate):
    """the prototype in float64 (round with .astype(np.float32) for h32)"""
    L, M, N, _ = plan(rate)
    if N == 0:
        return np.zeros(0)
    F = max(L, M)
    fc = 0.9 / (2 * F)
    i = np.arange(N, dtype=np.float64)
    return L * 2 * fc * np.sinc(2 * fc * (i - Z * F)) * np.kaiser(N, BETA)


def delay_native(rate):
    """Z F / L: the delay of the converted stream in native samples"""
    L, M, N, _ = plan(rate)
    return 0.0 if N == 0 else Z * max(L, M) / L


def n_out(rate, n_native):
    L, M, _, _ = plan(rate)
    return n_native * L // M


def _gamma(n):
    return n * U / (1.0 - n * U)


def _sum_terms(h, L, M, N, taps, xpad, pad, n0, count):
    """outputs n0 .. n0 + count - 1 over xpad (x with `pad` samples in front): the float64 sum in ascending k and sum |h_k x_k|"""
    n = np.arange(n0, n0 + count, dtype=np.int64)
    t = n * M
    p, j = t % L, t // L
    y = np.zeros(count)
    s = np.zeros(count)
    for k in range(taps):
        idx = p + k * L
        ok = idx < N
        hk = np.where(ok, h[np.minimum(idx, N - 1)], 0.0)
        term = hk * xpad[j - k + pad]
        y = y + term
        s = s + np.abs(term)
    return y, s


def convert(x, rate, h32=None):
    """the whole-signal form.  x: native samples from the stream's reset on (f32 values).  Returns (y, bound): y in float64, clamped to [-1, 1];
    |f32 result - y| <= bound for an f32 fma chain over the same terms"""
    x = np.asarray(x, np.float32).astype(np.float64)
    L, M, N, taps = plan(rate)
    if N == 0:
        return np.clip(x, -1.0, 1.0), np.zeros(x.size)
    h = (table(rate).astype(np.float32) if h32 is None else np.asarray(h32, np.float32)).astype(np.float64)
    assert h.size == N
    pad = taps
    xpad = np.concatenate([np.zeros(pad), x])   # x[< 0] = 0
    y, s = _sum_terms(h, L, M, N, taps, xpad, pad, 0, x.size * L // M)
    return np.clip(y, -1.0, 1.0), _gamma(taps + 2) * s


class Stream:
    """the stateful form: push(chunk of whole frames) -> (y, bound) of that chunk's output samples; nothing but the last 96 native samples is
    kept between chunks, and no phase (a frame is a whole number of output samples)"""

    def __init__(self, rate, h32=None):
        self.rate = rate
        self.L, self.M, self.N, self.taps = plan(rate)
        if self.N:
            self.h = (table(rate).astype(np.float32) if h32 is None else np.asarray(h32, np.float32)).astype(np.float64)
            assert self.h.size == self.N and self.taps - 1 <= HIST
        self.reset()

    def reset(self):
        self.hist = np.zeros(HIST)

    def push(self, chunk):
        c = np.asarray(chunk, np.float32).astype(np.float64)
        assert c.size >= FRAME and c.size % FRAME == 0
        if self.N == 0:
            return np.clip(c, -1.0, 1.0), np.zeros(c.size)
        xpad = np.concatenate([self.hist, c])
        y, s = _sum_terms(self.h, self.L, self.M, self.N, self.taps, xpad, HIST, 0, c.size * self.L // self.M)
        self.hist = c[-HIST:].copy()
        return np.clip(y, -1.0, 1.0), _gamma(self.taps + 2) * s


def stream_convert(x, rate, chunk_frames, h32=None):
    s = Stream(rate, h32)
    ys, bs, at = [], [], 0
    for f in chunk_frames:
        y, b = s.push(x[at: at + f * FRAME])
        ys.append(y); bs.append(b); at += f * FRAME
    assert at == len(x)
    return np.concatenate(ys), np.concatenate(bs)


def s16_of(y32):
    """(int16) rintf(y * 32767.0f) of f32 values already clamped to [-1, 1]: the product rounded to f32, then ties to even"""
    y32 = np.asarray(y32, np.float32)
    return np.rint(y32 * np.float32(32767.0)).astype(np.int16)


def phase_rows(h, L):
    """the taps of each phase: row p = h[p], h[p + L], ..."""
    return [np.asarray(h, np.float64)[p::L] for p in range(L)]


def response_db(h, L, freqs_hz):
    """|H(f)| / L in dB of the prototype, which runs at 24000 L Hz"""
    h = np.asarray(h, np.float64)
    fs = float(NATIVE) * L
    out = np.empty(len(freqs_hz))
    i = np.arange(h.size, dtype=np.float64)
    for a in range(0, len(freqs_hz), 256):   # blocks keep the [freqs][taps] matrix small at L = 147
        f = np.asarray(freqs_hz[a: a + 256], np.float64)
        e = np.exp(-2j * np.pi * np.outer(f / fs, i))
        out[a: a + 256] = 20 * np.log10(np.maximum(np.abs(e @ h) / L, 1e-30))
    return out
