"""float64 numpy restatement of include/q3tts_spec.h "pitch": the stretcher of tests/tsm_ref.py at the rational tempo R / P (stage 1, z) and
the L / M = 100 / P resampler behind it (stage 2, y).

Positions are sample indices from the stream's reset.  The window tables and the tap tables are the normative f32 ones (evaluated in double,
rounded to f32); everything else is float64.  Counts are counted, not taken from the closed forms.  table() restates the library's builder
operation for operation (the same power series, the same libm sine), so the two agree bit for bit."""
import functools
import math

import numpy as np

import tsm_ref as T

HOP, LOOK, SEARCH, HIST, ZHIST, MIN, MAX, Z, BETA = T.HOP, T.LOOK, T.SEARCH, T.HIST, 64, 50, 200, 16, 9.0
U = 2.0 ** -24
# the (rate, pitch) pairs of the GPU decision tests: test_pitch_ref_cpu.py shows that tsm_ref's speech_like(12) and noise(9) leave no frame
# undecided in float64 at any of them
GPU_PAIRS = ((100, 107), (100, 89), (100, 50), (100, 200), (125, 80), (90, 120), (150, 75), (77, 131), (100, 199))


def pair_ok(R, P):
    return MIN <= R <= MAX and MIN <= P <= MAX and 2 * R >= P and R <= 2 * P


def plan(P):
    """(L, M, N, taps): 100 / P = L / M in lowest terms, N prototype taps, at most `taps` terms per delivered sample"""
    g = math.gcd(100, P)
    L, M = 100 // g, P // g
    N = 2 * Z * max(L, M) + 1
    return L, M, N, -(-N // L)


def _i0(x):
    """the library's power series, element by element: a term is added until it no longer changes the sum"""
    x = np.asarray(x, np.float64)
    q = x * x / 4.0
    term, s = np.ones_like(q), np.ones_like(q)
    for k in range(1, 500):
        term = term * (q / (float(k) * float(k)))
        nxt = s + term
        if np.array_equal(nxt, s):
            break
        s = nxt
    return s


@functools.lru_cache(maxsize=None)
def table(P):
    """h32 of pitch P"""
    L, M, N, _ = plan(P)
    F = max(L, M)
    c = Z * F
    fc2 = 0.9 / float(F)
    i = np.arange(N, dtype=np.float64) - float(c)
    x = fc2 * i
    r = i / float(c)
    px = math.pi * x
    with np.errstate(invalid="ignore", divide="ignore"):
        sinc = np.array([math.sin(v) for v in px]) / px
    sinc[c] = 1.0
    w = _i0(BETA * np.sqrt(1.0 - r * r)) / _i0(np.float64(BETA))
    h = (float(L) * fc2 * sinc * w).astype(np.float32)
    h.setflags(write=False)
    return h


def a_of(R, P, k):
    return (int(k) * HOP * int(R)) // int(P)


def n_frames(R, P, n_native, final):
    """#{k : a_k + 1200 <= N} while streaming, #{k : a_k < N} once final -- counted"""
    k = 0
    while (a_of(R, P, k) < n_native) if final else (a_of(R, P, k) + LOOK <= n_native):
        k += 1
    return k


def n_of_z(P, nz):
    """delivered samples of nz intermediate ones: #{n : n M div L < nz} -- counted"""
    L, M, _, _ = plan(P)
    n = np.arange(0, 2 * nz + 2, dtype=np.int64)
    return int(np.count_nonzero((n * M) // L < nz))


def n_samples(R, P, n_native, final):
    return n_of_z(P, HOP * n_frames(R, P, n_native, final))


def _padded(x, R, P, nf):
    x = np.asarray(x, np.float64)
    need = a_of(R, P, max(nf - 1, 0)) + LOOK + HOP
    return np.concatenate([x, np.zeros(max(need - x.size, 0))])


def reach(R, P, frames=400):
    """brute force over both extremes of d: the least t_k - a_k, the greatest t_k + 480 - a_k and p_k + 960 - a_k over `frames` frames"""
    lo, hi = 0, 0
    for d in (-SEARCH, SEARCH):
        for k in range(1, frames):
            t = a_of(R, P, k - 1) + d + HOP
            lo, hi = min(lo, t - a_of(R, P, k)), max(hi, t + HOP - a_of(R, P, k))
    return lo, max(hi, SEARCH + 2 * HOP)


def stretch(x, R, P, final=False, deltas=None):
    """stage 1: z (float64, clamped), the offsets used, and per sample the rounding bound 2^-23 (w|x_p| + w2|x_t|) + 2^-149"""
    x = np.asarray(x, np.float64)
    nf = n_frames(R, P, x.size, final)
    xp = _padded(x, R, P, nf)
    w, w2 = (t.astype(np.float64) for t in T.windows())
    z, bound, out, p_prev = np.zeros(nf * HOP), np.zeros(nf * HOP), [], -HOP
    for k in range(nf):
        a, t = a_of(R, P, k), p_prev + HOP
        dk = int(deltas[k]) if deltas is not None else T.choose(*T.costs(xp, a, t))
        p = a + dk
        assert p >= 0 and abs(dk) <= SEARCH and t >= 0
        z[k * HOP: (k + 1) * HOP] = w * xp[p: p + HOP] + w2 * xp[t: t + HOP]
        bound[k * HOP: (k + 1) * HOP] = 2.0 ** -23 * (w * np.abs(xp[p: p + HOP]) + w2 * np.abs(xp[t: t + HOP])) + 2.0 ** -149
        out.append(dk)
        p_prev = p
    return np.clip(z, -1.0, 1.0), np.array(out, np.int32), bound


def decisions(x, R, P, deltas, final=False):
    """tsm_ref.decisions at the rational tempo: per frame, with the trace's own d_{k-1}, (ok, decided, d_ref)"""
    x = np.asarray(x, np.float64)
    nf = n_frames(R, P, x.size, final)
    assert len(deltas) == nf
    xp = _padded(x, R, P, nf)
    res, p_prev = [], -HOP
    for k in range(nf):
        a, t = a_of(R, P, k), p_prev + HOP
        d, ssd = T.costs(xp, a, t)
        ref = T.choose(d, ssd)
        m = ssd.min()
        dk = int(deltas[k])
        got = ssd[np.nonzero(d == dk)[0][0]] if dk in d else np.inf
        others = ssd[d != ref]
        decided = bool(others.size == 0 or others.min() > m * T.DECIDE)
        res.append((bool(got <= m * T.DECIDE), decided, ref))
        p_prev = a + dk
    return res


def gamma(n):
    return n * U / (1.0 - n * U)


def resample(z, P, bz=None, before=None, n0=0, n1=None):
    """stage 2 in float64 over the f32 taps: delivered samples [n0, n1) (default: all ceil(nz L / M)) of the intermediate stream z, with
    z[m < 0] = before(m) (default 0).  Returns (y clamped, bound) with bound = sum |h| bz[j - k] + gamma(K + 1) sum |h z| + 2^-149, K the
    terms of the sample"""
    z = np.asarray(z, np.float64)
    L, M, N, taps = plan(P)
    h = table(P).astype(np.float64)
    n1 = n_of_z(P, z.size) if n1 is None else n1
    n = np.arange(n0, n1, dtype=np.int64)
    t = n * M
    p, j = t % L, t // L
    assert n.size == 0 or j.max() < z.size
    bz = np.zeros(z.size) if bz is None else np.asarray(bz, np.float64)
    y, A, B, K = np.zeros(n.size), np.zeros(n.size), np.zeros(n.size), np.zeros(n.size)
    for k in range(taps):
        idx = p + k * L
        ok = idx < N
        hk = np.where(ok, h[np.minimum(idx, N - 1)], 0.0)
        m = j - k
        inside = m >= 0
        zz = np.where(inside, z[np.maximum(m, 0)], 0.0)
        if before is not None:
            zz = np.where(inside, zz, before(m))
        bb = np.where(inside, bz[np.maximum(m, 0)], 0.0)
        y += hk * zz
        A += np.abs(hk) * bb
        B += np.abs(hk * zz)
        K += ok
    return np.clip(y, -1.0, 1.0), A + gamma(K + 1) * B + 2.0 ** -149


def pitch(x, R, P, final=False, deltas=None):
    """both stages: (y64, its bound, the offsets, z64)"""
    z, d, bz = stretch(x, R, P, final, deltas)
    y, b = resample(z, P, bz)
    return y, b, d, z


def s16_of(y32):
    return T.s16_of(y32)


def crossings_hz(y, rate=24000.0):
    """(frequency, margin) of a tone from the upward zero crossings of the middle third: (count - 1) periods over the span between the first
    and the last, each located by linear interpolation; the margin is one crossing interval over the span"""
    y = np.asarray(y, np.float64)
    a, b = y.size // 3, 2 * y.size // 3
    s = y[a:b]
    i = np.nonzero((s[:-1] < 0) & (s[1:] >= 0))[0]
    assert i.size >= 3
    pos = i + s[i] / (s[i] - s[i + 1])
    f = (pos.size - 1) * rate / (pos[-1] - pos[0])
    return f, f / (pos.size - 1)
