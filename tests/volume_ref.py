"""[EXT] volume (include/q3tts_spec.h "volume") restated in numpy: the float64 evaluation the kernel is judged against, its f32 twin with
the kernel's roundings, the error bounds, and the signals the GPU tests use.  Every function takes x, a stream's native f32 samples from its
reset, and returns arrays of x's length: sample n of the result is sample n of the stream."""
import numpy as np

VOL_MIN, VOL_MAX, LOOK, HOLD, DELAY, HIST = -400, 200, 128, 512, 127, 638
FRAME = 1920
U = 2.0 ** -24
SPEECH_SEED = 20261


def gain(db10):
    """G = (float) pow(10.0, db10 / 200.0)"""
    assert VOL_MIN <= db10 <= VOL_MAX
    return np.float32(np.power(10.0, db10 / 200.0))


def scaled(x, db10):
    """v = G * x, one f32 multiply"""
    return (gain(db10) * np.asarray(x, np.float32)).astype(np.float32)


def _levels(v, dt, tree=True):
    """(g, delayed v) in the number format dt from the f32 v; index j of the padded arrays is sample j - HIST, and v[n < 0] = 0"""
    one = dt(1.0)
    vp = np.concatenate([np.zeros(HIST, dt), np.asarray(v, np.float32).astype(dt)])
    av = np.abs(vp)
    with np.errstate(divide="ignore"):
        r = np.where(av <= one, one, one / av).astype(dt)
    m = r.copy()
    for i in range(9):                              # min over [k - 511, k]: exact in any order
        off = 1 << i
        m[off:] = np.minimum(m[off:], m[:-off].copy())
    s = m.copy()
    if tree:
        for i in range(7):                          # s_{i+1}[k] = s_i[k - 2^i] + s_i[k]
            off = 1 << i
            s[off:] = (s[:-off].copy() + s[off:]).astype(dt)
    else:                                           # the plain window sum, oldest term first
        s[LOOK - 1:] = np.lib.stride_tricks.sliding_window_view(m, LOOK).sum(axis=1).astype(dt)
    g = (dt(2.0 ** -7) * s)[HIST:]
    vd = vp[HIST - DELAY: vp.size - DELAY]
    return g.astype(dt), vd


def volume64(v, tree=True):
    """(y, g, unclamped product) in float64 from the f32 v"""
    g, vd = _levels(v, np.float64, tree)
    p = g * vd
    return np.clip(p, -1.0, 1.0), g, p


def volume32(v):
    """(y, g) with the kernel's roundings: every operation in f32"""
    g, vd = _levels(v, np.float32)
    y = (g * vd).astype(np.float32)
    return np.where(y < -1, np.float32(-1), np.where(y > 1, np.float32(1), y)).astype(np.float32), g


def y_bound(y64):
    """given the same f32 v: one rounding in r, none in the minimum, seven in the tree of non-negative adds, one in the product"""
    return 10 * U * np.abs(y64) + 2.0 ** -149


def g_bound(g64):
    return 8 * U * np.abs(g64)


def limited_share(v):
    """the share of samples whose float64 gain is below 1"""
    return float(np.mean(volume64(v)[1] < 1.0))


def speech_like(n_frames, seed=SPEECH_SEED):
    """a harmonic tone whose fundamental glides between 80 and 140 Hz, 6 harmonics of amplitude 1 / h, under the slow envelope
    0.04 + 0.96 sin^4(2 pi 1.3 t + 0.4), normalised to a peak of 0.9, plus 1 % Gaussian noise; clamped like the output conv's samples"""
    n = n_frames * FRAME
    t = np.arange(n) / 24000.0
    f0 = 110.0 + 30.0 * np.sin(2 * np.pi * 0.9 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 24000.0
    s = sum((1.0 / h) * np.sin(h * ph + 0.7 * h) for h in range(1, 7))
    s = s * (0.04 + 0.96 * np.sin(2 * np.pi * 1.3 * t + 0.4) ** 4)
    s = 0.9 * s / np.abs(s).max()
    s = s + 0.01 * np.random.default_rng(seed).standard_normal(n)
    return np.clip(s, -1.0, 1.0).astype(np.float32)


def quiet(n_frames, seed=SPEECH_SEED + 1):
    """the speech-like signal scaled so that a boost of 6 dB stays below 1"""
    return (np.float32(0.45) * speech_like(n_frames, seed)).astype(np.float32)
