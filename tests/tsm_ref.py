"""float64 numpy restatement of include/q3tts_spec.h "speaking rate": the WSOLA stretcher behind the codec.

Positions are sample indices from the stream's reset.  The window tables are the normative f32 ones (evaluated in double, rounded to f32);
everything else is float64.  stretch() chooses its own offsets or, given a list, runs teacher-forced; decisions() judges a trace frame by
frame against the float64 costs; explain() finds the offsets behind an engine's output when no trace is at hand."""
import numpy as np

HOP, WIN, SEARCH, LOOK, HIST, MIN, MAX = 480, 960, 240, 1200, 1920, 50, 200
U = 2.0 ** -24
GAMMA = 482 * U / (1 - 482 * U)          # running-error bound of the 480-term all-positive f32 sum (subtraction, square, add)
DECIDE = (1 + GAMMA) / (1 - GAMMA)


def windows():
    i = np.arange(HOP, dtype=np.float64)
    c = np.cos(2.0 * np.pi * i / WIN)
    return (0.5 - 0.5 * c).astype(np.float32), (0.5 + 0.5 * c).astype(np.float32)


def a_of(pct, k):
    return (int(k) * HOP * int(pct)) // 100


def n_frames(pct, n_native, final):
    """#{k : a_k + 1200 <= N} while streaming, #{k : a_k < N} once final -- counted, not from the closed form"""
    k = 0
    while (a_of(pct, k) < n_native) if final else (a_of(pct, k) + LOOK <= n_native):
        k += 1
    return k


def n_samples(pct, n_native, final):
    return HOP * n_frames(pct, n_native, final)


def order_of(d):
    return 0 if d == 0 else (-2 * d - 1 if d < 0 else 2 * d)


def _padded(x, pct, nf):
    x = np.asarray(x, np.float64)
    need = a_of(pct, max(nf - 1, 0)) + LOOK + HOP
    return np.concatenate([x, np.zeros(max(need - x.size, 0))])


def costs(xp, a, t):
    """(offsets d, SSD64(d)) of every candidate c = a + d >= 0 against the template at t"""
    lo = max(-SEARCH, -a)
    d = np.arange(lo, SEARCH + 1)
    win = np.lib.stride_tricks.sliding_window_view(xp[a + lo: a + SEARCH + HOP], HOP)
    diff = win - xp[t: t + HOP][None, :]
    return d, np.einsum("ij,ij->i", diff, diff)


def choose(d, ssd):
    """the offset that minimises (SSD, o) lexicographically"""
    m = ssd.min()
    return int(min((order_of(int(v)), int(v)) for v in d[ssd == m])[1])


def stretch(x, pct, final=False, deltas=None):
    """y (float64, clamped), the offsets used, and per sample the rounding bound 2^-23 (w|x_p| + w2|x_t|) + 2^-149"""
    x = np.asarray(x, np.float64)
    nf = n_frames(pct, x.size, final)
    xp = _padded(x, pct, nf)
    w, w2 = (t.astype(np.float64) for t in windows())
    y, bound, out, p_prev = np.zeros(nf * HOP), np.zeros(nf * HOP), [], -HOP
    for k in range(nf):
        a, t = a_of(pct, k), p_prev + HOP
        dk = int(deltas[k]) if deltas is not None else choose(*costs(xp, a, t))
        p = a + dk
        assert p >= 0 and abs(dk) <= SEARCH
        y[k * HOP: (k + 1) * HOP] = w * xp[p: p + HOP] + w2 * xp[t: t + HOP]
        bound[k * HOP: (k + 1) * HOP] = 2.0 ** -23 * (w * np.abs(xp[p: p + HOP]) + w2 * np.abs(xp[t: t + HOP])) + 2.0 ** -149
        out.append(dk)
        p_prev = p
    return np.clip(y, -1.0, 1.0), np.array(out, np.int32), bound


def decisions(x, pct, deltas, final=False):
    """teacher-forced judgement of a trace: per frame, with the trace's own d_{k-1}, (ok, decided, d_ref).  ok: SSD64(d_k) is within DECIDE of
    the minimum.  decided: every candidate but the float64 choice lies above DECIDE times the minimum (then d_k must equal d_ref)"""
    x = np.asarray(x, np.float64)
    nf = n_frames(pct, x.size, final)
    assert len(deltas) == nf
    xp = _padded(x, pct, nf)
    res, p_prev = [], -HOP
    for k in range(nf):
        a, t = a_of(pct, k), p_prev + HOP
        d, ssd = costs(xp, a, t)
        ref = choose(d, ssd)
        m = ssd.min()
        dk = int(deltas[k])
        got = ssd[np.nonzero(d == dk)[0][0]] if dk in d else np.inf
        others = ssd[d != ref]
        decided = bool(others.size == 0 or others.min() > m * DECIDE)
        res.append((bool(got <= m * DECIDE), decided, ref))
        p_prev = a + dk
    return res


def s16_of(y32):
    return np.rint(np.asarray(y32, np.float32) * np.float32(32767.0)).astype(np.int16)


def explain(native, got, pct, final=True):
    """finds, hop by hop, the candidate p (with t = previous p + 480) whose overlap-add of `native` is closest to the delivered hop.
    Returns dict(p, recon, ssd_p, ssd_min): the positions, the reconstruction of `got` from them, and per frame the float64 cost of the
    candidate found and the least cost any candidate had against the same template"""
    native = np.asarray(native, np.float64)
    got = np.asarray(got, np.float64)
    nf = got.size // HOP
    xp = _padded(native, pct, max(nf, n_frames(pct, native.size, final)))
    w, w2 = (t.astype(np.float64) for t in windows())
    ps, ssd_p, ssd_min, recon, p_prev = [], [], [], np.zeros(nf * HOP), -HOP
    for k in range(nf):
        a, t = a_of(pct, k), p_prev + HOP
        d, ssd = costs(xp, a, t)
        lo = int(d[0])
        win = np.lib.stride_tricks.sliding_window_view(xp[a + lo: a + SEARCH + HOP], HOP)
        cand = np.clip(w[None, :] * win + (w2 * xp[t: t + HOP])[None, :], -1.0, 1.0)
        err = ((cand - got[k * HOP: (k + 1) * HOP][None, :]) ** 2).sum(axis=1)
        same = np.nonzero(err == err.min())[0]       # w[0] = 0 and zeros past the end make candidates with the very same hop: the cheapest
        j = int(same[np.argmin(ssd[same])])
        ps.append(a + int(d[j])); ssd_p.append(float(ssd[j])); ssd_min.append(float(ssd.min()))
        recon[k * HOP: (k + 1) * HOP] = cand[j]
        p_prev = ps[-1]
    return dict(p=np.array(ps), recon=recon, ssd_p=np.array(ssd_p), ssd_min=np.array(ssd_min))


SPEECH_SEED, NOISE_SEED = 1, 9   # the seeds of the GPU tests' signals: test_tsm_ref_cpu.py shows that they leave no frame undecided in float64


def speech_like(n_frames_, seed=SPEECH_SEED):
    """8 harmonics of f0 = 140 + 25 sin(2 pi 2.3 t), amplitude 0.5 / h, envelope 0.55 + 0.45 sin(2 pi 3.1 t), times 0.5, plus 0.02 Gaussian"""
    n = n_frames_ * 1920
    t = np.arange(n) / 24000.0
    f0 = 140.0 + 25.0 * np.sin(2 * np.pi * 2.3 * t)
    ph = 2 * np.pi * np.cumsum(f0) / 24000.0
    s = sum((0.5 / h) * np.sin(h * ph) for h in range(1, 9))
    s = s * (0.55 + 0.45 * np.sin(2 * np.pi * 3.1 * t)) * 0.5
    s = s + 0.02 * np.random.default_rng(seed).standard_normal(n)
    return np.clip(s, -1.0, 1.0).astype(np.float32)


def noise(n_frames_, seed=NOISE_SEED):
    return (0.3 * np.random.default_rng(seed).standard_normal(n_frames_ * 1920)).astype(np.float32)


def periodic(P, n_frames_, seed):
    tab = np.random.default_rng(seed).uniform(-0.8, 0.8, P).astype(np.float32)
    return tab, tab[np.arange(n_frames_ * 1920) % P]
