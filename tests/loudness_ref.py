"""[EXT] loudness (include/q3tts_spec.h "loudness") restated in numpy / Python at float64, twice: the plain sequential recurrence over the
whole signal, and the segmented evaluation order the spec makes normative (segments of 96 samples from the zero state, one ascending walk
with M = A^96, every segment again from its start state).  Python floats and numpy float64 are IEEE doubles and neither fuses a multiply
with an add, so the segmented form here is bit for bit what the library computes when it is fed the library's own coef and M.  The gate is
restated too."""
import math

import numpy as np

FS, FRAME, SEG, BLOCK, STATE = 24000, 1920, 96, 2400, 6
SEGS_PER_BLOCK = BLOCK // SEG
VOL_MIN, VOL_MAX = -400, 200

# the coefficient table printed in ITU-R BS.1770-4 (48 kHz): shelf b0 b1 b2 a1 a2, high-pass a1 a2
BS1770_48K = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585, -1.99004745483398, 0.99007225036621)
# what the formulas give at 24 kHz (the issue's figures): shelf b0 b1 b2 a1 a2, high-pass a1 a2
K24 = (1.4879002209622763, -2.2462054681411368, 0.904909123246438, -1.3902346051928203, 0.5368384812603979, -1.9801441262289323, 0.9802428178592764)


def coefs(fs=FS):
    """coef [10] float64: shelf b0 b1 b2 a1 a2, high-pass 1 -2 1 a1 a2, through the bilinear transform of BS.1770's analog prototypes"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / fs)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    c = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    c += [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    return np.array(c, np.float64)


def step(s, v, c):
    """one sample through both stages, transposed direct form II; s = [s1, s2, t1, t2] (floats, or arrays: one entry per segment)"""
    y = c[0] * v + s[0]
    s1 = (c[1] * v - c[3] * y) + s[1]
    s2 = c[2] * v - c[4] * y
    z = y + s[2]
    t1 = (-2.0 * y - c[8] * z) + s[3]
    t2 = y - c[9] * z
    return [s1, s2, t1, t2], z


def matrix(coef):
    """M = A^96 [4][4]: column i is the state after 96 zero-input steps from the unit state e_i"""
    c = [float(v) for v in coef]
    M = np.zeros((4, 4), np.float64)
    for i in range(4):
        s = [0.0] * 4
        s[i] = 1.0
        for _ in range(SEG):
            s, _z = step(s, 0.0, c)
        M[:, i] = s
    return M


def sequential(x, coef):
    """z [n] float64: the plain recurrence over the whole signal from the zero state"""
    c = [float(v) for v in coef]
    s = [0.0] * 4
    z = np.zeros(len(x), np.float64)
    for n, v in enumerate(np.asarray(x, np.float64).tolist()):
        s, z[n] = step(s, v, c)
    return z


def sequential_rows(x, coef):
    """rows [len(x) // 2400][2] from the sequential recurrence: the energy of each whole block (numpy's pairwise sum) and its peak"""
    nb = len(x) // BLOCK
    z = sequential(x, coef)[: nb * BLOCK].reshape(nb, BLOCK)
    pk = np.abs(np.asarray(x, np.float64)[: nb * BLOCK]).reshape(nb, BLOCK).max(axis=1) if nb else np.zeros(0)
    return np.stack([(z * z).sum(axis=1), pk], axis=1) if nb else np.zeros((0, 2))


def fresh_state():
    return np.zeros(STATE, np.float64)


def chunk(x, pos, state, coef, M):
    """the segmented evaluation of one chunk x (f32, a multiple of 96 samples) at stream position pos: returns (rows [n][2], the new state)"""
    x = np.asarray(x, np.float32)
    assert x.size % SEG == 0 and pos % SEG == 0
    nseg = x.size // SEG
    X = x.astype(np.float64).reshape(nseg, SEG)
    c = [np.float64(v) for v in coef]
    s = [np.zeros(nseg, np.float64) for _ in range(4)]
    for n in range(SEG):                                   # phase 1
        s, _z = step(s, X[:, n], c)
    Z = [a.tolist() for a in s]
    m = [[float(M[r, j]) for j in range(4)] for r in range(4)]
    cur = [float(v) for v in state[:4]]
    start = np.zeros((nseg, 4), np.float64)
    for k in range(nseg):                                  # phase 2
        start[k] = cur
        cur = [(((m[r][0] * cur[0] + m[r][1] * cur[1]) + m[r][2] * cur[2]) + m[r][3] * cur[3]) + Z[r][k] for r in range(4)]
    s = [start[:, i].copy() for i in range(4)]
    q = np.zeros(nseg, np.float64)
    for n in range(SEG):                                   # phase 3
        s, z = step(s, X[:, n], c)
        q = q + z * z
    p = np.abs(X).max(axis=1) if nseg else np.zeros(0)
    e, pk, rows = float(state[4]), float(state[5]), []
    for k in range(nseg):                                  # the blocks
        e = e + float(q[k])
        pk = max(pk, float(p[k]))
        if (pos // SEG + k + 1) % SEGS_PER_BLOCK == 0:
            rows.append((e, pk))
            e, pk = 0.0, 0.0
    return np.array(rows, np.float64).reshape(-1, 2), np.array(cur + [e, pk], np.float64)


def segmented(x, coef, M, chunks=None, state=None, pos=0):
    """a whole stream through chunk(), cut as `chunks` says (samples each; None: one chunk): (rows, final state)"""
    state = fresh_state() if state is None else state
    chunks = [len(x)] if chunks is None else chunks
    rows, at = [np.zeros((0, 2), np.float64)], 0
    for t in chunks:
        r, state = chunk(x[at: at + t], pos + at, state, coef, M)
        rows.append(r)
        at += t
    assert at == len(x)
    return np.concatenate(rows), state


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def lufs(z):
    return -0.691 + 10.0 * math.log10(z) if z > 0.0 else -math.inf


def gate(rows):
    """the gate over rows [n][2]: dict(integrated_lufs, momentary_max_lufs, peak_dbfs, n_blocks, n_gated)"""
    rows = np.asarray(rows, np.float64).reshape(-1, 2)
    n = rows.shape[0]
    e = rows[:, 0].tolist()
    pk = max(rows[:, 1].tolist() + [0.0])
    out = dict(integrated_lufs=-math.inf, momentary_max_lufs=-math.inf, peak_dbfs=20.0 * math.log10(pk) if pk > 0.0 else -math.inf, n_blocks=n, n_gated=0)
    z = [(((e[j] + e[j + 1]) + e[j + 2]) + e[j + 3]) / 9600.0 for j in range(n - 3)]
    if not z:
        return out
    l = [lufs(v) for v in z]
    out["momentary_max_lufs"] = max(l)
    ab = [v for v, lv in zip(z, l) if lv > -70.0]
    if not ab:
        return out
    s = 0.0
    for v in ab:
        s = s + v
    rel = lufs(s / len(ab)) - 10.0
    both = [v for v, lv in zip(z, l) if lv > -70.0 and lv > rel]
    out["n_gated"] = len(both)
    if both:
        s = 0.0
        for v in both:
            s = s + v
        out["integrated_lufs"] = lufs(s / len(both))
    return out


def response_db(coef, f, fs=FS):
    """10 log10 |H(e^jw)|^2 of the two stages at f Hz"""
    w = np.exp(-2j * np.pi * f / fs)
    h = 1.0
    for o in (0, 5):
        b0, b1, b2, a1, a2 = (float(v) for v in coef[o: o + 5])
        h = h * (b0 + b1 * w + b2 * w * w) / (1.0 + a1 * w + a2 * w * w)
    return 10.0 * math.log10(abs(h) ** 2)


# ---- the signals of the tests (f32, seeded) ----
def noise(n, amp=0.25, seed=7):
    return (np.random.default_rng(seed).standard_normal(n) * amp).clip(-1.0, 1.0).astype(np.float32)


def sine(n, f=997.0, amp=1.0):
    return (amp * np.sin(2.0 * np.pi * f * np.arange(n) / FS)).astype(np.float32)


def dc_hum(n):
    return (0.5 + 0.25 * np.sin(2.0 * np.pi * 20.0 * np.arange(n) / FS)).astype(np.float32)


def impulse(n, at, amp=1.0):
    x = np.zeros(n, np.float32)
    x[at] = amp
    return x


def square(n, period=48):
    return np.where((np.arange(n) // (period // 2)) % 2 == 0, 1.0, -1.0).astype(np.float32)
