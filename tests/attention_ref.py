"""Float64 restatement of one transformer attention step, written from the spec's words and independent of the C code: per-head RMSNorm
(S4'), NeoX M-RoPE (S5), f16 KV append (S6), causal GQA attention (S7), int8 block quantisation (S2), and the paged device layout of the
KV caches.  Also the error bound the GPU attention tests hold every kernel form to (tests/test_gpu_attention.py)."""
import math

import numpy as np

HD = 128          # head dim
PAGE = 64         # positions per KV page
CHUNK = 256       # positions per softmax chunk of the S7 kernels
U = 2.0 ** -24    # unit roundoff of f32
NAN16 = 0x7E00    # a quiet f16 NaN


# ---------------- S4' / S5 ----------------
def mrope_stream(i, sec):
    """pair i rotates with stream s where i mod sum(sec) falls in section s; sum(sec) = 0 means stream 0"""
    tot = int(sum(sec))
    if tot <= 0:
        return 0
    r, acc = i % tot, 0
    for s in range(4):
        acc += int(sec[s])
        if r < acc:
            return s
    raise AssertionError("unreachable")


def head_norm(x, w, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt(np.mean(x * x) + float(np.float32(eps))) * np.asarray(w, np.float64)


def rope_angles(pos4, sec, base, n_ctx):
    """angle of pair i: p * base^(-i/64), p = the pair's stream position clamped to [0, n_ctx - 1]"""
    i = np.arange(64)
    stream = np.array([mrope_stream(k, sec) for k in i])
    p = np.clip(np.asarray(pos4, np.int64)[stream], 0, n_ctx - 1).astype(np.float64)
    return p * np.power(float(np.float32(base)), -i / 64.0)


def rope(y, ang):
    c, s = np.cos(ang), np.sin(ang)
    y1, y2 = y[:64], y[64:]
    return np.concatenate([y1 * c - y2 * s, y2 * c + y1 * s])


def head_rope(x, w, eps, pos4, sec, base, n_ctx):
    """(rotated vector, |y1| + |y2| of each element's pair): the second is what f32 rounding errors of the rotation scale with"""
    y = head_norm(x, w, eps)
    mag = np.abs(y[:64]) + np.abs(y[64:])
    return rope(y, rope_angles(pos4, sec, base, n_ctx)), np.concatenate([mag, mag])


# ---------------- f16 ----------------
def f16_bits(x):
    """round to nearest even f16, as bit patterns"""
    return np.asarray(x).astype(np.float16).view(np.uint16)


def h2f(bits):
    return np.asarray(bits, np.uint16).view(np.float16).astype(np.float64)


def f16_bracket(lo, hi):
    """the f16 values v with round_down(lo) <= v <= round_up(hi) (as float64 bounds)"""
    a = np.asarray(lo, np.float64).astype(np.float16)
    a = np.where(a.astype(np.float64) > lo, np.nextafter(a, np.float16(-np.inf)), a)
    b = np.asarray(hi, np.float64).astype(np.float16)
    b = np.where(b.astype(np.float64) < hi, np.nextafter(b, np.float16(np.inf)), b)
    return a.astype(np.float64), b.astype(np.float64)


# ---------------- S7 ----------------
def attention(q, K, V):
    """causal-prefix attention of one query head over n positions: (y[128], sum_j p_j |v_j| [128], scores[n])"""
    K = np.asarray(K, np.float64)
    V = np.asarray(V, np.float64)
    s = K @ np.asarray(q, np.float64) / math.sqrt(HD)
    e = np.exp(s - s.max())
    p = e / e.sum()
    return p @ V, p @ np.abs(V), s


def attention_tol(form, q, qmag, K):
    """tol of |y - y64| <= tol * sum_j p_j |v_j| for one head (derivation: DESIGN.md "Attention forms against float64").
    q / qmag: the f64 query and its pair magnitudes; K: the stored keys (f64 of the f16 the device holds)."""
    K = np.asarray(K, np.float64)
    n = K.shape[0]
    c = 1.0 / math.sqrt(HD)
    s = c * (K @ q)
    dot_abs = c * (np.abs(K) @ np.abs(q))         # scale * sum_d |q_d k_d|
    dot_mag = c * (np.abs(K) @ qmag)              # scale * sum_d (|y1| + |y2|)_d |k_d|
    if form == "GGML":
        # score: 128 products and 128 adds, each rounded; q from the double-sum norm and the rotation
        E = (2 * HD + 2) * U * dot_abs + 16 * U * dot_mag
    else:
        E = (HD + 2) * U * dot_abs + 16 * U * dot_mag        # f32 fma chain of 128 terms and the scale; q from norm + rotation
    R = float(s.max() - s.min() + 2 * E.max())               # spread of the device's scores
    if form == "GGML":
        delta = 2 * float(E.max()) + U * R + 2 * U          # two score errors, the rounded argument, glibc expf (< 1 ulp)
        gamma = (2 * n + 4) * U                              # PV: n rounded products + n rounded adds; 1/sum and the final product
    else:
        delta = 2 * float(E.max()) + U * R + 3 * U           # two score errors, the rounded argument, Cephes expf
        chunks = -(-n // CHUNK)
        chain = -(-min(n, CHUNK) // 16)
        gamma = (chain + 8 + chunks * (8 + R)) * U           # PV chains + combine tree, per-chunk rescale (two expf, rounded argument)
    return 2 * delta + 2 * gamma + U                         # numerator and denominator (L) each; the final division


# ---------------- S2 ----------------
def quant_blocks(x):
    """int8 blocks of 32 with f16 scales, in f32 arithmetic: d = amax / 127, q = rint(x * (1 / d))"""
    x = np.asarray(x, np.float32).reshape(-1, 32)
    amax = np.abs(x).max(axis=1)
    d = (amax / np.float32(127)).astype(np.float32)
    inv = np.where(d != 0, np.float32(1) / np.where(d != 0, d, np.float32(1)), np.float32(0)).astype(np.float32)
    q = np.rint(x * inv[:, None]).astype(np.int8)
    return q.reshape(-1), f16_bits(d)


# ---------------- paged layout ----------------
def new_caches(n_pages, n_layer, n_kv, fill):
    """K [page][layer][kvh][16][64][8] and V [page][layer][kvh][64][128] f16 bit patterns, every element = fill"""
    K = np.full((n_pages, n_layer, n_kv, 16, PAGE, 8), fill, np.uint16)
    V = np.full((n_pages, n_layer, n_kv, PAGE, HD), fill, np.uint16)
    return K, V


def _where(pages, positions):
    positions = np.asarray(positions, np.int64)
    return np.asarray(pages, np.int64)[positions // PAGE], positions % PAGE


def write_rows(Kc, Vc, pages, layer, positions, K_rows, V_rows):
    """logical rows [len][n_kv][128] of one sequence (physical page of logical page lp = pages[lp]) into the paged caches"""
    pg, pp = _where(pages, positions)
    n = pg.size
    Kc[pg, layer, :, :, pp, :] = np.asarray(K_rows, np.uint16).reshape(n, -1, 16, 8)
    Vc[pg, layer, :, pp, :] = np.asarray(V_rows, np.uint16).reshape(n, -1, HD)


def read_rows(Kc, Vc, pages, layer, positions):
    """the inverse of write_rows: ([len][n_kv][128], [len][n_kv][128])"""
    pg, pp = _where(pages, positions)
    n = pg.size
    return Kc[pg, layer, :, :, pp, :].reshape(n, -1, HD), Vc[pg, layer, :, pp, :].reshape(n, -1, HD)
