"""float64 references of the codec decoder's non-GEMM kernels (csrc/codec.hip, q3tts_op_codec_kernel), written from the oracle's semantics
(oracle/q3o_codec.c), and the error bounds tests/test_gpu_codec_ops.py holds each kernel to (derivations: DESIGN.md "Codec kernels against
float64").

Layouts: R = G * T logical rows, stream g owns rows g*T .. g*T+T-1.  An extended buffer is [G][H + T][C]: H history rows per stream, then the
T new rows.  Plain row buffers are [R][C].  Every bound is per element, |device - ref| <= bar."""
import math

import numpy as np

U = 2.0 ** -24          # unit roundoff of f32
SNAKE_SIN_ERR = 1e-7    # the accuracy codec.hip claims for snake_sin up to |x| = 1e5


def ext_rows(G, T, H, new_only=True):
    """physical rows of an extended buffer: the new rows [G*T] (new_only) or every row [G][H+T]"""
    g, t = np.divmod(np.arange(G * T), T)
    return g * (H + T) + H + t if new_only else np.arange(G * (H + T))


def hist_rows(G, T, H):
    """[G][H] physical rows of the history part of each segment"""
    return (np.arange(G)[:, None] * (H + T) + np.arange(H)[None, :])


# ---------------- RVQ sum ----------------
def rvq_sum(codes, cb, clamp=True):
    """codes [R][n_q], cb [n_q][cb_size][C] -> (sum [R][C], sum of |terms| [R][C])"""
    codes = np.asarray(codes, np.int64)
    cb = np.asarray(cb, np.float64)
    c = np.clip(codes, 0, cb.shape[1] - 1) if clamp else codes % cb.shape[1]
    terms = cb[np.arange(cb.shape[0])[None, :], c]            # [R][n_q][C]
    return terms.sum(1), np.abs(terms).sum(1)


def rvq_bar(n_q, abs_sum):
    return n_q * U * abs_sum


# ---------------- norms ----------------
def _red_depth(C):
    """summation depth of the kernels' row reductions: C/256 per thread, 6 butterfly levels, 3 adds over the 4 waves"""
    return -(-C // 256) + 9


def rmsnorm(x, g, eps):
    x = np.asarray(x, np.float64)
    inv = 1.0 / np.sqrt((x * x).mean(1, keepdims=True) + eps)
    return x * inv * np.asarray(g, np.float64)


def rmsnorm_bar(x, g, eps):
    k = _red_depth(x.shape[1])
    return (0.5 * (k + 1) + 6) * U * np.abs(rmsnorm(x, g, eps)) + 1e-37


def layernorm(x, w, b, eps, two_pass=True):
    x = np.asarray(x, np.float64)
    mu = x.mean(1, keepdims=True)
    var = ((x - mu) ** 2).mean(1, keepdims=True) if two_pass else (x * x).mean(1, keepdims=True) - mu * mu
    return (x - mu) / np.sqrt(var + eps) * np.asarray(w, np.float64) + np.asarray(b, np.float64)


def layernorm_f32_single_pass(x, w, b, eps):
    """the kernel with the variance taken as E[x^2] - mean^2, in f32 (the classic mistake the two-pass kernel avoids)"""
    x = np.asarray(x, np.float32)
    mu = x.mean(1, keepdims=True, dtype=np.float32)
    var = np.maximum((x * x).mean(1, keepdims=True, dtype=np.float32) - mu * mu, np.float32(0))
    return ((x - mu) / np.sqrt(var + np.float32(eps)) * np.asarray(w, np.float32) + np.asarray(b, np.float32)).astype(np.float64)


def layernorm_bar(x, w, b, eps):
    """the mean's error dm enters every centred value; the variance sees it squared plus its own reduction"""
    x = np.asarray(x, np.float64)
    C = x.shape[1]
    k = _red_depth(C)
    mu = x.mean(1, keepdims=True)
    d = x - mu
    var = (d * d).mean(1, keepdims=True)
    inv = 1.0 / np.sqrt(var + eps)
    dm = (k + 1) * U * np.abs(x).mean(1, keepdims=True)
    dd = dm + 2 * U * np.abs(d)
    var_err = 2 * (np.abs(d) * dd).mean(1, keepdims=True) + dm * dm + (k + 3) * U * var
    rel_inv = 0.5 * var_err / (var + eps) + 4 * U
    y = d * inv * np.asarray(w, np.float64) + np.asarray(b, np.float64)
    return np.abs(np.asarray(w, np.float64)) * (dd * inv + np.abs(d) * inv * rel_inv) + 3 * U * (np.abs(y) + np.abs(b)) + 1e-37


# ---------------- RoPE ----------------
def rope_angles(pos, hd, base):
    """[R][hd/2] float64 angles p * base^(-i/half)"""
    half = hd // 2
    return np.asarray(pos, np.float64)[:, None] * np.power(float(base), -np.arange(half) / half)[None, :]


def rope(x, pos, n_heads, hd, base, clamp_at=None, adjacent=False):
    """NeoX RoPE of x [R][n_heads*hd] at absolute positions pos [R]: pairs (i, i + hd/2) of every head (adjacent: (2i, 2i+1), a mistake);
    clamp_at: positions clamped to clamp_at - 1 (the old table clamp).  Returns (rotated, |a||cos| + |b||sin| per element)"""
    x = np.asarray(x, np.float64).reshape(len(pos), n_heads, hd)
    p = np.asarray(pos, np.int64)
    if clamp_at is not None:
        p = np.minimum(p, clamp_at - 1)
    ang = rope_angles(p, hd, base)[:, None, :]
    c, s = np.cos(ang), np.sin(ang)
    half = hd // 2
    if adjacent:
        a, b = x[..., 0::2], x[..., 1::2]
    else:
        a, b = x[..., :half], x[..., half:]
    y = np.empty_like(x)
    mag = np.empty_like(x)
    ya, yb = a * c - b * s, b * c + a * s
    ma, mb = np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)
    if adjacent:
        y[..., 0::2], y[..., 1::2], mag[..., 0::2], mag[..., 1::2] = ya, yb, ma, mb
    else:
        y[..., :half], y[..., half:], mag[..., :half], mag[..., half:] = ya, yb, ma, mb
    return y.reshape(len(pos), -1), mag.reshape(len(pos), -1)


def rope_bar(y, mag):
    """cos / sin rounded to f32 from double (u each), two rounded products and a rounded sum"""
    return 3 * U * mag + U * np.abs(y) + 1e-37


# ---------------- sliding-window attention ----------------
def window_keys(kv_len, t, W, start_off=0):
    """oracle numbering (history positions 0 .. kv_len-1, new row t at kv_len + t): the keys of new row t"""
    j1 = kv_len + t
    return max(0, j1 - (W - 1) + start_off), j1


def window_attn(q, Kx, Vx, kv_len, G, T, W, n_heads, hd, start_off=0, left_aligned=False):
    """q [R][C]; Kx / Vx extended [G][W-1+T][C] with each stream's last kv_len[g] history rows valid (right-aligned; left_aligned: the first
    kv_len rows, a mistake).  Returns (out [R][C], sum_j p_j |v_j| [R][C], per-row score spread and key count)."""
    H = W - 1
    C = n_heads * hd
    q = np.asarray(q, np.float64).reshape(G * T, n_heads, hd)
    Kx = np.asarray(Kx, np.float64).reshape(G, H + T, n_heads, hd)
    Vx = np.asarray(Vx, np.float64).reshape(G, H + T, n_heads, hd)
    out = np.zeros((G * T, n_heads, hd))
    pv = np.zeros_like(out)
    info = []
    for g in range(G):
        L = int(kv_len[g])
        hist = np.arange(L) if left_aligned else np.arange(H - L, H)
        rows = np.concatenate([hist, H + np.arange(T)])       # physical row of oracle position j
        for t in range(T):
            j0, j1 = window_keys(L, t, W, start_off)
            K, V = Kx[g, rows[j0:j1 + 1]], Vx[g, rows[j0:j1 + 1]]  # [n][heads][hd]
            s = np.einsum("nhd,hd->hn", K, q[g * T + t]) / math.sqrt(hd)
            e = np.exp(s - s.max(1, keepdims=True))
            p = e / e.sum(1, keepdims=True)
            out[g * T + t] = np.einsum("hn,nhd->hd", p, V)
            pv[g * T + t] = np.einsum("hn,nhd->hd", p, np.abs(V))
            dot_abs = np.einsum("nhd,hd->hn", np.abs(K), np.abs(q[g * T + t])) / math.sqrt(hd)
            info.append((float((s.max(1) - s.min(1)).max()), j1 - j0 + 1, float(dot_abs.max())))
    return out.reshape(G * T, C), pv.reshape(G * T, C), info


def masked_full_attn(q, seq_k, seq_v, n_heads, hd, W):
    """brute force for one stream: every query position i over all keys j <= i with i - j < W, by masking a full score matrix"""
    n = seq_k.shape[0]
    qh = np.asarray(q, np.float64).reshape(-1, n_heads, hd)
    K = np.asarray(seq_k, np.float64).reshape(n, n_heads, hd)
    V = np.asarray(seq_v, np.float64).reshape(n, n_heads, hd)
    m = qh.shape[0]
    i = np.arange(n - m, n)[:, None]
    j = np.arange(n)[None, :]
    mask = (j <= i) & (i - j < W)
    s = np.einsum("jhd,ihd->ihj", K, qh) / math.sqrt(hd)
    s = np.where(mask[:, None, :], s, -np.inf)
    e = np.exp(s - s.max(2, keepdims=True))
    p = e / e.sum(2, keepdims=True)
    return np.einsum("ihj,jhd->ihd", p, V).reshape(m, -1)


def attn_bar(info, hd, T, pv):
    """|y - y64| <= tol * sum_j p_j |v_j| per row: the scores carry hd rounded products and adds plus the scale (E), the exponent argument
    2E + u * spread, expf within 2 ulp; the PV sum is a chain of n products and adds, the denominator a lane sum and 6 butterfly levels"""
    tol = np.empty(len(info))
    for r, (spread, n, dot) in enumerate(info):
        E = (hd + 2) * U * dot
        delta = 2 * E + U * (spread + 2 * E) + 2 * U
        tol[r] = 2 * delta + (2 * n + 2) * U + (-(-n // 64) + 8) * U + U
    return tol[:, None] * pv + 1e-37


# ---------------- SwiGLU, depthwise conv, SnakeBeta, output conv ----------------
def swiglu(gu, ff):
    gu = np.asarray(gu, np.float64).reshape(-1, 2 * ff)
    g, u = gu[:, :ff], gu[:, ff:]
    return g / (1.0 + np.exp(-g)) * u


def swiglu_bar(ref):
    return 8 * U * np.abs(ref) + 1e-37


def dwconv7(xe, w, b, G, T, H=6):
    """xe extended [G][H+T][C] (H = 6), w [C][7] (tap 6 = the current row), b [C] -> ([R][C], |b| + sum |w x|)"""
    C = w.shape[0]
    xe = np.asarray(xe, np.float64).reshape(G, H + T, C)
    w = np.asarray(w, np.float64)
    out = np.repeat(np.asarray(b, np.float64)[None, None, :], T, 1).repeat(G, 0)
    mag = np.abs(out).copy()
    for j in range(7):
        prod = w[:, j][None, None, :] * xe[:, j:j + T, :]
        out = out + prod
        mag = mag + np.abs(prod)
    return out.reshape(G * T, C), mag.reshape(G * T, C)


def dwconv_bar(mag):
    return 15 * U * mag + 1e-37


def snake_arg(x, ea):
    """the sine's argument, rounded to f32 as the oracle (sinf(v * ea)) and the kernels both round it"""
    return (np.asarray(x, np.float32) * np.asarray(ea, np.float32)).astype(np.float64)


def snake(x, ea, ib, square=True):
    x = np.asarray(x, np.float64)
    s = np.sin(snake_arg(x, ea))
    return x + np.asarray(ib, np.float64) * (s * s if square else s), s


def snake_bar(ref, s, ib):
    return np.abs(np.asarray(ib, np.float64)) * (2 * np.abs(s) * SNAKE_SIN_ERR + SNAKE_SIN_ERR ** 2 + 3 * U * s * s) + 2 * U * np.abs(ref) + 1e-37


def conv_out(xe, w, bias, G, T, H=6, clamp=True):
    """xe extended [G][H+T][C], w [7][C] tap-major (tap 6 = the current row) -> (pcm [R], |bias| + sum |w x|)"""
    C = w.shape[1]
    xe = np.asarray(xe, np.float64).reshape(G, H + T, C)
    w = np.asarray(w, np.float64)
    acc = np.full((G, T), float(bias))
    mag = np.full((G, T), abs(float(bias)))
    for j in range(7):
        prod = xe[:, j:j + T, :] * w[j][None, None, :]
        acc = acc + prod.sum(2)
        mag = mag + np.abs(prod).sum(2)
    acc = acc.reshape(-1)
    return (np.clip(acc, -1.0, 1.0) if clamp else acc), mag.reshape(-1)


def conv_out_bar(C, mag):
    """per lane: 4 products summed and added (7C/4/64 times), 6 butterfly levels, the bias; the clamp is 1-Lipschitz"""
    return (-(-7 * C // 256) * 5 + 8) * U * mag + 1e-37


# ---------------- histories ----------------
def hist_load(store, work, slots, G, T, H, C):
    """work extended [G][H+T][C] with every stream's history rows from store [n][H][C] slot slots[g]"""
    w = np.array(work, copy=True).reshape(G, H + T, C)
    s = np.asarray(store).reshape(-1, H, C)
    for g in range(G):
        w[g, :H] = s[slots[g]]
    return w.reshape(-1)


def hist_save(work, store, slots, G, T, H, C):
    """the last H rows of (history + new rows) of stream g become slot slots[g]'s next history"""
    w = np.asarray(work).reshape(G, H + T, C)
    s = np.array(store, copy=True).reshape(-1, H, C)
    for g in range(G):
        s[slots[g]] = w[g, T:T + H]
    return s.reshape(-1)
