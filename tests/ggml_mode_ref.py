"""Plain numpy restatement of the ggml-mode arithmetic (csrc/ggml_mode.hip, oracle/q3o_ggml.c) and its float64 side.

Every f32 step of ggml's portable ("generic") CPU path is one numpy float32 operation here, in ggml's order, so nothing is contracted into an
fma and every intermediate is rounded where ggml rounds it.  Quantised weights are decoded from the raw GGUF bytes by this file's own readers
(the public block formats: Q8_0 {f16 d; i8 qs[32]}, Q5_K {f16 d, dmin; u8 scales[12]; u8 qh[32]; u8 qs[128]}, Q6_K {u8 ql[128]; u8 qh[64];
i8 scales[16]; f16 d}).  tests/test_ggml_mode_ref_cpu.py holds all of it against the oracle bit for bit; tests/test_gpu_ggml_mode.py holds
the device against it.

The float64 side works on DEQUANTISED operands (weights w = a - b from linear_ref.decode_parts, activations xq * scale), which float64 holds
exactly, so the only error bounded is the f32 arithmetic's.  Bounds are gamma(n) * magnitude (u = 2^-24, linear_ref.gamma) plus a floor for
results that leave the normal f32 range; each n is derived where it is used.  They hold while no f32 intermediate overflows."""
import numpy as np

from linear_ref import gamma

F = np.float32
ROW_BYTES = {8: lambda k: k // 32 * 34, 13: lambda k: k // 256 * 176, 14: lambda k: k // 256 * 210}
TINY = 2.0 ** -149          # the smallest f32 subnormal: the most one rounding into the subnormal range can move a result


def _h2f(u8pairs):
    """[..., 2] u8 -> [...] f32 (the f16 they spell, converted exactly)"""
    return np.ascontiguousarray(u8pairs).view(np.float16)[..., 0].astype(F)


# ---------------------------------------------------------------- rounding rules ----------------------------------------------------------
def roundf(v):
    """C roundf on f32: half away from zero.  t = trunc(v) and v - t are exact, so nothing here rounds twice"""
    v = np.asarray(v, F)
    t = np.trunc(v)
    return (t + np.where(np.abs(v - t) >= F(0.5), np.copysign(F(1), v), F(0))).astype(F)


def nearest_int(v):
    """ggml's nearest_int: the low mantissa bits of v + 1.5 * 2^23, i.e. round half to even for |v| <= 2^22"""
    val = (np.asarray(v, F) + F(12582912.0)).astype(F)
    return (val.view(np.int32) & 0x007FFFFF) - 0x00400000


def _to_i8(i):
    return np.asarray(i).astype(np.int64).astype(np.int8)   # C's (int8_t) of an int: the low byte


# ---------------------------------------------------------------- the two activation quantisers -------------------------------------------
def quantize_row_q8_0(x, rnd=roundf):
    """quantize_row_q8_0_ref per 32: d = amax / 127, id = d ? 1 / d : 0, q = roundf(x * id), scale stored as f16.
    x [ntok][k] f32 -> q8 [ntok][k] int8, d8 [ntok][k/32] uint16.  rnd: the rounding rule (the tie test swaps it)"""
    x = np.asarray(x, F)
    nt, k = x.shape
    blk = x.reshape(nt, k // 32, 32)
    amax = np.abs(blk).max(-1)
    d = amax / F(127)
    with np.errstate(divide="ignore"):
        id_ = np.where(d != 0, F(1) / d, F(0)).astype(F)
    q = rnd(blk * id_[..., None])
    return _to_i8(q).reshape(nt, k), d.astype(np.float16).view(np.uint16)


def quantize_row_q8_K(x, rnd=nearest_int):
    """quantize_row_q8_K_ref per 256: max = the FIRST element of largest magnitude, sign kept; iscale = -127 / max; q = min(127,
    nearest_int(iscale * x)); d = 1 / iscale; bsums = sums of 16.  An all-zero super-block is d = 0, q = 0, bsums = 0.
    x [ntok][k] f32 -> qk [ntok][k] int8, dk [ntok][k/256] f32, bs [ntok][k/16] int16"""
    x = np.asarray(x, F)
    nt, k = x.shape
    blk = x.reshape(nt, k // 256, 256)
    first = np.abs(blk).argmax(-1)                      # argmax returns the first maximum, as the strict `ax > amax` keeps it
    mx = np.take_along_axis(blk, first[..., None], -1)[..., 0]
    zero = mx == 0
    with np.errstate(divide="ignore", invalid="ignore"):
        iscale = F(-127) / np.where(zero, F(1), mx).astype(F)
        v = np.asarray(rnd(iscale[..., None] * blk)).astype(np.int64)
        q = _to_i8(np.minimum(v, 127))
        d = (F(1) / iscale).astype(F)
    q[zero] = 0
    d = np.where(zero, F(0), d).astype(F)
    bs = q.astype(np.int32).reshape(nt, k // 256, 16, 16).sum(-1).astype(np.int16)
    return q.reshape(nt, k), d, bs.reshape(nt, k // 16)


def quantize(x):
    """what k_gg_quant writes: (q8, d8, qk, dk, bs)"""
    return quantize_row_q8_0(x) + quantize_row_q8_K(x)


# ---------------------------------------------------------------- weight readers (integers and f32 scales) --------------------------------
def _scale_min_k4(s):
    """get_scale_min_k4 over s [..., 12] -> sc, m [..., 8]"""
    s = s.astype(np.int32)
    sc = np.zeros(s.shape[:-1] + (8,), np.int32); m = np.zeros_like(sc)
    for j in range(8):
        if j < 4:
            sc[..., j] = s[..., j] & 63; m[..., j] = s[..., j + 4] & 63
        else:
            sc[..., j] = (s[..., j + 4] & 0xF) | ((s[..., j - 4] >> 6) << 4)
            m[..., j] = (s[..., j + 4] >> 4) | ((s[..., j] >> 6) << 4)
    return sc, m


def read_q8_0(raw, n, k):
    b = np.ascontiguousarray(raw, np.uint8).reshape(n, k // 32, 34)
    return _h2f(b[..., 0:2]), b[..., 2:].view(np.int8).astype(np.int32)                  # d [n][nb], q [n][nb][32]


def read_q5_k(raw, n, k):
    b = np.ascontiguousarray(raw, np.uint8).reshape(n, k // 256, 176)
    sc, m = _scale_min_k4(b[..., 4:16])
    qh, qs = b[..., 16:48].astype(np.int32), b[..., 48:176].astype(np.int32)
    a = np.zeros(b.shape[:2] + (256,), np.int32)
    for p in range(4):                                                                     # 64 elements per pass, as dequantize_row_q5_K walks them
        ql = qs[..., 32 * p:32 * p + 32]
        a[..., 64 * p:64 * p + 32] = (ql & 0xF) + np.where(qh & (1 << (2 * p)), 16, 0)
        a[..., 64 * p + 32:64 * p + 64] = (ql >> 4) + np.where(qh & (2 << (2 * p)), 16, 0)
    return _h2f(b[..., 0:2]), _h2f(b[..., 2:4]), sc, m, a                                  # d, dmin [n][nsb]; sc, m [n][nsb][8]; a [n][nsb][256]


def read_q6_k(raw, n, k):
    b = np.ascontiguousarray(raw, np.uint8).reshape(n, k // 256, 210)
    ql, qh = b[..., 0:128].astype(np.int32), b[..., 128:192].astype(np.int32)
    a = np.zeros(b.shape[:2] + (256,), np.int32)
    for h in range(2):                                                                     # 128 elements per pass, as dequantize_row_q6_K walks them
        L, H = ql[..., 64 * h:64 * h + 64], qh[..., 32 * h:32 * h + 32]
        a[..., 128 * h + 0:128 * h + 32] = ((L[..., :32] & 0xF) | (((H >> 0) & 3) << 4)) - 32
        a[..., 128 * h + 32:128 * h + 64] = ((L[..., 32:] & 0xF) | (((H >> 2) & 3) << 4)) - 32
        a[..., 128 * h + 64:128 * h + 96] = ((L[..., :32] >> 4) | (((H >> 4) & 3) << 4)) - 32
        a[..., 128 * h + 96:128 * h + 128] = ((L[..., 32:] >> 4) | (((H >> 6) & 3) << 4)) - 32
    return _h2f(b[..., 208:210]), b[..., 192:208].view(np.int8).astype(np.int32), a       # d [n][nsb]; sc [n][nsb][16] SIGNED; a [n][nsb][256]


def n_negative_q6k_scales(raw, n, k):
    return int((read_q6_k(raw, n, k)[1] < 0).sum())


# ---------------------------------------------------------------- ggml_vec_dot_*_generic --------------------------------------------------
def vec_dot_q8_0(raw, n, k, q8, d8):
    """-> [ntok][n] f32: per 32-block sumi (int), sumf = sumf + (float)sumi * (d_w * d_x), blocks in order"""
    wd, wq = read_q8_0(raw, n, k)
    nt = q8.shape[0]
    xq = q8.astype(np.int32).reshape(nt, k // 32, 32)
    xd = np.ascontiguousarray(d8, np.uint16).view(np.float16).astype(F).reshape(nt, k // 32)
    sumi = np.einsum("rbj,tbj->trb", wq, xq)
    sumf = np.zeros((nt, n), F)
    for ib in range(k // 32):
        sc = wd[None, :, ib] * xd[:, None, ib]
        sumf = sumf + sumi[:, :, ib].astype(F) * sc
    return sumf


def _k_dot(d, aux, xdk, dmin=None, sumi=None):
    """the shared tail of the two K-quant dots.  d [n][nsb] f32, aux [ntok][n][nsb][8] int (the eight lane sums of a super-block),
    xdk [ntok][nsb] f32; with mins: sumf = sumf - (dmin * xdk) * (float)sumi per super-block.  Then sumf += sums[l], l = 0..7"""
    nt, n, nsb, _ = aux.shape
    sums = np.zeros((nt, n, 8), F)
    sumf = np.zeros((nt, n), F)
    for i in range(nsb):
        dd = d[None, :, i] * xdk[:, None, i]
        sums = sums + dd[..., None] * aux[:, :, i, :].astype(F)
        if dmin is not None:
            dm = dmin[None, :, i] * xdk[:, None, i]
            sumf = sumf - dm * sumi[:, :, i].astype(F)
    for l in range(8):
        sumf = sumf + sums[..., l]
    return sumf


def vec_dot_q5_K(raw, n, k, qk, dk, bs):
    """aux32[l] += scale_j * (int16)(q8[e] * a[e]) over the elements e = l (mod 8) of sub-block j = e / 32 (|q8 a| <= 128 * 31: the int16 never
    wraps); sumi = sum_j bsums[j] * mins[j / 2]"""
    d, dmin, sc, m, a = read_q5_k(raw, n, k)
    nt, nsb = qk.shape[0], k // 256
    wa = (a * np.repeat(sc, 32, axis=-1)).reshape(n, nsb, 32, 8)
    xq = qk.astype(np.int32).reshape(nt, nsb, 32, 8)
    aux = np.einsum("risl,tisl->tril", wa, xq)
    sumi = np.einsum("tij,rij->tri", bs.astype(np.int32).reshape(nt, nsb, 16), np.repeat(m, 2, axis=-1))
    return _k_dot(d, aux, np.asarray(dk, F).reshape(nt, nsb), dmin, sumi)


def vec_dot_q6_K(raw, n, k, qk, dk):
    """aux32[l] += scale_j * (int16)(q8[e] * a[e]) over the elements e = l (mod 8) of the 16-element sub-block j = e / 16, scale_j a SIGNED int8"""
    d, sc, a = read_q6_k(raw, n, k)
    nt, nsb = qk.shape[0], k // 256
    wa = (a * np.repeat(sc, 16, axis=-1)).reshape(n, nsb, 32, 8)
    xq = qk.astype(np.int32).reshape(nt, nsb, 32, 8)
    return _k_dot(d, np.einsum("risl,tisl->tril", wa, xq), np.asarray(dk, F).reshape(nt, nsb))


def matvec(raw, qtype, n, k, row0, nrows, act):
    """k_gg_matvec: rows [row0, row0 + nrows) of the n-row matrix against the quantised activations act = (q8, d8, qk, dk, bs) -> [ntok][nrows]"""
    q8, d8, qk, dk, bs = act
    rb = ROW_BYTES[qtype](k)
    rows = np.ascontiguousarray(raw, np.uint8).reshape(n, rb)[row0:row0 + nrows]
    if qtype == 8:
        return vec_dot_q8_0(rows, nrows, k, q8, d8)
    if qtype == 13:
        return vec_dot_q5_K(rows, nrows, k, qk, dk, bs)
    return vec_dot_q6_K(rows, nrows, k, qk, dk)


def dequant_act(qtype, act):
    """the activations the dot of `qtype` sees, exact in float64"""
    q8, d8, qk, dk, bs = act
    if qtype == 8:
        return q8.astype(np.float64) * np.repeat(np.ascontiguousarray(d8, np.uint16).view(np.float16).astype(np.float64), 32, axis=-1)
    return qk.astype(np.float64) * np.repeat(np.asarray(dk, np.float64), 256, axis=-1)


def dot64(a, b, x64):
    return (x64 @ (a - b).T)


def bound_dot(qtype, k, a, b, x64):
    """|y - (a - b) . x| <= gamma(n) * sum_i (|a_i| + |b_i|) |x_i| + floor.
    n = the f32 roundings on the longest chain a term goes through:
      Q8_0   the scale product d_w * d_x (1), sumi * scale (1), then the term is added in block 0 and every later block adds to it: k/32
             additions -> n = k/32 + 2;
      K      d * d_x (1), that times aux32[l] (1), one addition per super-block into sums[l] (k/256), then the eight final additions (8)
             -> n = k/256 + 10.  The min term (Q5_K) goes dmin * d_x (1), times sumi (1), k/256 subtractions, 8 additions: the same n.
    The integer sums are exact and below 2^24 in magnitude (Q6_K worst case 32 * 128 * 127 * 32 = 16.6e6), so their conversion is exact.
    floor: a scale product that lands in the subnormal range is off by up to 2^-150, times an integer below 2^24, once per block: k/32 * 2^-125;
    and 1e-12 of the magnitude for the float64 reference's own summation."""
    n = k // 32 + 2 if qtype == 8 else k // 256 + 10
    mag = np.abs(x64) @ (np.abs(a) + np.abs(b)).T
    return (gamma(n) + 1e-12) * mag + (k // 32) * 2.0 ** -125


# ---------------------------------------------------------------- RMSNorm, SwiGLU, loads, add ---------------------------------------------
def rmsnorm(x, g, eps, squares=F):
    """ggml_compute_forward_rms_norm_f32: f32 squares (they overflow to inf as ggml's do), summed in double in index order, mean cast to f32,
    scale = 1 / sqrtf(mean + eps), y = (x * scale) * g.  squares = np.float64 is the WRONG variant (products taken in double) that the
    cases must tell from the right one"""
    x = np.asarray(x, F); g = np.asarray(g, F)
    with np.errstate(over="ignore"):
        sq = (x.astype(squares) * x.astype(squares)).astype(np.float64)
        s = np.cumsum(sq, axis=-1)[..., -1]                  # cumsum adds strictly left to right
        mean = (s / float(x.shape[-1])).astype(F)
    scale = (F(1) / np.sqrt((mean + F(eps)).astype(F))).astype(F)
    return ((x * scale[..., None]).astype(F) * g).astype(F)


def rmsnorm64(x, g, eps):
    x = np.asarray(x, np.float64)
    return x / np.sqrt((x * x).mean(-1, keepdims=True) + float(F(eps))) * np.asarray(g, np.float64)


def squares_overflow(x):
    """rows of x whose f32 squares reach inf: ggml's (and the device's) norm is 0 there, by construction, and float64 has nothing to say"""
    with np.errstate(over="ignore"):
        return np.isinf(np.asarray(x, F) * np.asarray(x, F)).any(-1)


def bound_rmsnorm(x, g, eps):
    """|y - y64| <= gamma(6) |y64| + floor.  Chain of one output: the squares round once each (relative u on the sum), the double sum is
    exact to 1e-13, the mean's cast (1) and + eps (1) make 3 u under the square root, which halves them; the root (1) and the reciprocal (1)
    bring the scale to 3.5 u; x * scale (1) and * g (1): 5.5 u -> n = 6.
    floor: squares that underflow (|x| < 2^-75) are missing from the sum, at most d * 2^-149 against eps >= 1e-6: relative 1e-36, nothing;
    x * scale and the product with g may land in the subnormal range: 2^-149 (1 + |g|)"""
    y64 = rmsnorm64(x, g, eps)
    return gamma(6) * np.abs(y64) + TINY * (1 + np.abs(np.asarray(g, np.float64)))


def swiglu64(g, u):
    g = np.asarray(g, np.float64)
    return g / (1 + np.exp(-g)) * np.asarray(u, np.float64)


def bound_swiglu(g, u):
    """y = fl(fl(g / fl(1 + e)) * u), e = expf(-g) within one ulp = 2 u of exp(-g) (glibc states 0.502 ulp).  The error of e enters 1 + e
    with weight e / (1 + e) <= 1: 2 u; the addition, the division and the product round once each: 3 u -> n = 5 on |silu(g) u|.
    Two floors: where exp(-g) exceeds FLT_MAX, e is inf and the result is 0, while the true |silu(g) u| is below |g u| / FLT_MAX; and the
    quotient and the product may land in the subnormal range: 2^-149 (1 + |u|)."""
    g = np.asarray(g, np.float64); u = np.asarray(u, np.float64)
    fmax = float(np.finfo(np.float32).max)
    over = np.exp(np.minimum(-g, 700.0)) > fmax
    return gamma(5) * np.abs(swiglu64(g, u)) + np.where(over, np.abs(g * u) / fmax, 0.0) + TINY * (1 + np.abs(u))


def load_rows(x, rows, d):
    """k_gg_load_rows: h[t][0..d) = x[rows[t]][0..d), x [x_rows][x_stride]"""
    return np.ascontiguousarray(np.asarray(x, F)[np.asarray(rows, np.int64), :d])


def add(h, o):
    return (np.asarray(h, F) + np.asarray(o, F)).astype(F)
