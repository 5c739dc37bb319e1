"""float64 references for the talker / predictor linear layers (q3tts_op_linear) and the oracle compositions the GPU tests compare against bit
for bit.  Decoders are vectorised restatements of the public ggml block formats; tests/test_linear_plan_cpu.py checks them against ggml_ref.py.

Bounds (u = 2^-24, gamma(n) = n u / (1 - n u)); they hold while no f32 intermediate overflows and no f16 block scale overflows:
 (a) GEMM, given the int8 activations: |y_dev - W64 . (xq * f16(xd))| <= gamma(24) * A, A = sum_i (|a_i| + |b_i|) |x_i| with w_i = a_i - b_i the
     split of each weight into its scale term a and its min term b (b = 0 for Q8_0 / Q6_K).  24 roundings bound any term's chain: the scale
     product, the sub-block products and their difference (K-quants), 8 fma blocks per segment, 8 segment adds, 3 super-segment adds.
 (b) Norm: |xn - xn64| <= gamma(d/64 + 12) |xn64| + tiny (lane sum-of-squares chain d/64, butterfly 6, mean, eps, sqrt, reciprocal, two
     products); every xq is within 0.5 + 1e-3 of xn / (amax / 127) and xd == f16(amax / 127) of the block.
 (c) End to end (fused norm + GEMV): |y - W64 . xn64| <= sum_i |w_i| * 0.57 * dd_b(i) + gamma(24) A + sum_i |w_i| |xn_i - xn64_i|, where
     0.57 dd >= the quantisation error 0.5 dd + 127 dd 2^-11 (f16 rounding of the scale)."""
import ctypes as C

import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1 - n * U)


def f16(v):
    return np.asarray(v, np.float64).astype(np.float16).astype(np.float64)


# ---------------------------------------------------------------- decoders (float64, vectorised) ----------------------------------------------
def dec_q8_0(raw, n, k):
    """-> (a, b): w = a - b, shape [n][k]"""
    b = np.ascontiguousarray(raw).reshape(n, k // 32, 34)
    d = b[..., :2].copy().view(np.float16).astype(np.float64)
    q = b[..., 2:].copy().view(np.int8).astype(np.float64)
    a = (d * q).reshape(n, k)
    return a, np.zeros_like(a)


def _scale_min(scales):
    """scales [nb][12] u8 -> sc, m [nb][8]"""
    s = scales.astype(np.int64)
    sc = np.zeros(s.shape[:-1] + (8,), np.int64); m = np.zeros_like(sc)
    for j in range(8):
        if j < 4:
            sc[..., j] = s[..., j] & 63; m[..., j] = s[..., j + 4] & 63
        else:
            sc[..., j] = (s[..., j + 4] & 0xF) | ((s[..., j - 4] >> 6) << 4)
            m[..., j] = (s[..., j + 4] >> 4) | ((s[..., j] >> 6) << 4)
    return sc, m


def dec_q5_k(raw, n, k, wrong_min_sign=False):
    blk = np.ascontiguousarray(raw).reshape(n * (k // 256), 176)
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float64)[:, 0]
    dmin = blk[:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]
    sc, m = _scale_min(blk[:, 4:16])
    qh, qs = blk[:, 16:48].astype(np.int64), blk[:, 48:176].astype(np.int64)
    q = np.zeros((blk.shape[0], 8, 32), np.int64)
    for j in range(8):
        p = j // 2
        nib = (qs[:, 32 * p:32 * p + 32] >> (4 * (j & 1))) & 0xF
        q[:, j] = nib + 16 * ((qh >> j) & 1)
    a = (d[:, None] * sc)[:, :, None] * q
    b = np.broadcast_to((dmin[:, None] * m)[:, :, None], q.shape)
    if wrong_min_sign:
        b = -b
    return a.reshape(n, k), np.ascontiguousarray(b).reshape(n, k)


def dec_q6_k(raw, n, k):
    blk = np.ascontiguousarray(raw).reshape(n * (k // 256), 210)
    ql, qh = blk[:, 0:128].astype(np.int64), blk[:, 128:192].astype(np.int64)
    sc = blk[:, 192:208].copy().view(np.int8).astype(np.float64)
    d = blk[:, 208:210].copy().view(np.float16).astype(np.float64)[:, 0]
    y = np.zeros((blk.shape[0], 256))
    for h in range(2):
        L, H, S = ql[:, 64 * h:64 * h + 64], qh[:, 32 * h:32 * h + 32], sc[:, 8 * h:8 * h + 8]
        l = np.arange(32); is_ = l // 16
        q1 = ((L[:, :32] & 0xF) | (((H >> 0) & 3) << 4)) - 32
        q2 = ((L[:, 32:] & 0xF) | (((H >> 2) & 3) << 4)) - 32
        q3 = ((L[:, :32] >> 4) | (((H >> 4) & 3) << 4)) - 32
        q4 = ((L[:, 32:] >> 4) | (((H >> 6) & 3) << 4)) - 32
        for qq, off in ((q1, 0), (q2, 2), (q3, 4), (q4, 6)):
            y[:, 128 * h + 32 * (off // 2) + l] = d[:, None] * S[:, is_ + off] * qq
    y = y.reshape(n, k)
    return y, np.zeros_like(y)


def decode(raw, qtype, n, k):
    return {8: dec_q8_0, 13: dec_q5_k, 14: dec_q6_k}[qtype](raw, n, k)


def decode_parts(weights, k):
    """[(raw, type, rows)] -> (a, b) of the stacked matrix"""
    A, B = zip(*[decode(r, t, n, k) for r, t, n in weights])
    return np.concatenate(A), np.concatenate(B)


def dequant_act(xq, xd):
    return xq.astype(np.float64) * np.repeat(f16(xd.view(np.float16).astype(np.float32)), 32, axis=-1)


def bound_gemm(a, b, x):
    """(a): |y - (a - b) . x| <= gamma(24) * A"""
    return gamma(24) * ((np.abs(a) + np.abs(b)) @ np.abs(x).T).T


def bound_norm(xn64, d):
    return gamma(d // 64 + 12) * np.abs(xn64) + 1e-30


def rmsnorm64(h, g, eps):
    h = h.astype(np.float64)
    return h / np.sqrt((h * h).mean(-1, keepdims=True) + eps) * g.astype(np.float64)


def quant_check(xn, xq, xd):
    """(b): xd == f16(amax/127) and |xq - xn/dd| <= 0.5 + 1e-3, blockwise on the device's own xn"""
    nt, k = xn.shape
    blk = xn.astype(np.float32).reshape(nt, k // 32, 32)
    dd = np.abs(blk).max(-1) / np.float32(127)
    ok_d = np.array_equal(dd.astype(np.float16).view(np.uint16), xd.reshape(nt, k // 32))
    r = np.where(dd[..., None] > 0, blk.astype(np.float64) / np.where(dd > 0, dd, 1)[..., None], 0)
    return ok_d and np.abs(xq.reshape(nt, k // 32, 32) - r).max() <= 0.5 + 1e-3


def bound_e2e(w, xn64, xn_err, dd, a, b, x_deq):
    """(c) for y = W . dequant(quant(xn)): see the module docstring"""
    aw = np.abs(w)
    return (aw @ (0.57 * np.repeat(dd, 32, axis=-1)).T).T + bound_gemm(a, b, x_deq) + (aw @ np.abs(xn_err).T).T


def silu64(G):
    return 0.5 * G * (1 + np.tanh(0.5 * G))   # g * sigmoid(g) without overflow


def swiglu64(G, Uu):
    return silu64(G) * Uu


def bound_swiglu_e2e(G64, U64, eg, eu, ad):
    """(c) for gate/up + SwiGLU + quant, given the int8 inputs: |aq * f16(ad) - swiglu(G64, U64)| <= 0.57 dd (quantisation, dd <= f16(ad)
    (1 + 2^-10)) + 1.1 |u| eg + |silu(g)| eu + 1.1 eg eu + 0.25 |u| eg^2 (d silu / dg in [-0.1, 1.1], |silu''| <= 0.5) + 1e-5 |s|
    (the f32 evaluation of silu and the product)"""
    dd = np.repeat(f16(np.asarray(ad).view(np.float16).astype(np.float32)) * (1 + 2.0 ** -10), 32, axis=-1)
    silu = np.abs(silu64(G64))
    return 0.57 * dd + 1.1 * np.abs(U64) * eg + silu * eu + 1.1 * eg * eu + 0.25 * np.abs(U64) * eg * eg + 1e-5 * np.abs(swiglu64(G64, U64)) + 1e-30


# ---------------------------------------------------------------- argmax keys (kdev.h pack_key) -------------------------------------------------
def pack_key(v, idx):
    b = int(np.float32(v).view(np.uint32))
    if b == 0x80000000:
        b = 0
    ord_ = (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)
    return (ord_ << 32) | (~idx & 0xFFFFFFFF)


def key_code(k):
    return int(np.int32(np.uint32(~int(k) & 0xFFFFFFFF)))


def greedy_key(logits, mask, idx_add, armed):
    """first maximum with strict '>' over the rows with a logit > -inf (NaN never), the masked index skipped; no such row -> the armed key"""
    best, bi = None, -1
    for i, v in enumerate(logits):
        if i + idx_add == mask or not (v > -np.inf):
            continue
        if best is None or v > best:
            best, bi = v, i
    return armed if best is None else max(armed, pack_key(best, bi + idx_add))


# ---------------------------------------------------------------- oracle compositions (bit-exact bars) -------------------------------------------
def _slice_cols(raw, qtype, n, k, c0, c1):
    rb = {8: 34 * k // 32, 13: 176 * k // 256, 14: 210 * k // 256}[qtype]
    per = {8: 34 / 32, 13: 176 / 256, 14: 210 / 256}[qtype]
    r = np.ascontiguousarray(raw).reshape(n, rb)
    return np.ascontiguousarray(r[:, int(c0 * per):int(c1 * per)])


def oracle_slabs(L, weights, k, row0, nrows, xq, xd):
    """per super-segment partials [nsseg][ntok][nrows] of rows [row0, row0 + nrows): q3o_matvec on each 2048-column slice"""
    nt = xq.shape[0]
    nss = (k // 256 + 7) // 8
    out = np.zeros((nss, nt, nrows), np.float32)
    for s in range(nss):
        c0, c1 = 2048 * s, min(k, 2048 * (s + 1))
        rows = []
        for raw, t, n in weights:
            rows.append((_slice_cols(raw, t, n, k, c0, c1), t, n))
        for tok in range(nt):
            xs = np.ascontiguousarray(xq[tok, c0:c1]); ds = np.ascontiguousarray(xd[tok, c0 // 32:c1 // 32])
            ys = []
            for raw, t, n in rows:
                y = np.zeros(n, np.float32)
                L.q3o_matvec(t, raw.ctypes.data, n, c1 - c0, xs.ctypes.data, ds.ctypes.data, None, y.ctypes.data)
                ys.append(y)
            out[s, tok] = np.concatenate(ys)[row0:row0 + nrows]
    return out


def sum_slabs(sl):
    y = sl[0].copy()
    for s in range(1, sl.shape[0]):
        y = y + sl[s]
    return y


def oracle_float(L, w, wtype, k, row0, nrows, x):
    w = np.ascontiguousarray(w[row0:row0 + nrows])
    y = np.zeros((x.shape[0], nrows), np.float32)
    for t in range(x.shape[0]):
        xt = np.ascontiguousarray(x[t], np.float32)
        L.q3o_matvec(wtype, w.ctypes.data, nrows, k, None, None, xt.ctypes.data, y[t].ctypes.data)
    return y


def residual(h_rows, parts, nparts):
    """spec S9: y = P0; y += P1 ...; h = h_in + y (parts [nparts][ntok][K], already gathered)"""
    if nparts == 0:
        return h_rows.astype(np.float32).copy()
    y = parts[0].astype(np.float32).copy()
    for s in range(1, nparts):
        y = y + parts[s]
    return h_rows.astype(np.float32) + y


def oracle_norm(L, h, g, eps):
    """-> xn, xq, xd of every row of h (q3o_rmsnorm + q3o_quant_act)"""
    nt, k = h.shape
    xn = np.zeros((nt, k), np.float32); xq = np.zeros((nt, k), np.int8); xd = np.zeros((nt, k // 32), np.uint16)
    g = np.ascontiguousarray(g, np.float32)
    for t in range(nt):
        ht = np.ascontiguousarray(h[t], np.float32)
        L.q3o_rmsnorm(ht.ctypes.data, g.ctypes.data, k, C.c_float(eps), xn[t].ctypes.data)
        L.q3o_quant_act(xn[t].ctypes.data, k, xq[t].ctypes.data, xd[t].ctypes.data)
    return xn, xq, xd


def oracle_swiglu_quant(L, G, Uu):
    L.q3o_spec_swiglu_vec.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    nt, ff = G.shape
    act = np.zeros((nt, ff), np.float32); aq = np.zeros((nt, ff), np.int8); ad = np.zeros((nt, ff // 32), np.uint16)
    for t in range(nt):
        g = np.ascontiguousarray(G[t], np.float32); u = np.ascontiguousarray(Uu[t], np.float32)
        L.q3o_spec_swiglu_vec(g.ctypes.data, u.ctypes.data, ff, act[t].ctypes.data)
        L.q3o_quant_act(act[t].ctypes.data, ff, aq[t].ctypes.data, ad[t].ctypes.data)
    return act, aq, ad


def rand_rows(rng, qtype, n, k, scale=1.0):
    """n rows of k weights as raw GGUF blocks with RANDOM fields (every bit pattern of quants, scales and mins is a valid block)"""
    nsb = n * (k // 256)
    f16u = lambda lo, hi, m: (rng.uniform(lo * scale, hi * scale, m).astype(np.float16)).view(np.uint16).view(np.uint8).reshape(-1, 2)
    if qtype == 8:
        blk = rng.integers(0, 256, (n * (k // 32), 34), dtype=np.uint8)
        blk[:, :2] = f16u(0.001, 0.05, n * (k // 32))
        return blk.reshape(-1)
    if qtype == 13:  # {f16 d, dmin; u8 scales[12]; u8 qh[32]; u8 qs[128]}
        blk = rng.integers(0, 256, (nsb, 176), dtype=np.uint8)
        blk[:, 0:2] = f16u(0.0005, 0.01, nsb); blk[:, 2:4] = f16u(0.0005, 0.01, nsb)
        return blk.reshape(-1)
    blk = rng.integers(0, 256, (nsb, 210), dtype=np.uint8)  # {u8 ql[128]; u8 qh[64]; i8 scales[16]; f16 d}
    blk[:, 208:210] = f16u(0.0002, 0.004, nsb)
    return blk.reshape(-1)
