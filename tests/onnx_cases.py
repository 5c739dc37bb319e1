"""Case tables of tests/test_gpu_onnx_products.py: every product kernel of the ONNX executor (csrc/onnx_exec.hip) at its tile edges, operand
layouts and on both kernel families, with a float64 reference and a bound derived from the kernel's own chain.  No rtol / atol pairs.

u = 2^-24, gamma(n) = n u / (1 - n u).  `abs_sum` below is the same operation applied to the absolute values of its operands (and |bias|).
  MatMul / Gemm     k_mm_mfma (M >= 16 and N >= 16) and k_matmul (otherwise, or everywhere under Q3_ONNX_NAIVE=1) accumulate K products in f32
                    (mfma steps or an fmaf chain, K roundings at most), then alpha * acc, beta * c and one add:
                    gamma(K + 3) (|alpha| sum_k |a_k b_k| + |beta c|).
  Conv1d, fast      the same GEMM over K = C kw with the bias as c: gamma(C kw + 3) abs_sum.
  ConvTranspose1d,  a GEMM over C into per-tap columns, then k_col2im1d adds at most ceil(kw / s) taps to the bias:
    fast            gamma(C + ceil(kw / s) + 2) abs_sum.
  k_conv2d,         an fmaf chain over terms = (C / g) kh kw products that starts from the bias: gamma(terms + 1) abs_sum.
  k_convtr2d
`fast` is which side of mm_fast_ok(M, N, K) a case lies on, computed from its shape exactly as the executor does: M, N, K of the GEMM the
operator becomes (Conv1d: M, OW, C kw; ConvTranspose1d: M kw, W, C), both >= 16, one spatial dimension and group 1.  Where the session's
launch counter can tell the two families apart (a fast transposed convolution is two launches, a direct one is one; a partial batch
broadcast adds one Expand copy) `launches` says so and the test asserts it; MatMul, Gemm and Conv are one launch on either side.

Row kernels (one 256-thread workgroup per row; thread t takes columns t, t + 256, ..., then an 8-level tree).  L = ceil(cols / 256):
  sums              a thread chain of L adds, 8 tree levels, and up to 2 more roundings (the product of a squared sum, the final divide
                    or root): gamma(L + 10) sum |x| (sum x^2 for the squared sums; ReduceL2 is the root of that, bound gamma(L + 10) sqrt(S)).
  ReduceProd        cols - 1 inexact products in whatever order: gamma(cols) |prod|, on values in [0.9, 1.1].
  ReduceLogSumExp   m + ln S, S = sum exp(x - m) >= 1: x - m rounds (u |x - m|, scaled by the term's share of S), expf is within 1 ulp (2u),
                    the sum adds gamma(L + 8), logf 2u |ln S|, the last add u |result|.
  Max / Min / Arg*  exact.
  Softmax           y_i = e_i / S with e_i = exp(x_i - m) (m exact): e_i carries eps_i = 2u + u |x_i - m| relatively, S carries
                    sum_j e_j eps_j / S + gamma(L + 8), the divide u:  |dy_i| <= y_i (eps_i + dS + u) + 2^-126 (a result below the normal
                    range may flush).  LogSoftmax: u |x_i - m| + dS + 2u |ln S| + u |y_i|.
  Normalisations    mean = sum / cols: |dmean| <= gamma(L + 9) sum |x| / cols.  d_i = x_i - mean: |dd_i| <= |dmean| + u |d_i| -- this is where
                    a mean of 1000 costs 1000 gamma(L + 9) against a spread of 1, and why the bound is not a relative one.
                    var = sum d^2 / cols: |dvar| <= (2 sum |d| dd + sum dd^2) / cols + gamma(L + 10) var.  inv = 1 / sqrt(var + eps):
                    |dinv| <= inv (|dvar| / (2 (var + eps)) + 4u).  y = d inv g + b: |dy| <= |g| (dd inv + |d| dinv) + 3u (|d inv g| + |b|).
                    A one-pass variance (E x^2 - mean^2) at mean 1000 errs by about 1e6 gamma(L) / var ~ 0.4 in y: far outside.
  LpNormalization   x / norm with the norm from the sums above: |y| (gamma(L + 10) + u).
  CumSum            a serial chain per row: gamma(cols) sum |x| (prefix sums are bounded by the running sum of |x|, so by the whole one)."""
import os
import sys

import numpy as np

import onnx_writer as W

U = 2.0 ** -24
F32, I64 = W.F32, W.I64


def gamma(n):
    return n * U / (1 - n * U)


class Case:
    def __init__(self, name, nodes, inits, feeds, ref, bound, family, fast=None, launches=None, naive_bound=None, naive_launches=None, opset=17, out="y"):
        self.name, self.nodes, self.inits, self.feeds, self.out, self.opset = name, nodes, inits, feeds, out, opset
        self.ref, self.bound, self.family, self.fast, self.launches = ref, bound, family, fast, launches
        self.naive_bound = bound if naive_bound is None else naive_bound
        self.naive_launches = launches if naive_launches is None else naive_launches


def _rng(name):
    return np.random.default_rng(abs(hash_name(name)) % (1 << 32))


def hash_name(name):
    h = 2166136261
    for ch in name.encode():
        h = ((h ^ ch) * 16777619) & 0xFFFFFFFF
    return h


def _f(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def mm_fast(M, N, K):
    return M >= 16 and N >= 16 and K >= 1


# ------------------------------------------------------------------------------------------------------------------ MatMul / Gemm
TRIPLES = [(15, 15, 1), (16, 16, 15), (17, 17, 16), (63, 63, 17), (64, 64, 31), (65, 65, 32), (128, 128, 33), (15, 64, 48),
           (16, 128, 1), (17, 15, 15), (63, 16, 16), (64, 17, 17), (65, 63, 31), (128, 65, 32), (64, 128, 33), (128, 64, 48),
           (16, 17, 16), (65, 16, 1), (15, 128, 32), (128, 15, 17), (63, 65, 48), (17, 63, 33), (64, 16, 15), (16, 64, 31),
           (1, 64, 17), (16, 128, 1), (64, 64, 16), (128, 128, 32)]          # the last four are pinned to a layout below
SCALES = (0.0, 1.0, -0.5, 2.0)
BIAS_KINDS = ("scalar", "n", "1n", "m1", "mn", None)


def _gemm_case(i, M, N, K, layout, bias_kind, alpha, beta):
    name = "gemm%02d_%dx%dx%d_%s_bias-%s_a%g_b%g" % (i, M, N, K, ("rm", "tA", "tB", "tAtB")[layout], bias_kind, alpha, beta)
    rng = _rng(name)
    ta, tb = layout & 1, layout >> 1
    a, b = _f(rng, M, K), _f(rng, K, N)
    A, B = (a.T.copy() if ta else a), (b.T.copy() if tb else b)
    feeds, ins = {"A": A, "B": B}, ["A", "B"]
    c = None
    if bias_kind is not None:
        c = _f(rng, *{"scalar": (), "n": (N,), "1n": (1, N), "m1": (M, 1), "mn": (M, N)}[bias_kind])
        ins.append("C")
    inits = [W.tensor("C", c)] if c is not None else []
    attrs = [W.attr_int("transA", ta), W.attr_int("transB", tb), W.attr_float("alpha", alpha), W.attr_float("beta", beta)]
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    al, be = float(np.float32(alpha)), float(np.float32(beta))
    ref, mag = al * (a64 @ b64), abs(al) * (np.abs(a64) @ np.abs(b64))
    if c is not None:
        ref, mag = ref + be * c.astype(np.float64), mag + abs(be) * np.abs(c.astype(np.float64))
    return Case(name, [W.node("Gemm", ins, ["y"], attrs=attrs)], inits, feeds, ref, gamma(K + 3) * mag,
                "k_mm_mfma" if mm_fast(M, N, K) else "k_matmul", fast=mm_fast(M, N, K), launches=1)


def gemm_cases():
    out = []
    for i, (M, N, K) in enumerate(TRIPLES):
        layout = i % 4
        if i == 24: layout = 1      # transA with A.shape[1] == 1: a_m == a_k == 1 (k_matmul side, M = 1)
        if i == 25: layout = 2      # transB with K == 1: b_k == b_n == 1 on the k_mm_mfma side; row-major K == 1 (case 8) has a_m == a_k == 1 there
        if i == 26: layout = 3      # aligned 64 tile, K == 16: the prefetch branch is never taken
        if i == 27: layout = 0      # aligned 128, K == 32: taken exactly once
        out.append(_gemm_case(i, M, N, K, layout, BIAS_KINDS[i % 6], SCALES[(i + 1) % 4], SCALES[(i // 4 + 1) % 4]))
    return out


def _matmul_case(name, ashape, bshape, launches=1):
    rng = _rng(name)
    a, b = _f(rng, *ashape), _f(rng, *bshape)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ref, mag = np.matmul(a64, b64), np.matmul(np.abs(a64), np.abs(b64))
    M = 1 if len(ashape) == 1 else ashape[-2]
    N = 1 if len(bshape) == 1 else bshape[-1]
    K = ashape[-1]
    fast = mm_fast(M, N, K)
    return Case(name, [W.node("MatMul", ["A", "B"], ["y"])], [], {"A": a, "B": b}, ref, gamma(K + 3) * mag, "k_mm_mfma" if fast else "k_matmul",
                fast=fast, launches=launches)


def matmul_cases():
    out = []
    for tag, (M, N, K) in (("fast", (17, 65, 33)), ("slow", (5, 70, 20))):
        out += [_matmul_case("matmul_%s_plain" % tag, (M, K), (K, N)),
                _matmul_case("matmul_%s_equal_batches" % tag, (2, 3, M, K), (2, 3, K, N)),
                _matmul_case("matmul_%s_A_broadcast_2d" % tag, (M, K), (2, 3, K, N)),                 # batch stride 0 on A
                _matmul_case("matmul_%s_A_broadcast_ones" % tag, (1, 1, M, K), (2, 3, K, N)),
                _matmul_case("matmul_%s_B_broadcast_2d" % tag, (2, 3, M, K), (K, N)),                 # batch stride 0 on B
                _matmul_case("matmul_%s_partial_broadcast" % tag, (1, 3, M, K), (2, 3, K, N), launches=2),   # the expand path: one copy more
                _matmul_case("matmul_%s_partial_broadcast_B" % tag, (2, 3, M, K), (2, 1, K, N), launches=2)]
    out += [_matmul_case("matmul_vec_A", (33,), (3, 33, 65)), _matmul_case("matmul_vec_B", (3, 17, 33), (33,)),
            _matmul_case("matmul_vec_both", (48,), (48,)), _matmul_case("matmul_vec_A_2d", (16,), (16, 64))]
    return out


# ------------------------------------------------------------------------------------------------------------------ convolutions
def _pads_same(inp, k, s, d, upper):
    eff = (k - 1) * d + 1
    o = -(-inp // s)
    tot = max(0, (o - 1) * s + eff - inp)
    pb = tot // 2 if upper else tot - tot // 2
    return pb, tot - pb


def conv_ref(x, w, b, strides, dils, pb, pe, groups):
    """float64 cross-correlation of ONNX Conv, x [N][C][*sp], w [M][C / g][*k]; explicit begin / end pads per spatial axis"""
    import torch
    import torch.nn.functional as F
    sp = x.ndim - 2
    xt = torch.from_numpy(np.asarray(x, np.float64))
    pad = []
    for d in reversed(range(sp)):
        pad += [pb[d], pe[d]]
    xt = F.pad(xt, pad)
    fn = F.conv1d if sp == 1 else F.conv2d
    y = fn(xt, torch.from_numpy(np.asarray(w, np.float64)), None if b is None else torch.from_numpy(np.asarray(b, np.float64)), stride=tuple(strides),
           dilation=tuple(dils), groups=groups)
    return y.numpy()


def convtr_ref(x, w, b, strides, dils, pb, out_sp, groups):
    """float64 ONNX ConvTranspose, w [C][M / g][*k]: the full overlap-add, then output index t is full index t + pb (zeros past the end)"""
    import torch
    import torch.nn.functional as F
    sp = x.ndim - 2
    fn = F.conv_transpose1d if sp == 1 else F.conv_transpose2d
    y = fn(torch.from_numpy(np.asarray(x, np.float64)), torch.from_numpy(np.asarray(w, np.float64)), None, stride=tuple(strides), dilation=tuple(dils),
           groups=groups).numpy()
    for d in range(sp):
        ax = 2 + d
        need = pb[d] + out_sp[d]
        if y.shape[ax] < need:
            padw = [(0, 0)] * y.ndim
            padw[ax] = (0, need - y.shape[ax])
            y = np.pad(y, padw)
        y = np.take(y, np.arange(pb[d], need), axis=ax)
    if b is not None:
        y = y + np.asarray(b, np.float64).reshape((1, -1) + (1,) * sp)
    return y


def _conv_case(name, N, C, sp_in, M, ks, strides=None, dils=None, pads=None, auto_pad=None, bias=True, groups=1):
    rng = _rng(name)
    sp = len(sp_in)
    strides, dils = list(strides or [1] * sp), list(dils or [1] * sp)
    x, w = _f(rng, N, C, *sp_in), _f(rng, M, C // groups, *ks)
    b = _f(rng, M) if bias else None
    attrs = [W.attr_ints("strides", strides), W.attr_ints("dilations", dils), W.attr_int("group", groups), W.attr_ints("kernel_shape", ks)]
    if auto_pad in ("SAME_UPPER", "SAME_LOWER"):
        pp = [_pads_same(sp_in[d], ks[d], strides[d], dils[d], auto_pad == "SAME_UPPER") for d in range(sp)]
        pb, pe = [p[0] for p in pp], [p[1] for p in pp]
        attrs.append(W.attr_str("auto_pad", auto_pad))
    elif auto_pad == "VALID":
        pb, pe = [0] * sp, [0] * sp
        attrs.append(W.attr_str("auto_pad", "VALID"))
    else:
        pads = list(pads or [0] * (2 * sp))
        pb, pe = pads[:sp], pads[sp:]
        attrs.append(W.attr_ints("pads", pads))
    ref = conv_ref(x, w, b, strides, dils, pb, pe, groups)
    mag = conv_ref(np.abs(x), np.abs(w), None if b is None else np.abs(b), strides, dils, pb, pe, groups)
    terms = (C // groups) * int(np.prod(ks))
    fast = sp == 1 and groups == 1 and mm_fast(M, ref.shape[-1], C * ks[0])
    direct = gamma(terms + 1) * mag
    inits = [W.tensor("w", w)] + ([W.tensor("b", b)] if bias else [])
    return Case(name, [W.node("Conv", ["x", "w"] + (["b"] if bias else []), ["y"], attrs=attrs)], inits, {"x": x}, ref,
                gamma(terms + 3) * mag if fast else direct, "conv1d_mfma" if fast else "k_conv2d", fast=fast, launches=1, naive_bound=direct)


def conv1d_cases():
    c = _conv_case
    return [
        c("conv1d_K1_M16_OW64", 1, 1, [64], 16, [1]),
        c("conv1d_K15_M15_OW15_direct", 3, 5, [17], 15, [3], bias=False),                        # M < 16: the direct kernel
        c("conv1d_K16_M16_OW16", 1, 16, [16], 16, [1]),
        c("conv1d_K17_M64_OW17_b3", 3, 1, [33], 64, [17]),
        c("conv1d_K35_M65_OW65", 1, 5, [71], 65, [7], bias=False),
        c("conv1d_K15_M64_OW15_direct", 1, 5, [17], 64, [3]),                                    # OW < 16: the direct kernel
        c("conv1d_K15_M16_OW16_threshold", 1, 5, [18], 16, [3]),                                 # the smallest fast shape at K = 15
        c("conv1d_left_pad_past_reach", 3, 4, [20], 16, [3], pads=[10, 0]),                      # outputs 0..7 read only padding
        c("conv1d_right_pad_past_W", 1, 3, [14], 16, [5], pads=[0, 9], bias=False),
        c("conv1d_stride_above_kw", 1, 5, [64], 64, [3], strides=[4]),
        c("conv1d_dilation_span_above_W", 1, 2, [12], 16, [3], dils=[9], pads=[12, 12]),
        c("conv1d_W10_OW16", 3, 5, [10], 65, [3], pads=[4, 4]),
        c("conv1d_same_upper", 1, 3, [33], 16, [4], strides=[2], auto_pad="SAME_UPPER"),
        c("conv1d_same_lower", 1, 3, [33], 16, [4], strides=[2], auto_pad="SAME_LOWER", bias=False),
        c("conv1d_valid_K35_M15_direct", 1, 7, [68], 15, [5], auto_pad="VALID"),
        c("conv1d_valid_K35_M16_OW64", 1, 7, [68], 16, [5], auto_pad="VALID"),
    ]


def _convtr_case(name, N, C, sp_in, Mg, ks, strides=None, dils=None, pads=None, opad=None, oshape=None, auto_pad=None, bias=True, groups=1):
    rng = _rng(name)
    sp = len(sp_in)
    strides, dils = list(strides or [1] * sp), list(dils or [1] * sp)
    opad = list(opad or [0] * sp)
    M = Mg * groups
    x, w = _f(rng, N, C, *sp_in), _f(rng, C, Mg, *ks)
    b = _f(rng, M) if bias else None
    attrs = [W.attr_ints("strides", strides), W.attr_ints("dilations", dils), W.attr_int("group", groups), W.attr_ints("kernel_shape", ks)]
    if any(opad):
        attrs.append(W.attr_ints("output_padding", opad))
    eff = [(ks[d] - 1) * dils[d] + 1 for d in range(sp)]
    if oshape is not None or auto_pad in ("SAME_UPPER", "SAME_LOWER"):
        out_sp = list(oshape) if oshape is not None else [sp_in[d] * strides[d] for d in range(sp)]
        tot = [max(0, (sp_in[d] - 1) * strides[d] + opad[d] + eff[d] - out_sp[d]) for d in range(sp)]
        pb = [t // 2 if auto_pad == "SAME_UPPER" else t - t // 2 for t in tot]
        if oshape is not None:
            attrs.append(W.attr_ints("output_shape", out_sp))
        if auto_pad:
            attrs.append(W.attr_str("auto_pad", auto_pad))
    else:
        pads = list(pads or [0] * (2 * sp))
        pb = pads[:sp]
        out_sp = [(sp_in[d] - 1) * strides[d] - pads[d] - pads[sp + d] + eff[d] + opad[d] for d in range(sp)]
        attrs.append(W.attr_ints("pads", pads))
    ref = convtr_ref(x, w, b, strides, dils, pb, out_sp, groups)
    mag = convtr_ref(np.abs(x), np.abs(w), None if b is None else np.abs(b), strides, dils, pb, out_sp, groups)
    fast = sp == 1 and groups == 1 and mm_fast(M * ks[0], sp_in[0], C)
    terms = (C // groups) * int(np.prod(ks))
    direct = gamma(terms + 1) * mag
    inits = [W.tensor("w", w)] + ([W.tensor("b", b)] if bias else [])
    return Case(name, [W.node("ConvTranspose", ["x", "w"] + (["b"] if bias else []), ["y"], attrs=attrs)], inits, {"x": x}, ref,
                gamma(C + -(-ks[0] // strides[0]) + 2) * mag if fast else direct, "convtr1d_mfma+col2im" if fast else "k_convtr2d", fast=fast,
                launches=2 if fast else 1, naive_bound=direct, naive_launches=1)


def convtr1d_cases():
    c = _convtr_case
    return [
        c("convtr1d_stride_eq_kw_W16", 1, 8, [16], 4, [4], strides=[4]),                         # no overlap
        c("convtr1d_stride_above_kw_W17", 3, 8, [17], 8, [2], strides=[3], bias=False),          # gaps that only the bias fills
        c("convtr1d_stride1_W17", 1, 16, [17], 16, [3]),
        c("convtr1d_kw1_W16", 1, 5, [16], 16, [1], strides=[2]),
        c("convtr1d_output_padding_W15_direct", 1, 6, [15], 8, [3], strides=[3], opad=[2]),      # W < 16: the direct kernel
        c("convtr1d_output_padding_W16", 3, 6, [16], 8, [3], strides=[3], opad=[2], pads=[1, 0]),
        c("convtr1d_output_shape_W16", 1, 4, [16], 8, [5], strides=[2], oshape=[33]),
        c("convtr1d_same_upper_W17", 1, 4, [17], 8, [5], strides=[2], auto_pad="SAME_UPPER"),
        c("convtr1d_same_lower_W17", 1, 4, [17], 8, [5], strides=[2], auto_pad="SAME_LOWER", bias=False),
        c("convtr1d_M2_kw8_fast", 1, 3, [17], 2, [8], strides=[4]),                              # M kw == 16
        c("convtr1d_M1_kw15_direct", 1, 3, [16], 1, [15], strides=[5]),                          # M kw == 15
        c("convtr1d_dilated_W16", 1, 7, [16], 4, [4], strides=[2], dils=[3], pads=[2, 3]),
    ]


def direct_cases():
    c, t = _conv_case, _convtr_case
    return [
        c("conv1d_depthwise", 3, 6, [40], 6, [5], pads=[2, 2], groups=6),
        c("conv1d_grouped_M_per_group_2", 1, 6, [40], 12, [3], strides=[2], pads=[1, 0], groups=6, bias=False),
        c("conv1d_grouped_large", 1, 32, [33], 32, [3], groups=2),                               # would be fast but for the groups
        c("conv2d_asymmetric", 3, 3, [9, 11], 5, [3, 2], strides=[2, 3], dils=[1, 2], pads=[1, 0, 2, 3]),
        c("conv2d_depthwise", 1, 4, [8, 8], 4, [3, 3], pads=[1, 1, 1, 1], groups=4, bias=False),
        c("conv2d_same_upper", 1, 2, [7, 10], 3, [4, 3], strides=[2, 2], auto_pad="SAME_UPPER"),
        t("convtr1d_depthwise", 3, 6, [20], 1, [4], strides=[2], pads=[1, 1], groups=6),
        t("convtr1d_grouped_M_per_group_2", 1, 6, [20], 2, [3], strides=[3], groups=3, bias=False),
        t("convtr2d_asymmetric", 3, 3, [5, 6], 4, [3, 2], strides=[2, 3], dils=[2, 1], pads=[1, 0, 2, 1], opad=[1, 2]),
        t("convtr2d_depthwise", 1, 4, [6, 5], 1, [3, 3], strides=[2, 2], pads=[1, 1, 1, 1], groups=4, bias=False),
    ]


def product_cases():
    cases = gemm_cases() + matmul_cases() + conv1d_cases() + convtr1d_cases() + direct_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert all(np.asarray(v).size < 100000 for v in c.feeds.values()) and c.ref.size < 100000, c.name
    return cases


# ------------------------------------------------------------------------------------------------------------------ row kernels
COLS = (1, 2, 255, 256, 257, 511, 513, 1000)
REDUCE_OPS = ("ReduceSum", "ReduceMean", "ReduceMax", "ReduceMin", "ReduceProd", "ReduceL2", "ReduceSumSquare", "ReduceL1", "ReduceLogSumExp")


def _levels(cols):
    return -(-cols // 256)


def reduce_ref(op, x, axes, keep):
    """(float64 result, bound) of one Reduce* over `axes` (a tuple) of x (float64)"""
    cols = int(np.prod([x.shape[a] for a in axes]))
    g = gamma(_levels(cols) + 10)
    kw = dict(axis=axes, keepdims=bool(keep))
    ax = np.abs(x)
    if op == "ReduceSum": return x.sum(**kw), g * ax.sum(**kw)
    if op == "ReduceMean": return x.mean(**kw), g * ax.sum(**kw) / cols
    if op == "ReduceMax": return x.max(**kw), 0.0
    if op == "ReduceMin": return x.min(**kw), 0.0
    if op == "ReduceProd": return x.prod(**kw), gamma(cols) * ax.prod(**kw)
    if op == "ReduceL2": return np.sqrt((x * x).sum(**kw)), g * np.sqrt((x * x).sum(**kw))
    if op == "ReduceSumSquare": return (x * x).sum(**kw), g * (x * x).sum(**kw)
    if op == "ReduceL1": return ax.sum(**kw), g * ax.sum(**kw)
    if op == "ReduceLogSumExp":
        m = x.max(axis=axes, keepdims=True)
        e = np.exp(x - m)
        S = e.sum(axis=axes, keepdims=True)
        r = m + np.log(S)
        b = (e * U * np.abs(x - m)).sum(axis=axes, keepdims=True) / S + 2 * U + gamma(_levels(cols) + 8) + 2 * U * np.abs(np.log(S)) + U * np.abs(r)
        if not keep:
            r, b = np.squeeze(r, axis=axes), np.squeeze(b, axis=axes)
        return r, b
    raise KeyError(op)


def _reduce_graph(name, x, axes, keep, form, opset, family="k_reduce_rows"):
    """all nine Reduce* ops over the same axes in one graph.  form: 'attr' (axes attribute, ReduceSum takes the input from opset 13 on) or 'input'"""
    nodes, inits, ref, bound = [], [W.tensor("axes", np.asarray(axes, np.int64))], {}, {}
    x64 = x.astype(np.float64)
    for op in REDUCE_OPS:
        xin = "xp" if op == "ReduceProd" else "x"
        as_input = form == "input" or (op == "ReduceSum" and opset >= 13)
        attrs = [W.attr_int("keepdims", keep)] + ([] if as_input else [W.attr_ints("axes", axes)])
        nodes.append(W.node(op, [xin] + (["axes"] if as_input else []), ["y_" + op], attrs=attrs))
        src = (0.9 + 0.2 * (np.abs(x64) % 1.0)) if op == "ReduceProd" else x64
        ref["y_" + op], bound["y_" + op] = reduce_ref(op, src, tuple(a % x.ndim for a in axes), keep)
    xp = (0.9 + 0.2 * (np.abs(x64) % 1.0)).astype(np.float32)
    ref["y_ReduceProd"], bound["y_ReduceProd"] = reduce_ref("ReduceProd", xp.astype(np.float64), tuple(a % x.ndim for a in axes), keep)
    return Case(name, nodes, inits, {"x": x, "xp": xp}, ref, bound, family, opset=opset, out=list(ref))


def reduce_cases():
    out = []
    for i, cols in enumerate(COLS):
        rows = 3 + i % 3
        name = "reduce_last_cols%d" % cols
        out.append(_reduce_graph(name, 2 * _f(_rng(name), rows, cols), [-1], i % 2, "attr" if i % 2 else "input", 13 if i % 2 else 18))
    for shape, tag in (((4, 257, 3), "4x257x3"), ((16, 3, 16), "16x3x16")):
        for axes, what in (([0], "first"), ([1], "middle"), ([0, 2], "pair"), ([0, 1, 2], "all"), ([-1], "last")):
            for keep, form, opset in ((1, "attr", 13), (0, "input", 18)):
                name = "reduce_%s_%s_keep%d_opset%d" % (tag, what, keep, opset)
                out.append(_reduce_graph(name, 2 * _f(_rng(name), *shape), axes, keep, form, opset))
    # empty axes: reduce everything by default, pass through with noop_with_empty_axes
    name = "reduce_empty_axes"
    x = _f(_rng(name), 3, 257)
    x64 = x.astype(np.float64)
    r, b = reduce_ref("ReduceSum", x64, (0, 1), 1)
    nodes = [W.node("ReduceSum", ["x", "none"], ["y_all"], attrs=[W.attr_int("keepdims", 1)]),
             W.node("ReduceSum", ["x", "none"], ["y_noop"], attrs=[W.attr_int("keepdims", 1), W.attr_int("noop_with_empty_axes", 1)])]
    out.append(Case(name, nodes, [W.tensor("none", np.zeros((0,), np.int64))], {"x": x}, {"y_all": r, "y_noop": x64}, {"y_all": b, "y_noop": 0.0},
                    "k_reduce_rows", opset=18, out=["y_all", "y_noop"]))
    return out


def arg_cases():
    out = []
    for cols in (600, 257):
        name = "arg_cols%d" % cols
        rng = _rng(name)
        x = _f(rng, 7, cols)
        x[0, 7] = x[0, 263 % cols] = 10.0                 # ties at c and c + 256: one thread sees both (cols 257: columns 7 and 6)
        x[1, 100] = x[1, 101] = 10.0                      # neighbouring threads
        x[2, cols - 1] = 10.0                             # the maximum in the last column
        x[3, :] = 3.0                                     # all equal
        x[4, :] = -np.inf
        x[5, 0] = x[5, 256] = x[5, cols - 1] = 10.0       # column 0 and 256 are thread 0's first two
        nodes, ref = [], {}
        for op, sign in (("ArgMax", 1.0), ("ArgMin", -1.0)):
            feed = "x" if sign > 0 else "xn"
            for last in (0, 1):
                for keep in (0, 1):
                    o = "y_%s_last%d_keep%d" % (op, last, keep)
                    nodes.append(W.node(op, [feed], [o], attrs=[W.attr_int("axis", 1), W.attr_int("keepdims", keep), W.attr_int("select_last_index", last)]))
                    r = (cols - 1 - np.argmax(x[:, ::-1], axis=1)) if last else np.argmax(x, axis=1)
                    ref[o] = r.reshape(-1, 1) if keep else r
        out.append(Case(name, nodes, [], {"x": x, "xn": -x}, ref, {k: 0.0 for k in ref}, "k_reduce_rows(arg)", out=list(ref)))
    return out


def softmax_ref(x, axis, log):
    m = x.max(axis=axis, keepdims=True)
    d = x - m
    e = np.exp(d)
    S = e.sum(axis=axis, keepdims=True)
    cols = x.shape[axis]
    fin = np.isfinite(d)
    eps = np.where(fin, 2 * U + U * np.abs(np.where(fin, d, 0.0)), 0.0)
    dS = (e * eps).sum(axis=axis, keepdims=True) / S + gamma(_levels(cols) + 8)
    if log:
        y = d - np.log(S)
        b = np.where(fin, U * np.abs(np.where(fin, d, 0.0)) + dS + 2 * U * np.abs(np.log(S)) + U * np.abs(np.where(fin, y, 0.0)), 0.0)
        return y, b
    y = e / S
    return y, np.where(fin, y * (eps + dS + U) + 2.0 ** -126, 0.0)


def softmax_cases():
    out = []
    for cols in COLS:
        for axis, shape in ((-1, (4, cols)), (1, (3, cols, 2))):
            name = "softmax_cols%d_axis%d" % (cols, axis)
            rng = _rng(name)
            x = 30 * _f(rng, *shape)
            if cols >= 3:                                   # rows 1 and 3 (axis -1) / slice 1 (middle axis): a third of the entries masked
                mask = rng.random(shape) < 1 / 3
                keepone = np.zeros(shape, bool)
                np.put_along_axis(keepone, np.argmax(x, axis=axis, keepdims=True), True, axis=axis)
                sel = np.zeros(shape, bool)
                sel[1::2] = True
                x[mask & sel & ~keepone] = -np.inf
            x64 = x.astype(np.float64)
            nodes = [W.node("Softmax", ["x"], ["y_sm"], attrs=[W.attr_int("axis", axis)]), W.node("LogSoftmax", ["x"], ["y_lsm"], attrs=[W.attr_int("axis", axis)])]
            (r0, b0), (r1, b1) = softmax_ref(x64, axis, False), softmax_ref(x64, axis, True)
            out.append(Case(name, nodes, [], {"x": x}, {"y_sm": r0, "y_lsm": r1}, {"y_sm": b0, "y_lsm": b1}, "k_softmax_rows", out=["y_sm", "y_lsm"]))
    return out


def norm_ref(x, eps, g, b):
    """rows of x [rows][cols] normalised; g, b broadcastable to x (or None) -> (y, bound)"""
    cols = x.shape[1]
    L = _levels(cols)
    mean = x.mean(axis=1, keepdims=True)
    dmean = gamma(L + 9) * np.abs(x).sum(axis=1, keepdims=True) / cols
    d = x - mean
    dd = dmean + U * np.abs(d)
    var = (d * d).mean(axis=1, keepdims=True)
    dvar = (2 * (np.abs(d) * dd).sum(axis=1, keepdims=True) + (dd * dd).sum(axis=1, keepdims=True)) / cols + gamma(L + 10) * var
    inv = 1 / np.sqrt(var + eps)
    dinv = inv * (dvar / (2 * (var + eps)) + 4 * U)
    g = np.ones_like(x) if g is None else np.broadcast_to(g, x.shape)
    b = np.zeros_like(x) if b is None else np.broadcast_to(b, x.shape)
    y = d * inv * g + b
    return y, np.abs(g) * (dd * inv + np.abs(d) * dinv) + 3 * U * (np.abs(d * inv * g) + np.abs(b))


def norm_cases():
    out = []
    for cols in COLS:
        name = "norm_cols%d" % cols
        rng = _rng(name)
        eps = 1e-5
        e32 = float(np.float32(eps))
        # LayerNormalization over the last axis: [4][cols], rows 2 and 3 at mean 1000, variance 1
        x = _f(rng, 4, cols)
        x[2:] += 1000.0
        g, b = _f(rng, cols), _f(rng, cols)
        ln, lnb = norm_ref(x.astype(np.float64), e32, g.astype(np.float64)[None], b.astype(np.float64)[None])
        # InstanceNormalization [2][3][cols]; GroupNormalization [2][4][cols] in 2 groups (cols of the kernel = 2 cols), per-channel affine
        xi = _f(rng, 2, 3, cols)
        xi[1] += 1000.0
        gi, bi = _f(rng, 3), _f(rng, 3)
        inn, innb = norm_ref(xi.astype(np.float64).reshape(6, cols), e32, np.tile(gi.astype(np.float64), 2)[:, None], np.tile(bi.astype(np.float64), 2)[:, None])
        xg = _f(rng, 2, 4, cols)
        xg[1] += 1000.0
        gg, bg = _f(rng, 4), _f(rng, 4)
        gfull = np.repeat(np.tile(gg.astype(np.float64), 2).reshape(4, 2), cols, axis=1)      # rows = (n, group), columns = (channel in group, pos)
        bfull = np.repeat(np.tile(bg.astype(np.float64), 2).reshape(4, 2), cols, axis=1)
        gn0, gnb0 = norm_ref(xg.astype(np.float64).reshape(4, 2 * cols), e32, None, None)
        gn = gn0 * gfull + bfull                                                              # the affine runs as two more kernels: Mul, Add
        gnb = np.abs(gfull) * gnb0 + 2 * U * (np.abs(gn0 * gfull) + np.abs(bfull)) + U * np.abs(gn)
        # LpNormalization p = 1, 2 over the last axis
        xl = _f(rng, 4, cols)
        xl64 = xl.astype(np.float64)
        l1, l2 = np.abs(xl64).sum(axis=1, keepdims=True), np.sqrt((xl64 * xl64).sum(axis=1, keepdims=True))
        gl = gamma(_levels(cols) + 10) + U
        nodes = [W.node("LayerNormalization", ["x", "g", "b"], ["y_ln"], attrs=[W.attr_int("axis", -1), W.attr_float("epsilon", eps)]),
                 W.node("InstanceNormalization", ["xi", "gi", "bi"], ["y_in"], attrs=[W.attr_float("epsilon", eps)]),
                 W.node("GroupNormalization", ["xg", "gg", "bg"], ["y_gn"], attrs=[W.attr_int("num_groups", 2), W.attr_float("epsilon", eps)]),
                 W.node("LpNormalization", ["xl"], ["y_l1"], attrs=[W.attr_int("axis", -1), W.attr_int("p", 1)]),
                 W.node("LpNormalization", ["xl"], ["y_l2"], attrs=[W.attr_int("axis", -1), W.attr_int("p", 2)])]
        inits = [W.tensor("g", g), W.tensor("b", b), W.tensor("gi", gi), W.tensor("bi", bi), W.tensor("gg", gg), W.tensor("bg", bg)]
        ref = {"y_ln": ln, "y_in": inn.reshape(xi.shape), "y_gn": gn.reshape(xg.shape), "y_l1": xl64 / l1, "y_l2": xl64 / l2}
        bound = {"y_ln": lnb, "y_in": innb.reshape(xi.shape), "y_gn": gnb.reshape(xg.shape), "y_l1": np.abs(xl64 / l1) * gl, "y_l2": np.abs(xl64 / l2) * gl}
        out.append(Case(name, nodes, inits, {"x": x, "xi": xi, "xg": xg, "xl": xl}, ref, bound, "k_norm_rows", opset=21, out=list(ref)))
    return out


def cumsum_cases():
    out = []
    for cols in (1, 2, 257):
        for axis, shape in ((-1, (3, cols)), (1, (2, cols, 3))):
            name = "cumsum_cols%d_axis%d" % (cols, axis)
            x = _f(_rng(name), *shape)
            x64 = x.astype(np.float64)
            nodes, ref, bound = [], {}, {}
            for ex in (0, 1):
                for rev in (0, 1):
                    o = "y_ex%d_rev%d" % (ex, rev)
                    nodes.append(W.node("CumSum", ["x", "ax"], [o], attrs=[W.attr_int("exclusive", ex), W.attr_int("reverse", rev)]))
                    v = np.flip(x64, axis) if rev else x64
                    c = np.cumsum(v, axis=axis)
                    if ex:
                        c = c - v
                    ref[o] = np.flip(c, axis) if rev else c
                    bound[o] = np.broadcast_to(gamma(cols) * np.abs(x64).sum(axis=axis, keepdims=True), x64.shape)
                    if ex:   # the exclusive prefix is a partial sum of the chain, not a difference: same bound
                        vv = np.concatenate([np.zeros_like(np.take(v, [0], axis=axis)), np.take(np.cumsum(v, axis=axis), np.arange(cols - 1), axis=axis)], axis=axis)
                        ref[o] = np.flip(vv, axis) if rev else vv
            out.append(Case(name, nodes, [W.tensor("ax", np.asarray(axis, np.int64))], {"x": x}, ref, bound, "k_cumsum_rows", out=list(ref)))
    return out


def row_cases():
    return reduce_cases() + arg_cases() + softmax_cases() + norm_cases() + cumsum_cases()


# ------------------------------------------------------------------------------------------------------------------ the operator zoo
# One tiny graph per operator name that the product and row tables do not reach (plus a few forms they leave out), for
# scripts/onnx_exec_digest.py: no reference, the outputs are pinned bit for bit in tests/golden/onnx_exec_digests.json.  Tensors hold at
# most 256 elements and have rank at most 4.  Feeds are device tensors; integer initialisers and float initialisers of at most 8 elements
# stay on the host, so `h*` operands below take the executor's host evaluators and the rest its kernels.
UNARY_OPS = ("Relu", "Sigmoid", "Tanh", "Exp", "Log", "Sqrt", "Reciprocal", "Neg", "Abs", "Sin", "Cos", "Erf", "Floor", "Ceil", "Round", "Sign", "Elu",
             "LeakyRelu", "HardSigmoid", "Gelu", "Softplus", "Selu", "Not", "Softsign", "HardSwish", "IsNaN", "Celu", "ThresholdedRelu", "Mish", "Tan",
             "Atan", "Sinh", "Cosh")
BINARY_OPS = ("Add", "Sub", "Mul", "Div", "Pow", "Min", "Max", "Equal", "Less", "Greater", "LessOrEqual", "GreaterOrEqual", "And", "Or", "Xor", "Mod",
              "PRelu", "Sum", "Mean")
OTHER_OPS = ("Identity", "Dropout", "Reshape", "Flatten", "Squeeze", "Unsqueeze", "Transpose", "Concat", "Slice", "Split", "Gather", "Shape", "Size",
             "Constant", "ConstantOfShape", "Range", "Cast", "Expand", "Tile", "Where", "Clip", "Softmax", "LogSoftmax", "LayerNormalization",
             "InstanceNormalization", "BatchNormalization", "MatMul", "Gemm", "Conv", "ConvTranspose", "Pad", "CumSum", "GlobalAveragePool",
             "GlobalMaxPool", "Trilu", "GatherElements", "ScatterND", "Resize", "GroupNormalization", "LpNormalization")
EXECUTABLE_OPS = UNARY_OPS + BINARY_OPS + REDUCE_OPS + ("ArgMax", "ArgMin") + OTHER_OPS     # 33 + 19 + 11 + 40 = 103 names
NOT_EXECUTABLE_OPS = ("LSTM", "GRU", "AveragePool", "SimplifiedLayerNormalization", "RMSNormalization", "NoSuchOp")


def _zoo(name, nodes, inits, feeds, outs, opset=17):
    assert all(np.asarray(v).size <= 256 and np.asarray(v).ndim <= 4 for v in feeds.values()), name
    return Case(name, nodes, inits, feeds, None, None, "zoo", opset=opset, out=list(outs))


def _i(name, v):
    return W.tensor(name, np.asarray(v, np.int64))


def _q(rng, *shape):
    """normals rounded to halves: exact zeros, ties for Round and equal pairs for the comparisons all occur"""
    return (np.round(2 * rng.standard_normal(shape)) / 2).astype(np.float32)


def _zoo_unary():
    attrs = {"Elu": [W.attr_float("alpha", 0.7)], "LeakyRelu": [W.attr_float("alpha", 0.1)], "HardSigmoid": [W.attr_float("alpha", 0.25), W.attr_float("beta", 0.4)],
             "Selu": [W.attr_float("alpha", 1.5), W.attr_float("gamma", 1.1)], "Gelu": [W.attr_str("approximate", "tanh")], "Celu": [W.attr_float("alpha", 1.5)],
             "ThresholdedRelu": [W.attr_float("alpha", 0.3)]}
    out = []
    for op in UNARY_OPS:
        name = "zoo_" + op
        rng = _rng(name)
        x = _q(rng, 2, 3, 4) + np.float32(0.25) * _f(rng, 2, 3, 4)
        x[0, 0] = [0.0, 0.5, -1.5, 2.5]
        if op in ("Log", "Sqrt"):
            x = np.abs(x) + np.float32(0.125)
        if op == "IsNaN":
            x[1, 2, 3] = np.nan
        nodes, outs = [W.node(op, ["x"], ["y"])], ["y"]
        if op in attrs:
            nodes.append(W.node(op, ["x"], ["y_attr"], attrs=attrs[op])); outs.append("y_attr")
        if op in ("Floor", "Ceil", "Sqrt", "Neg", "Abs", "Round", "Not", "Sign"):          # a host float operand
            nodes.append(W.node(op, ["hf"], ["y_hf"])); outs.append("y_hf")
        if op in ("Neg", "Abs", "Sign", "Not", "Floor"):                                   # a host integer operand
            nodes.append(W.node(op, ["hi"], ["y_hi"])); outs.append("y_hi")
        inits = [W.tensor("hf", np.asarray([[0.0, 0.5, 1.5], [2.25, 6.5, 0.75]], np.float32)), _i("hi", [[-3, 0], [2, 7]])]
        out.append(_zoo(name, nodes, inits, {"x": x}, outs))
    return out


def _zoo_binary():
    out = []
    for op in BINARY_OPS:
        name = "zoo_" + op
        rng = _rng(name)
        a, b, c = _q(rng, 2, 1, 4), _q(rng, 3, 1), _q(rng, 4)
        if op == "Pow":
            a = np.abs(a) + np.float32(0.5)
        ia, ib = np.asarray([[7], [-7]], np.int64), np.asarray([2, -3, 5], np.int64)
        inits = [W.tensor("s", np.float32(1.5).reshape(())), _i("hi", [[7], [-7]]), _i("hj", [2, -3, 5])]
        nodes = [W.node(op, ["a", "b"], ["y"]),                   # device, rank 3 against rank 2
                 W.node(op, ["a", "s"], ["y_s"]),                 # a host scalar against a device tensor
                 W.node(op, ["hi", "hj"], ["y_h"])]               # both on the host, integers
        outs = ["y", "y_s", "y_h"]
        if op != "Div":                                           # integer division of device tensors is refused
            nodes.append(W.node(op, ["ia", "ib"], ["y_i"])); outs.append("y_i")
        if op == "Mod":
            nodes += [W.node(op, ["a", "b"], ["y_f"], attrs=[W.attr_int("fmod", 1)]), W.node(op, ["hi", "hj"], ["y_hf"], attrs=[W.attr_int("fmod", 1)])]
            outs += ["y_f", "y_hf"]
        if op in ("Sum", "Mean"):
            nodes += [W.node(op, ["a", "b", "c"], ["y3"]), W.node(op, ["a"], ["y1"])]
            outs += ["y3", "y1"]
        out.append(_zoo(name, nodes, inits, {"a": a, "b": b, "c": c, "ia": ia, "ib": ib}, outs))
    return out


def _zoo_other():
    n, out = W.node, []

    def add(op, nodes, inits, feeds, outs, opset=17, name=None):
        out.append(_zoo(name or "zoo_" + op, nodes, inits, feeds, outs, opset))

    def x_of(name, *shape):
        return _f(_rng(name), *shape)

    hi = _i("hi", [[-3, 0], [2, 7]])
    x = x_of("zoo_x234", 2, 3, 4)
    add("Identity", [n("Identity", ["x"], ["y"]), n("Identity", ["hi"], ["y_h"])], [hi], {"x": x}, ["y", "y_h"])
    add("Dropout", [n("Dropout", ["x"], ["y"])], [], {"x": x}, ["y"])
    add("Reshape", [n("Reshape", ["x", "s0"], ["y0"]), n("Reshape", ["x", "s1"], ["y1"]), n("Reshape", ["x", "s2"], ["y2"], attrs=[W.attr_int("allowzero", 1)]),
                    n("Reshape", ["hi", "s3"], ["y_h"])],
        [hi, _i("s0", [0, -1]), _i("s1", [4, 0, -1]), _i("s2", [6, 4]), _i("s3", [4])], {"x": x}, ["y0", "y1", "y2", "y_h"])
    add("Flatten", [n("Flatten", ["x"], ["y1"]), n("Flatten", ["x"], ["ym1"], attrs=[W.attr_int("axis", -1)]), n("Flatten", ["x"], ["y0"], attrs=[W.attr_int("axis", 0)]),
                    n("Flatten", ["x"], ["y3"], attrs=[W.attr_int("axis", 3)]), n("Flatten", ["hi"], ["y_h"])], [hi], {"x": x}, ["y1", "ym1", "y0", "y3", "y_h"])
    xs = x_of("zoo_Squeeze", 2, 1, 4, 1)
    add("Squeeze", [n("Squeeze", ["x", "a1"], ["y1"]), n("Squeeze", ["x", "am"], ["ym"]), n("Squeeze", ["x"], ["yall"]),
                    n("Squeeze", ["x"], ["yattr"], attrs=[W.attr_ints("axes", [-1])]), n("Squeeze", ["h1"], ["y_h"])],
        [_i("a1", [1]), _i("am", [-1, 1]), _i("h1", [[5], [6]])], {"x": xs}, ["y1", "ym", "yall", "yattr", "y_h"])
    xu = x_of("zoo_Unsqueeze", 2, 3)
    add("Unsqueeze", [n("Unsqueeze", ["x", "a0"], ["y0"]), n("Unsqueeze", ["x", "am"], ["ym"]), n("Unsqueeze", ["x", "a03"], ["y03"]),
                      n("Unsqueeze", ["x"], ["yattr"], attrs=[W.attr_ints("axes", [1])]), n("Unsqueeze", ["hi", "a0"], ["y_h"])],
        [hi, _i("a0", [0]), _i("am", [-1]), _i("a03", [3, 0])], {"x": xu}, ["y0", "ym", "y03", "yattr", "y_h"])
    add("Transpose", [n("Transpose", ["x"], ["yrev"]), n("Transpose", ["x"], ["y120"], attrs=[W.attr_ints("perm", [1, 2, 0])]),
                      n("Transpose", ["x"], ["yid"], attrs=[W.attr_ints("perm", [0, 1, 2])]), n("Transpose", ["hi"], ["y_h"]), n("Transpose", ["xi"], ["y_i"], attrs=[W.attr_ints("perm", [1, 0])])],
        [hi], {"x": x, "xi": np.arange(6, dtype=np.int64).reshape(2, 3) - 2}, ["yrev", "y120", "yid", "y_h", "y_i"])
    x2 = x_of("zoo_Concat", 2, 2, 4)
    add("Concat", [n("Concat", ["x", "x2"], ["y1"], attrs=[W.attr_int("axis", 1)]), n("Concat", ["x", "x"], ["ym1"], attrs=[W.attr_int("axis", -1)]),
                   n("Concat", ["hi", "hj"], ["y_h"], attrs=[W.attr_int("axis", 0)]), n("Concat", ["hi", "hk"], ["y_h1"], attrs=[W.attr_int("axis", -1)]),
                   n("Concat", ["xf", "hi"], ["y_mixed"], attrs=[W.attr_int("axis", 0)]), n("Concat", ["xi", "hi"], ["y_i"], attrs=[W.attr_int("axis", 0)]), n("Concat", ["x"], ["y_one"], attrs=[W.attr_int("axis", 2)])],
        [hi, _i("hj", [[9, 9]]), _i("hk", [[1], [2]])], {"x": x, "x2": x2, "xf": x_of("zoo_Concat_f", 1, 2), "xi": np.asarray([[1 << 40, -5]], np.int64)}, ["y1", "ym1", "y_h", "y_h1", "y_mixed", "y_i", "y_one"])
    x456 = x_of("zoo_Slice", 4, 5, 6)
    add("Slice", [n("Slice", ["x", "st0", "en0", "ax0", "sp0"], ["y0"]),          # axis 1 1:5:2, axis -1 4:begin:-1
                  n("Slice", ["x", "st1", "en1"], ["y1"]),                         # default axes and steps, bounds past both ends
                  n("Slice", ["x", "st2", "en2", "ax2", "sp2"], ["y2"]),           # negative step past the start: everything reversed, step -2
                  n("Slice", ["x"], ["yattr"], attrs=[W.attr_ints("starts", [1, 0]), W.attr_ints("ends", [3, 100]), W.attr_ints("axes", [0, 2])]),
                  n("Slice", ["x", "st3", "en3", "ax3"], ["yempty"]),              # start == end
                  n("Shape", ["x"], ["shp"]), n("Slice", ["shp", "st4", "en4"], ["y_h"])],
        [_i("st0", [1, 4]), _i("en0", [5, -(1 << 62)]), _i("ax0", [1, -1]), _i("sp0", [2, -1]), _i("st1", [-100, 2]), _i("en1", [100, -1]),
         _i("st2", [100]), _i("en2", [-100]), _i("ax2", [-2]), _i("sp2", [-2]), _i("st3", [2]), _i("en3", [2]), _i("ax3", [0]), _i("st4", [1]), _i("en4", [3])],
        {"x": x456}, ["y0", "y1", "y2", "yattr", "yempty", "y_h"])
    x264 = x_of("zoo_Split", 2, 6, 4)
    add("Split", [n("Split", ["x", "sz"], ["a0", "a1", "a2"], attrs=[W.attr_int("axis", 1)]), n("Split", ["x"], ["b0", "b1"], attrs=[W.attr_int("axis", -1)]),
                  n("Split", ["x"], ["c0", "c1"], attrs=[W.attr_int("axis", 0), W.attr_ints("split", [1, 1])]), n("Split", ["hi"], ["d0", "d1"], attrs=[W.attr_int("axis", 1)])],
        [hi, _i("sz", [1, 2, 3])], {"x": x264}, ["a0", "a1", "a2", "b0", "b1", "c0", "c1", "d0", "d1"])
    x345 = x_of("zoo_Gather", 3, 4, 5)
    add("Gather", [n("Gather", ["x", "idx"], ["y1"], attrs=[W.attr_int("axis", 1)]), n("Gather", ["x", "idx"], ["ym1"], attrs=[W.attr_int("axis", -1)]),
                   n("Gather", ["x", "i0"], ["y0"]), n("Shape", ["x"], ["shp"]), n("Gather", ["shp", "i0"], ["y_h"]), n("Gather", ["shp", "idm"], ["y_hm"]),
                   n("Gather", ["xi", "idx"], ["y_i"]), n("Gather", ["x", "di"], ["y_dev_idx"], attrs=[W.attr_int("axis", 2)])],
        [_i("idx", [[0, 2], [1, -1]]), _i("i0", 2), _i("idm", [-1, 0])],
        {"x": x345, "xi": (np.arange(12, dtype=np.int64).reshape(4, 3) - 6) * ((1 << 40) + 1), "di": np.asarray([4, -5, 0], np.int64)}, ["y1", "ym1", "y0", "y_h", "y_hm", "y_i", "y_dev_idx"])
    add("Shape", [n("Shape", ["x"], ["y"]), n("Shape", ["x"], ["y1"], attrs=[W.attr_int("start", 1)]), n("Shape", ["x"], ["ye"], attrs=[W.attr_int("end", -1)]),
                  n("Shape", ["x"], ["ys"], attrs=[W.attr_int("start", -2), W.attr_int("end", 100)]), n("Shape", ["hi"], ["y_h"])], [hi], {"x": x}, ["y", "y1", "ye", "ys", "y_h"])
    add("Size", [n("Size", ["x"], ["y"]), n("Size", ["hi"], ["y_h"])], [hi], {"x": x}, ["y", "y_h"])
    add("Constant", [n("Constant", [], ["yt"], attrs=[W.attr_tensor("value", np.arange(6, dtype=np.float32).reshape(2, 3) / 4)]),
                     n("Constant", [], ["yti"], attrs=[W.attr_tensor("value", np.asarray([3, -4], np.int64))]), n("Constant", [], ["yf"], attrs=[W.attr_float("value_float", 0.75)]),
                     n("Constant", [], ["yi"], attrs=[W.attr_int("value_int", -9)]), n("Constant", [], ["yis"], attrs=[W.attr_ints("value_ints", [4, 5, 6])]),
                     n("Constant", [], ["yfs"], attrs=[W.attr_floats("value_floats", [0.5, -2.25])]), n("Add", ["x", "yt"], ["y"])],
        [], {"x": x_of("zoo_Constant", 2, 3)}, ["yt", "yti", "yf", "yi", "yis", "yfs", "y"])
    add("ConstantOfShape", [n("ConstantOfShape", ["s"], ["yf"], attrs=[W.attr_tensor("value", np.asarray([1.5], np.float32))]), n("ConstantOfShape", ["s"], ["y0"]),
                            n("ConstantOfShape", ["s"], ["yi"], attrs=[W.attr_tensor("value", np.asarray([7], np.int64))]), n("Shape", ["x"], ["shp"]),
                            n("ConstantOfShape", ["shp"], ["yx"]), n("Add", ["x", "yf"], ["y"])],
        [_i("s", [2, 3])], {"x": x_of("zoo_ConstantOfShape", 2, 3)}, ["yf", "y0", "yi", "yx", "y"])
    add("Range", [n("Range", ["c0", "c20", "c3"], ["yi"]), n("Range", ["f0", "f1", "fd"], ["yf"]), n("Range", ["c20", "c0", "cm7"], ["yneg"]), n("Range", ["c0", "lim", "c3"], ["ydev"]),
                  n("Range", ["c20", "c0", "c3"], ["yempty"])],
        [_i("c0", 0), _i("c20", 20), _i("c3", 3), _i("cm7", -7), W.tensor("f0", np.float32(0.5).reshape(())), W.tensor("f1", np.float32(3.0).reshape(())),
         W.tensor("fd", np.float32(0.75).reshape(()))], {"lim": np.asarray(10, np.int64)}, ["yi", "yf", "yneg", "ydev", "yempty"])
    xc = _q(_rng("zoo_Cast"), 2, 3, 4) * np.float32(1.25)
    add("Cast", [n("Cast", ["x"], ["y7"], attrs=[W.attr_int("to", 7)]), n("Cast", ["x"], ["y9"], attrs=[W.attr_int("to", 9)]), n("Cast", ["x"], ["y11"], attrs=[W.attr_int("to", 11)]),
                 n("Cast", ["x"], ["y6"], attrs=[W.attr_int("to", 6)]), n("Cast", ["xi"], ["yi1"], attrs=[W.attr_int("to", 1)]), n("Cast", ["xi"], ["yi9"], attrs=[W.attr_int("to", 9)]),
                 n("Cast", ["hi"], ["yh1"], attrs=[W.attr_int("to", 1)]), n("Cast", ["hf"], ["yh7"], attrs=[W.attr_int("to", 7)]), n("Cast", ["hf"], ["yh9"], attrs=[W.attr_int("to", 9)]),
                 n("Cast", ["hf"], ["yhf1"], attrs=[W.attr_int("to", 1)])],
        [hi, W.tensor("hf", np.asarray([-1.75, 0.0, 2.5], np.float32))], {"x": xc, "xi": np.asarray([[3, 0], [-2, 1 << 20]], np.int64)},
        ["y7", "y9", "y11", "y6", "yi1", "yi9", "yh1", "yh7", "yh9", "yhf1"])
    add("Expand", [n("Expand", ["x", "s"], ["y"]), n("Expand", ["x", "s1"], ["ysame"]), n("Expand", ["h", "sh"], ["y_h"]), n("Expand", ["xi", "s"], ["y_i"])],
        [_i("s", [2, 3, 4]), _i("s1", [3, 1]), _i("h", [[5], [6]]), _i("sh", [2, 3])], {"x": x_of("zoo_Expand", 3, 1), "xi": np.asarray([[1], [2], [3]], np.int64)}, ["y", "ysame", "y_h", "y_i"])
    add("Tile", [n("Tile", ["x", "r0"], ["y0"]), n("Tile", ["x", "r1"], ["y1"]), n("Tile", ["hi", "r0"], ["y_h"]), n("Tile", ["x", "rz"], ["yzero"])],
        [hi, _i("r0", [2, 1]), _i("r1", [1, 3]), _i("rz", [0, 2])], {"x": x_of("zoo_Tile", 2, 3)}, ["y0", "y1", "y_h", "yzero"])
    rw = _rng("zoo_Where")
    add("Where", [n("Where", ["c", "a", "b"], ["y"]), n("Where", ["c", "ia", "ib"], ["y_i"]), n("Where", ["hc", "hi", "hj"], ["y_h"]), n("Less", ["a", "b"], ["lt"]),
                  n("Greater", ["a", "b"], ["gt"]), n("Where", ["c", "lt", "gt"], ["y_b"]), n("Where", ["hc", "a", "hk"], ["y_mixed"])],
        [hi, _i("hc", [[1], [0]]), _i("hj", [[10, 20]]), _i("hk", [[1], [2]])],
        {"c": (rw.random((3, 1)) < 0.5).astype(np.float32), "a": _q(rw, 2, 1, 4), "b": _q(rw, 4), "ia": np.asarray([[(1 << 40) + 1], [-3]], np.int64).reshape(2, 1, 1), "ib": np.arange(4, dtype=np.int64)},
        ["y", "y_i", "y_h", "y_b", "y_mixed"])
    add("Clip", [n("Clip", ["x", "lo", "hi"], ["y"]), n("Clip", ["x", "lo"], ["ylo"]), n("Clip", ["x", "", "hi"], ["yhi"]), n("Clip", ["x"], ["ynone"]),
                 n("Clip", ["x"], ["yattr"], attrs=[W.attr_float("min", -0.25), W.attr_float("max", 0.5)])],
        [W.tensor("lo", np.float32(-0.5).reshape(())), W.tensor("hi", np.float32(0.8).reshape(()))], {"x": x}, ["y", "ylo", "yhi", "ynone", "yattr"])
    rb = _rng("zoo_BatchNormalization")
    add("BatchNormalization", [n("BatchNormalization", ["x", "g", "b", "m", "v"], ["y"]), n("BatchNormalization", ["x4", "g", "b", "m", "v"], ["y4"], attrs=[W.attr_float("epsilon", 1e-3)])],
        [W.tensor("g", _f(rb, 3)), W.tensor("b", _f(rb, 3)), W.tensor("m", _f(rb, 3)), W.tensor("v", (rb.random(3) + 0.5).astype(np.float32))],
        {"x": x, "x4": _f(rb, 2, 3, 2, 5)}, ["y", "y4"])
    add("Pad", [n("Pad", ["x", "p6", "pv"], ["yc"]), n("Pad", ["x", "p2", "", "axm1"], ["yr"], attrs=[W.attr_str("mode", "reflect")]),
                n("Pad", ["x", "p4", "", "ax02"], ["ye"], attrs=[W.attr_str("mode", "edge")]),
                n("Pad", ["x"], ["yattr"], attrs=[W.attr_ints("pads", [0, 1, 0, 0, 0, 2]), W.attr_float("value", -1.0)]), n("Pad", ["x", "pneg"], ["ycrop"])],
        [_i("p6", [1, 0, 2, 0, 1, 0]), W.tensor("pv", np.float32(0.25).reshape(())), _i("p2", [2, 3]), _i("axm1", [-1]), _i("p4", [1, 2, 0, 1]), _i("ax02", [0, -1]),
         _i("pneg", [0, 0, -1, 0, 0, 0])], {"x": x}, ["yc", "yr", "ye", "yattr", "ycrop"])
    x2345 = x_of("zoo_pool", 2, 3, 4, 5)
    add("GlobalAveragePool", [n("GlobalAveragePool", ["x"], ["y"]), n("GlobalAveragePool", ["x3"], ["y3"])], [], {"x": x2345, "x3": x}, ["y", "y3"])
    add("GlobalMaxPool", [n("GlobalMaxPool", ["x"], ["y"]), n("GlobalMaxPool", ["x3"], ["y3"])], [], {"x": x2345, "x3": x}, ["y", "y3"])
    add("Trilu", [n("Trilu", ["x"], ["yu"]), n("Trilu", ["x", "km1"], ["yl"], attrs=[W.attr_int("upper", 0)]), n("Trilu", ["x", "k1"], ["yu1"]), n("Trilu", ["xi"], ["y_i"], attrs=[W.attr_int("upper", 0)])],
        [_i("km1", -1), _i("k1", 1)], {"x": x_of("zoo_Trilu", 2, 4, 5), "xi": np.arange(12, dtype=np.int64).reshape(3, 4) + 1}, ["yu", "yl", "yu1", "y_i"])
    rg = _rng("zoo_GatherElements")
    add("GatherElements", [n("GatherElements", ["x", "i1"], ["y1"], attrs=[W.attr_int("axis", 1)]), n("GatherElements", ["x", "im1"], ["ym1"], attrs=[W.attr_int("axis", -1)]),
                           n("GatherElements", ["x", "i0"], ["y0"]), n("GatherElements", ["xi", "ii"], ["y_i"], attrs=[W.attr_int("axis", 1)])],
        [_i("i1", rg.integers(-4, 4, (3, 2, 5))), _i("im1", rg.integers(-5, 5, (3, 4, 7))), _i("i0", rg.integers(0, 3, (1, 4, 5))), _i("ii", [[1, 0, 0], [-1, -2, 1]])],
        {"x": x345, "xi": np.asarray([[(1 << 40) + 1, 2], [3, -(1 << 41)]], np.int64)}, ["y1", "ym1", "y0", "y_i"])
    add("ScatterND", [n("ScatterND", ["kv", "i3", "u3"], ["y3"]), n("ScatterND", ["kv", "i2", "u2"], ["y2"]), n("ScatterND", ["kv", "i4", "u4"], ["y4"])],
        [_i("i3", [[0, 1, 2], [0, 0, 8], [0, -1, 0]]), _i("i2", [[0, 1], [0, 0]]), _i("i4", [[0, 1, 8, 3], [0, 0, 0, 0]])],
        {"kv": x_of("zoo_ScatterND", 1, 2, 9, 4), "u3": x_of("zoo_ScatterND_u3", 3, 4), "u2": x_of("zoo_ScatterND_u2", 2, 9, 4), "u4": x_of("zoo_ScatterND_u4", 2)}, ["y3", "y2", "y4"])
    x1234 = x_of("zoo_Resize", 1, 2, 3, 4)
    native = [W.attr_str("mode", "nearest"), W.attr_str("coordinate_transformation_mode", "asymmetric"), W.attr_str("nearest_mode", "floor")]
    add("Resize", [n("Resize", ["x", "roi", "sc"], ["ys"], attrs=native), n("Resize", ["x", "roi", "", "sz"], ["yz"], attrs=native), n("Resize", ["x", "", "sc"], ["ydef"]),
                   n("Resize", ["x", "", "sc15"], ["y15"], attrs=native)],
        [W.tensor("sc", np.asarray([1, 1, 2, 3], np.float32)), W.tensor("sc15", np.asarray([1, 1, 1.5, 0.5], np.float32)), W.tensor("roi", np.zeros(0, np.float32)), _i("sz", [1, 2, 6, 4])],
        {"x": x1234}, ["ys", "yz", "ydef", "y15"], opset=13)
    add("Resize", [n("Resize", ["x", "sc"], ["y"]), n("Resize", ["x", "sc"], ["ymode"], attrs=[W.attr_str("mode", "nearest")])],
        [W.tensor("sc", np.asarray([1, 1, 2, 3], np.float32))], {"x": x1234}, ["y", "ymode"], opset=10, name="zoo_resize_opset10")
    add("Softmax", [n("Softmax", ["x"], ["ydef"]), n("Softmax", ["x"], ["y0"], attrs=[W.attr_int("axis", 0)]), n("Softmax", ["x"], ["ym1"], attrs=[W.attr_int("axis", -1)]),
                    n("LogSoftmax", ["x"], ["ylog2"], attrs=[W.attr_int("axis", 2)]), n("LogSoftmax", ["x"], ["ylogdef"])],
        [], {"x": x}, ["ydef", "y0", "ym1", "ylog2", "ylogdef"], opset=12, name="zoo_softmax_opset12")
    add("Softmax", [n("Softmax", ["x"], ["ydef"]), n("Softmax", ["x"], ["y0"], attrs=[W.attr_int("axis", 0)]), n("Softmax", ["x"], ["ym2"], attrs=[W.attr_int("axis", -2)]),
                    n("LogSoftmax", ["x"], ["ylog0"], attrs=[W.attr_int("axis", -3)]), n("Softmax", ["hi"], ["y_h"])],
        [hi], {"x": x}, ["ydef", "y0", "ym2", "ylog0", "y_h"], opset=13, name="zoo_softmax_axes")
    # the reduce family: pass-through with noop_with_empty_axes (the node after it still finds its input), the host evaluator, negative and non-last axes
    add("ReduceSum", [n("ReduceSum", ["x", "none"], ["ynoop"], attrs=[W.attr_int("noop_with_empty_axes", 1)]), n("Neg", ["ynoop"], ["yafter"]),
                      n("ReduceMean", ["x", "none"], ["ymnoop"], attrs=[W.attr_int("noop_with_empty_axes", 1), W.attr_int("keepdims", 0)]),
                      n("ReduceMax", ["x", "none"], ["yall"], attrs=[W.attr_int("keepdims", 0)]),
                      n("ReduceSum", ["hi", "none"], ["y_hnoop"], attrs=[W.attr_int("noop_with_empty_axes", 1)])],
        [hi, _i("none", np.zeros((0,), np.int64))], {"x": x}, ["ynoop", "yafter", "ymnoop", "yall", "y_hnoop"], opset=18, name="zoo_reduce_noop_empty_axes")
    hnodes, houts = [n("Shape", ["x"], ["shp"])], []
    for op in ("ReduceSum", "ReduceProd", "ReduceMax", "ReduceMin", "ReduceMean"):
        hnodes += [n(op, ["shp"], ["s_" + op], attrs=[W.attr_int("keepdims", 0)]), n(op, ["hi", "am1"], ["h_" + op]), n(op, ["hi", "a0"], ["h0_" + op], attrs=[W.attr_int("keepdims", 0)])]
        houts += ["s_" + op, "h_" + op, "h0_" + op]
    hnodes += [n("ReduceL1", ["hi", "am1"], ["h_l1"]), n("ArgMax", ["hi"], ["h_argmax"], attrs=[W.attr_int("axis", -1)]),
               n("ArgMin", ["x"], ["argmin_m2"], attrs=[W.attr_int("axis", -2), W.attr_int("keepdims", 0)]), n("ArgMax", ["x"], ["argmax_0"])]
    add("ReduceProd", hnodes, [hi, _i("am1", [-1]), _i("a0", [0])], {"x": x}, houts + ["h_l1", "h_argmax", "argmin_m2", "argmax_0"], opset=18, name="zoo_reduce_host_and_arg_axes")
    # forms of the row operators that the row table leaves out: a non-last normalised extent, no bias, per-group affine, a middle LpNormalization axis
    rn = _rng("zoo_norm_forms")
    add("LayerNormalization", [n("LayerNormalization", ["x", "g34"], ["y1"], attrs=[W.attr_int("axis", 1)]), n("LayerNormalization", ["x", "g4", "b4"], ["ym1"]),
                               n("LayerNormalization", ["x", "g34", "b34"], ["ym2"], attrs=[W.attr_int("axis", -2), W.attr_float("epsilon", 1e-3)]),
                               n("GroupNormalization", ["x4", "gg", "gb"], ["ygn"], attrs=[W.attr_int("num_groups", 2)]),
                               n("LpNormalization", ["x"], ["ylp1"], attrs=[W.attr_int("axis", 1), W.attr_int("p", 1)]), n("LpNormalization", ["x"], ["ylp0"], attrs=[W.attr_int("axis", -3)]),
                               n("InstanceNormalization", ["x4", "ig", "ib"], ["yin"]), n("CumSum", ["x", "c0"], ["ycs0"], attrs=[W.attr_int("reverse", 1)]), n("CumSum", ["x", "cm2"], ["ycsm2"])],
        [W.tensor("g34", _f(rn, 3, 4)), W.tensor("b34", _f(rn, 3, 4)), W.tensor("g4", _f(rn, 4)), W.tensor("b4", _f(rn, 4)), W.tensor("gg", _f(rn, 2)), W.tensor("gb", _f(rn, 2)),
         W.tensor("ig", _f(rn, 4)), W.tensor("ib", _f(rn, 4)), _i("c0", 0), _i("cm2", -2)],
        {"x": x, "x4": _f(rn, 2, 4, 3, 2)}, ["y1", "ym1", "ym2", "ygn", "ylp1", "ylp0", "yin", "ycs0", "ycsm2"], opset=18, name="zoo_row_forms")
    return out


def zoo_cases():
    cases = _zoo_unary() + _zoo_binary() + _zoo_other()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    return cases


# ------------------------------------------------------------------------------------------------------------------ running a case
def run_outputs(q3, tmp_dir, case):
    """-> ({output name: array}, launches of the run) of any case, with or without a reference (the declared output shapes are not read by the executor)"""
    path = os.path.join(str(tmp_dir), case.name + ".onnx")
    ins = [W.value_info(k, I64 if np.issubdtype(np.asarray(v).dtype, np.integer) else F32, list(np.asarray(v).shape)) for k, v in case.feeds.items()]
    outs = case.out if isinstance(case.out, (list, tuple)) else [case.out]
    with open(path, "wb") as f:
        f.write(W.model(case.nodes, case.inits, ins, [W.value_info(o, F32, []) for o in outs], opset=case.opset))
    s = q3.OnnxSession(path)
    try:
        assert s.unsupported() == [], s.unsupported()
        r = s.run(case.feeds, list(outs))
        n = s.launches()
    finally:
        s.close()
    return r, n


def digest_cases(q3, tmp_dir):
    """{case name: {"ops": operator names of the graph, "sha256": over dtype, shape and bytes of every output in order, "launches": of the run}}
    for every product, row and zoo case, on whichever kernel family the loaded library runs (scripts/onnx_exec_digest.py)"""
    import hashlib
    res = {}
    for case in product_cases() + row_cases() + zoo_cases():
        got, launches = run_outputs(q3, tmp_dir, case)
        h = hashlib.sha256()
        for o in (case.out if isinstance(case.out, (list, tuple)) else [case.out]):
            a = np.ascontiguousarray(got[o])
            h.update(("%s %s %s;" % (o, a.dtype.str, list(a.shape))).encode())
            h.update(a.tobytes())
        m = q3.OnnxModel(os.path.join(str(tmp_dir), case.name + ".onnx"))
        ops = sorted({m.node(i)["op_type"] for i in range(m.n_nodes)})
        m.close()
        assert case.name not in res
        res[case.name] = {"ops": ops, "sha256": h.hexdigest(), "launches": int(launches)}
    return res


def run_case(q3, tmp_dir, case):
    """-> (output array, launches of the run)"""
    path = os.path.join(str(tmp_dir), case.name + ".onnx")
    ins = [W.value_info(k, I64 if np.issubdtype(np.asarray(v).dtype, np.integer) else F32, list(np.asarray(v).shape)) for k, v in case.feeds.items()]
    outs = case.out if isinstance(case.out, (list, tuple)) else [case.out]
    with open(path, "wb") as f:
        shp = lambda o: list(np.shape(case.ref[o] if isinstance(case.ref, dict) else case.ref))
        f.write(W.model(case.nodes, case.inits, ins, [W.value_info(o, F32, shp(o)) for o in outs], opset=case.opset))
    s = q3.OnnxSession(path)
    try:
        assert s.unsupported() == [], s.unsupported()
        r = s.run(case.feeds, list(outs))
        n = s.launches()
    finally:
        s.close()
    return (r[case.out] if not isinstance(case.out, (list, tuple)) else r), n


def ratio(got, ref, bound):
    """largest |got - ref| / bound; an exact expectation (bound 0) counts as 0 when met and inf when missed"""
    got, ref, bound = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.broadcast_to(np.asarray(bound, np.float64), np.shape(ref))
    if got.shape != ref.shape:
        return float("inf")
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    with np.errstate(invalid="ignore"):                   # inf - inf where both are the same infinity: `same` already covers it
        err = np.where(same, 0.0, np.abs(got - ref))
    err = np.where(np.isnan(err), np.inf, err)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(r.max()) if r.size else 0.0


if __name__ == "__main__":   # the Q3_ONNX_NAIVE=1 child of test_products_on_the_naive_kernels: the whole product table into one .npz
    import tempfile
    import q3tts
    assert os.environ.get("Q3_ONNX_NAIVE") == "1"
    res = {}
    with tempfile.TemporaryDirectory() as tmp:
        for case in product_cases():
            y, n = run_case(q3tts, tmp, case)
            res[case.name] = y
            res["launches:" + case.name] = np.asarray(n)
    np.savez(sys.argv[1], **res)
