"""float64 reference of one codec-decoder GEMM (csrc/codec.hip, q3tts_op_codec_gemm) and the case list of its forced-form tests.

Row mapping: GEMM row m of tap j reads A row m + (m // a_segT) * a_skip + j * dil (a_segT = 0: unsegmented); output row m starts at float
out_off + m * ldo + (m // o_segT) * o_skip of the output buffer, residual row m at m * ldr + (m // r_segT) * r_skip.  K index k = j * cin + ci."""
import numpy as np
from scipy.special import erf

EPI_NONE, EPI_GELU, EPI_RES_SCALE, EPI_RES, EPI_SNAKE = range(5)


def seg_rows(m, segT, skip):
    """physical row (or float offset, for skips in floats) of logical rows m"""
    m = np.asarray(m, np.int64)
    return m + (m // segT) * skip if segT > 0 else m


def im2col(A, M, cin, taps, dil, a_segT=0, a_skip=0):
    """[M][taps * cin] float64 operand the GEMM multiplies: A is [rows][>= cin] (logical values)"""
    base = seg_rows(np.arange(M), a_segT, a_skip)
    return np.concatenate([np.asarray(A, np.float64)[base + j * dil, :cin] for j in range(taps)], axis=1)


def f16_split(x):
    """hi = f16(x), lo = f16(x - hi) with x - hi in f32, both round-to-nearest-even (the device's v_cvt_f16_f32)"""
    x = np.asarray(x, np.float32)
    hi = x.astype(np.float16)
    lo = (x - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def split_rows(x):
    """rows of C values -> the pre-split layout [C x f16 hi][C x f16 lo], returned as uint32 words [rows][C] (same bytes as C floats)"""
    hi, lo = f16_split(x)
    return np.ascontiguousarray(np.concatenate([hi, lo], axis=1)).view(np.uint32)


def unsplit_rows(w, C):
    """inverse of split_rows for the first C words of each row: (hi, lo) f16 planes and the value hi + lo (exact in f32)"""
    h = np.ascontiguousarray(np.asarray(w, np.uint32)[:, :C]).view(np.float16)
    hi, lo = h[:, :C], h[:, C:]
    return hi, lo, hi.astype(np.float64) + lo.astype(np.float64)


def split_weights_emul(W, prescale=True):
    """the decoder's weight split (split_weights in codec.hip) in numpy: per-row power-of-two prescale, hi / lo f16 planes, and the float64
    value each weight is represented by once the accumulator is scaled back (prescale=False: the unscaled split)"""
    W = np.asarray(W, np.float32)
    s = np.zeros(W.shape[0], np.int64)
    if prescale:
        mx = np.abs(W).max(axis=1)
        _, e = np.frexp(mx)
        s = np.where(mx > 0, np.minimum(14 - e, 126), 0)
    x = (W.astype(np.float64) * np.exp2(s)[:, None]).astype(np.float32)
    hi, lo = f16_split(x)
    return hi, lo, (hi.astype(np.float64) + lo.astype(np.float64)) * np.exp2(-s)[:, None]


def epilogue(v, epi, bias=None, res=None, scale=None, ea=None, ib=None):
    """float64 epilogue of v = acc [M][N]; res: the [M][N] residual rows"""
    v = np.asarray(v, np.float64)
    if bias is not None:
        v = v + np.asarray(bias, np.float64)
    if epi == EPI_GELU:
        return 0.5 * v * (1.0 + erf(v / np.sqrt(2.0)))
    if epi == EPI_RES_SCALE:
        return np.asarray(res, np.float64) + np.asarray(scale, np.float64) * v
    if epi == EPI_RES:
        return np.asarray(res, np.float64) + v
    if epi == EPI_SNAKE:
        return v + np.asarray(ib, np.float64) * np.sin(v * np.asarray(ea, np.float64)) ** 2
    return v


def gemm_ref(A, W, M, cin, taps, dil, a_segT=0, a_skip=0):
    """(acc, sum |a||w|) float64 [M][N] for A's logical values"""
    X = im2col(A, M, cin, taps, dil, a_segT, a_skip)
    W = np.asarray(W, np.float64)
    return X @ W.T, np.abs(X) @ np.abs(W).T


def out_index(M, N, ldo, out_off=0, o_segT=0, o_skip=0):
    """[M][N] float positions of the logical output inside the output buffer"""
    m = np.arange(M)
    base = out_off + m * ldo + ((m // o_segT) * o_skip if o_segT > 0 else 0)
    return base[:, None] + np.arange(N)[None, :]


def shape_bar(K):
    """per-element bar factor on sum |a||w| (f32 accumulation order, a few ulp per partial sum)"""
    return 2.0 ** -20 * np.sqrt(max(1.0, K / 4096.0))


# ---- forced-form cases of tests/test_gpu_codec_gemm.py (tests/test_codec_gemm_plan_cpu.py checks the decoder uses nothing else) ----
# (form, M, N, cin, taps, dil, G, H, ksplit, reducer, a_split)
def _cases():
    c = []
    for form, Ms in (("SKINNY4", (1, 4)), ("SKINNY8", (5, 8)), ("SKINNY16", (9, 16))):
        for i, M in enumerate(Ms):
            c.append((form, M, 100, (1344, 16)[i], 1 + 6 * i, (1, 9)[i], (1, 3)[i], (0, 6)[i], 1, -1, i == 1))
    # f32 MFMA kernels: rows at the 32 / 64 tile edges, N off the 128 / 64 tiles, cin = 16, split-K with both reducers
    for form, Ms in (("F32_1", (17, 32, 33)), ("F32_2", (63, 64, 65))):
        for i, M in enumerate(Ms):
            c.append((form, M, 100, (16, 48, 1344)[i], (7, 2, 1)[i], (3, 1, 1)[i], (1, 3, 1)[i], (18, 1, 0)[i], 1, -1, False))
        c.append((form, Ms[0], 76, 64, 7, 9, 3, 54, 4, 0, False))
        c.append((form, Ms[2], 132, 32, 2, 1, 16, 71, 2, 1, True))
    # split-f16 64 x 64 / 128 x 64 tiles: M at 64 / 128 (and 1024 for the tall tile) edges, N off the 64 tile
    for form in ("H1", "H1_EPL", "H2", "H2_EPL"):
        Ms = (33, 63, 127, 129) if form.startswith("H1") else (64, 128, 1023, 1025)
        odd = 0 if form.endswith("EPL") else 1   # N % 4 == 0 is a precondition of the 16-byte epilogue
        for i, M in enumerate(Ms):
            cin, taps, dil = ((32, 7, 3), (1344, 1, 1), (64, 2, 1), (96, 7, 9))[i]
            G, H = ((1, 0), (3, 6), (16, 1), (3, 71))[i]
            c.append((form, M, (100, 36, 68, 196)[i] - odd, cin, taps, dil, G, H, 1, -1, i == 2))
        c.append((form, 65, 100, 64, 7, 1, 3, 18, 2, 1, False))
        c.append((form, 128, 36 + odd, 1344, 1, 1, 1, 0, 7, 0, True))
        c.append((form, 127, 100, 64, 7, 3, 16, 54, 14, 1, False))
    # 128 x 96 tile: N multiples of 96
    for form in ("H3", "H3_EPL"):
        for i, (M, N, cin, taps, dil, G, H) in enumerate(((127, 96, 32, 7, 1, 1, 6), (128, 192, 1344, 1, 1, 3, 0), (129, 96, 96, 2, 1, 16, 1),
                                                          (255, 288, 64, 7, 9, 3, 54))):
            c.append((form, M, N, cin, taps, dil, G, H, 1, -1, i == 2))
        c.append((form, 129, 96, 64, 7, 3, 3, 18, 2, 1, False))
        c.append((form, 128, 192, 1344, 1, 1, 1, 0, 3, 0, True))
        c.append((form, 65, 96, 96, 7, 1, 16, 71, 7, 1, False))
    return c


FORCED_CASES = _cases()
