"""The cases of tests/test_ggml_mode_ref_cpu.py and tests/test_gpu_ggml_mode.py: for each ggml-mode kernel the smallest shapes at which it
can still go wrong, with the edge values planted by hand.  Everything is seeded and cached: both test files see the same arrays, and the
restatement's outputs (ggml_mode_ref) are computed once per case."""
import functools

import numpy as np

import ggml_mode_ref as R
import linear_ref as LR

F = np.float32

# ---------------------------------------------------------------- quantiser ----------------------------------------------------------------
# k / 32 blocks on 64-thread workgroups, k / 256 super-blocks on the first threads of the same grid: 256 = one super-block, 2304 = 72 blocks
# (a partial second workgroup) and 9 super-blocks, 6144 = three full workgroups and 24 super-blocks
QUANT_CASES = [(k, ntok) for k in (256, 2304, 6144) for ntok in (1, 3)]
TIE_M = np.array([0, 1, 2, 3, 4, 5, 10, 11, 62, 63, 124, 125, 7, 8, 100, 101])   # even and odd: (m + 0.5) is a tie either way, the rules part on even m


def _tie_block(e, sign):
    """256 elements whose every 32-block has the maximum sign * 127 * 2^-e FIRST (so d = 2^-e and id = 2^e exactly, for Q8_0 per block and
    for Q8_K per super-block, where sign < 0 makes iscale positive) and an element of the opposite sign and equal magnitude LAST (it
    quantises to -sign * 127); the others sit at +-(m + 0.5) * 2^-e"""
    s = F(2.0) ** F(-e)
    blk = np.zeros((8, 32), F)
    for b in range(8):
        m = np.roll(TIE_M, b)[:15].astype(F)
        blk[b, 0] = sign * 127 * s
        blk[b, 1:16] = (m + F(0.5)) * s
        blk[b, 16:31] = -(m + F(0.5)) * s
        blk[b, 31] = -sign * 127 * s
    return blk.reshape(256)


def _edge_blocks(rng):
    """the edge super-blocks, by name"""
    rnd = lambda: (rng.standard_normal(256) * 0.5).astype(F)
    e = {}
    e["tie_q8_0"] = _tie_block(3, +1)                       # maximum +127 * 2^-3: Q8_0 id = 8, Q8_K iscale = -8
    e["tie_q8_K"] = _tie_block(-2, -1)                      # maximum -127 * 4: Q8_K iscale = +1/4
    v = rnd(); v[100] = -3.75; e["neg_max"] = v             # the element of largest magnitude is negative
    v = rnd(); v[5] = 2.5; v[200] = -2.5; e["equal_opposite"] = v   # equal magnitudes, opposite signs: the first wins
    v = rnd(); v[64:96] = 0; e["zero_block"] = v            # an all-zero 32-block (Q8_0 d = 0, id = 0) inside a non-zero super-block
    e["zero_super"] = np.zeros(256, F)                      # dk = 0, bsums = 0
    # subnormal inputs under one normal maximum of about 1e-30 per 32-block: the f16 scale (7.9e-33) underflows to 0.  (A block that is
    # subnormal THROUGHOUT is left out: its d is below 1 / FLT_MAX, id = inf, and ggml's own (int8_t)roundf(inf) is undefined in C: nothing to pin)
    v = (rng.integers(-9000, 9000, 256) * 1e-42).astype(F)
    v[17::32] = (np.arange(1, 9) * np.array([1, -1] * 4) * 1e-30).astype(F); v[40] = 0; e["tiny"] = v
    v = rnd(); v[3] = -0.0; v[32:64] = -0.0; v[255] = -0.0; e["neg_zero"] = v
    e["plain"] = rnd()
    return e


EDGE_NAMES = ["tie_q8_0", "tie_q8_K", "neg_max", "equal_opposite", "zero_block", "zero_super", "tiny", "neg_zero", "plain"]


@functools.lru_cache(maxsize=None)
def quant_case(k, ntok):
    """-> (x [ntok][k], names [ntok][k/256]): super-block s of row t holds edge (first + t * nsb + s) of EDGE_NAMES while they last, then
    random values; `first` differs between the two k = 256 cases so that between them they reach four different edges"""
    rng = np.random.default_rng(1000 + k + ntok)
    edges = _edge_blocks(rng)
    nsb = k // 256
    first = {(256, 1): 0, (256, 3): 1}.get((k, ntok), 0)
    x = (rng.standard_normal((ntok, k)) * 0.5).astype(F)
    names = [["random"] * nsb for _ in range(ntok)]
    for t in range(ntok):
        for s in range(nsb):
            i = first + t * nsb + s
            if i < len(EDGE_NAMES):
                x[t, 256 * s:256 * s + 256] = edges[EDGE_NAMES[i]]
                names[t][s] = EDGE_NAMES[i]
    x.setflags(write=False)
    return x, names


@functools.lru_cache(maxsize=None)
def quant_ref(k, ntok):
    return R.quantize(quant_case(k, ntok)[0])


def tie_rows():
    """[2][256]: the two tie super-blocks on their own"""
    e = _edge_blocks(np.random.default_rng(0))
    return np.stack([e["tie_q8_0"], e["tie_q8_K"]])


# ---------------------------------------------------------------- dot products -------------------------------------------------------------
# (type, rows of the matrix, k, row0, nrows, ntok): row0 > 0, nrows that is no multiple of 64, two workgroups of rows (70), ntok > 1
DOT_SHAPES = [(70, 256, 0, 70, 1), (70, 512, 3, 66, 3), (64, 2304, 0, 64, 2)]
DOT_CASES = [(t,) + s for t in (8, 13, 14) for s in DOT_SHAPES] + [(8, 1, 6144, 0, 1, 1)]
F16_SUBNORMAL = np.array([0x0003], np.uint16).view(np.uint8)      # 3 * 2^-24
_f16 = lambda v: np.array([v], np.float16).view(np.uint8)


def _hand_set(raw, qtype, n, k, row0):
    """plants the block fields no random draw is sure to reach into rows row0, row0 + 1, ... (first block / super-block of each)"""
    rows = raw.reshape(n, R.ROW_BYTES[qtype](k))
    at = lambda i: rows[min(row0 + i, n - 1)]
    if qtype == 8:
        if n == 1:   # the single row: one field per block
            rows[0, 0:2] = 0; rows[0, 34:36] = _f16(-0.0123); rows[0, 68:70] = F16_SUBNORMAL
            return
        at(0)[0:2] = 0                                  # d = 0
        at(1)[0:2] = _f16(-0.0123)                      # negative d
        at(2)[0:2] = F16_SUBNORMAL                      # f16-subnormal d
    elif qtype == 13:
        at(0)[0:2] = 0; at(0)[2:4] = _f16(0.004)        # d = 0 with dmin != 0
        at(1)[0:2] = _f16(-0.003); at(1)[2:4] = _f16(-0.002)   # negative d and dmin
        at(2)[0:2] = F16_SUBNORMAL; at(2)[2:4] = F16_SUBNORMAL
        at(3)[4:16] = 0xFF                              # every 6-bit scale and min 63: the high bits set in every position
        at(4)[2:4] = 0                                  # dmin = 0
    else:
        at(0)[208:210] = 0
        at(1)[208:210] = _f16(-0.0007)
        at(2)[208:210] = F16_SUBNORMAL
        at(3)[192:208] = np.array([-128, -127, -1, -64, -2, -100, -33, -17, -128, -5, -77, -1, -90, -3, -126, -50], np.int8).view(np.uint8)


@functools.lru_cache(maxsize=None)
def dot_case(qtype, n, k, row0, nrows, ntok):
    """-> (raw u8, x [ntok][k]): weights with random fields (linear_ref.rand_rows) and the hand-set blocks; activations with a zero
    super-block (k >= 512) and a last row whose maximum is negative"""
    rng = np.random.default_rng(7000 + 97 * qtype + k + n)
    raw = LR.rand_rows(rng, qtype, n, k).copy()
    _hand_set(raw, qtype, n, k, row0)
    x = (rng.standard_normal((ntok, k)) * 0.5).astype(F)
    if k >= 512:
        x[0, 256:512] = 0
    x[ntok - 1, 7] = -4.0
    raw.setflags(write=False); x.setflags(write=False)
    return raw, x


@functools.lru_cache(maxsize=None)
def dot_ref(qtype, n, k, row0, nrows, ntok):
    """-> (act, y): the restatement's quantised activations and dots of the chained form"""
    raw, x = dot_case(qtype, n, k, row0, nrows, ntok)
    act = R.quantize(x)
    return act, R.matvec(raw, qtype, n, k, row0, nrows, act)


@functools.lru_cache(maxsize=None)
def dot_given(qtype, n, k, row0, nrows, ntok):
    """-> (act, y) for gg_matvec ALONE on arrays no quantiser wrote: -128 in both int8 arrays and block sums that are not the sums of qk (the
    dot must take every array as given)"""
    raw, x = dot_case(qtype, n, k, row0, nrows, ntok)
    rng = np.random.default_rng(8000 + qtype + k)
    q8, d8, qk, dk, bs = [a.copy() for a in R.quantize(x)]
    q8[0, ::37] = -128; qk[0, ::41] = -128
    bs[:] = rng.integers(-2032, 2033, bs.shape)
    dk[ntok - 1, 0] = -dk[ntok - 1, 0]
    act = (q8, d8, qk, dk, bs)
    return act, R.matvec(raw, qtype, n, k, row0, nrows, act)


@functools.lru_cache(maxsize=None)
def dot_f64(qtype, n, k, row0, nrows, ntok, given=False):
    """-> (y64, bound) [ntok][nrows] on the dequantised operands"""
    raw, _ = dot_case(qtype, n, k, row0, nrows, ntok)
    act = (dot_given if given else dot_ref)(qtype, n, k, row0, nrows, ntok)[0]
    a, b = LR.decode(raw, qtype, n, k)
    a, b = a[row0:row0 + nrows], b[row0:row0 + nrows]
    x64 = R.dequant_act(qtype, act)
    if qtype == 13 and given:
        # with block sums that are not the sums of qk the min term is its own operand: sum_j dmin m_j dk bsums_j, not b . x
        d, dmin, sc, m, _ = R.read_q5_k(raw.reshape(n, -1)[row0:row0 + nrows], nrows, k)
        mterm = (dmin.astype(np.float64)[:, :, None] * m).reshape(nrows, k // 32)                      # [nrows][k/32]
        bsx = act[4].astype(np.float64) * np.repeat(np.asarray(act[3], np.float64), 16, axis=-1)       # [ntok][k/16]
        bsx = bsx.reshape(ntok, k // 32, 2)
        y64 = x64 @ a.T - np.einsum("tjh,rj->tr", bsx, mterm)
        mag = np.abs(x64) @ np.abs(a).T + np.einsum("tjh,rj->tr", np.abs(bsx), np.abs(mterm))
        return y64, (LR.gamma(k // 256 + 10) + 1e-12) * mag + (k // 32) * 2.0 ** -125
    return R.dot64(a, b, x64), R.bound_dot(qtype, k, a, b, x64)


def n_negative_q6k_scales():
    return sum(R.n_negative_q6k_scales(dot_case(*c)[0], c[1], c[2]) for c in DOT_CASES if c[0] == 14)


# ---------------------------------------------------------------- RMSNorm ------------------------------------------------------------------
NORM_CASES = [(d, ntok) for d in (64, 100, 256, 2048) for ntok in (1, 3)]
NORM_EPS = 1e-6
_NORM_KINDS = ["zero", "big", "subnormal"]


@functools.lru_cache(maxsize=None)
def norm_case(d, ntok):
    """-> (x [ntok][d], g [d], kinds): a zero row (scale 1 / sqrt(eps)), a row of +-1e20 (the f32 squares overflow to inf, the output is 0) and
    a subnormal row (the squares underflow to 0).  Of the three, the ntok = 3 case of a width holds two and the ntok = 1 case holds the third.
    Row 0 of the ntok = 3 case is one of two rows that tell ggml's f32 squares from squares taken in double:
      lowbit  random values, the first draw for which the two variants round the mean differently;
      spike   one element of 2e19 among ordinary ones: its f32 square is inf (output 0), its double square 4e38 leaves a finite mean"""
    rng = np.random.default_rng(3000 + d)
    i = (64, 100, 256, 2048).index(d)
    kinds = [("lowbit", "spike")[i % 2], _NORM_KINDS[i % 3], _NORM_KINDS[(i + 1) % 3]] if ntok == 3 else [_NORM_KINDS[(i + 2) % 3]]
    x = (rng.standard_normal((ntok, d)) * 0.7).astype(F)
    g = (1 + 0.5 * rng.standard_normal(d)).astype(F)
    for t, kind in enumerate(kinds):
        if kind == "zero":
            x[t] = 0
        elif kind == "big":
            x[t] = np.where(rng.random(d) < 0.5, F(1e20), F(-1e20)); x[t, 1] = 0.25
        elif kind == "subnormal":
            x[t] = (rng.integers(-9000, 9000, d) * 1e-42).astype(F)
        elif kind == "spike":
            x[t, d // 3] = 2e19
        elif kind == "lowbit":
            for _ in range(1000):
                x[t] = (rng.standard_normal(d) * 0.7).astype(F)
                if not np.array_equal(R.rmsnorm(x[t], g, NORM_EPS), R.rmsnorm(x[t], g, NORM_EPS, np.float64)):
                    break
    x.setflags(write=False); g.setflags(write=False)
    return x, g, kinds


@functools.lru_cache(maxsize=None)
def norm_ref(d, ntok):
    x, g, _ = norm_case(d, ntok)
    return R.rmsnorm(x, g, NORM_EPS)


# ---------------------------------------------------------------- SwiGLU, row loads, add ---------------------------------------------------
FLAT_NS = [1, 255, 256, 257, 1000]     # 256-thread workgroups: one element, one short of a workgroup, exactly one, one over, several
ADD_NS = [1, 255, 256, 257]
SWIGLU_GRID = np.array([0.0, -0.0, 1e-30, -1e-30, 20, -20, 88, -88, 104, -104], F)   # expf(-g) reaches inf at g = -104 and 0 at g = 104


@functools.lru_cache(maxsize=None)
def swiglu_case(n):
    """-> (g [n], u [n]): the grid (rotated by n, so that n = 1 holds -88) then random values"""
    rng = np.random.default_rng(4000 + n)
    g = (rng.standard_normal(n) * 3).astype(F); u = rng.standard_normal(n).astype(F)
    grid = np.roll(SWIGLU_GRID, -7 if n == 1 else n)[:n]
    g[:grid.size] = grid
    if n > 12:
        u[10] = 0; u[11] = -0.0
    g.setflags(write=False); u.setflags(write=False)
    return g, u


@functools.lru_cache(maxsize=None)
def add_case(n):
    rng = np.random.default_rng(5000 + n)
    return rng.standard_normal(n).astype(F), rng.standard_normal(n).astype(F)


LOAD_CASES = [(d, form, stride) for d in (256, 300) for form, stride in (("plain", 1), ("int32", 1), ("int32", 17), ("keys", 1), ("keys", 17))]
LOAD_ROWS, LOAD_NTOK = 40, 3


@functools.lru_cache(maxsize=None)
def load_case(d, form, stride):
    """-> (x [LOAD_ROWS][d + 5], rows [3], idx): x_stride = d + 5 > d; idx = None (plain: row t), int32 [ntok * stride] or argmax keys
    [ntok * stride] (kdev.h pack_key of any logit and the row), the entries between the strided ones pointing at row 39"""
    rng = np.random.default_rng(6000 + d + stride)
    x = rng.standard_normal((LOAD_ROWS, d + 5)).astype(F)
    if form == "plain":
        return x, np.arange(LOAD_NTOK), None
    rows = np.array([37, 0, 11])
    if form == "int32":
        idx = np.full((LOAD_NTOK - 1) * stride + 1, 39, np.int32)
        idx[::stride] = rows
    else:
        idx = np.full((LOAD_NTOK - 1) * stride + 1, LR.pack_key(1.0, 39), np.uint64)
        idx[::stride] = [LR.pack_key(v, int(r)) for v, r in zip((-2.5, 0.0, 7e9), rows)]
    return x, rows, idx
