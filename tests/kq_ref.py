"""What the K-quant op-level tests share (test_gpu_q3k.py, test_gpu_q4k.py, test_gpu_kq_forms.py and the CPU check of their case table): random
raw rows of every tensor type of the K-quant layout (8 Q8_0, 11 Q3_K, 12 Q4_K, 13 Q5_K, 14 Q6_K), the twin the CPU oracle reads (a Q3_K row goes
as its Q6_K twin, a Q4_K row as its Q5_K twin: spec S3), the float64 decoders, and the reference of one case of tests/kq_form_cases.py."""
import numpy as np

import linear_ref as R
import q3k_ref as K3
import q4k_ref as K4

RAND = {11: K3.rand_rows_q3k, 12: K4.rand_rows_q4k}
TWIN = {11: lambda raw: (K3.widen_to_q6k(raw), 14), 12: lambda raw: (K4.widen(raw), 13)}
DEC = {11: K3.dec_q3_k, 12: K4.dec_q4_k}
ROW_BYTES = {8: 34 * 8, 11: 110, 12: 144, 13: 176, 14: 210}   # of one row's 256-weight segment


def weights(rng, types, rows, k):
    """-> (device tensors, oracle tensors): Q3_K rows go to the oracle as their Q6_K twin, Q4_K rows as their Q5_K twin"""
    dev = [(RAND[t](rng, n, k) if t in RAND else R.rand_rows(rng, t, n, k), t, n) for t, n in zip(types, rows)]
    return dev, twins(dev)


def twins(dev):
    return [TWIN[t](raw) + (n,) if t in TWIN else (raw, t, n) for raw, t, n in dev]


def decode(dev, k):
    A, B = zip(*[DEC[t](r, n, k) if t in DEC else R.decode(r, t, n, k) for r, t, n in dev])
    return np.concatenate(A), np.concatenate(B)


def copy_row(dev, k, src, dst):
    """the raw bytes of row src over row dst of a one-tensor matrix, in place: the two rows then give bit-equal sums for every token"""
    (raw, t, n), = dev
    rows = raw.reshape(n, ROW_BYTES[t] * (k // 256))
    rows[dst] = rows[src]


def ratio(err, bound):
    return float((np.asarray(err) / np.maximum(bound, 1e-300)).max())


# ------------------------------------------------------------------ the reference of one case of kq_form_cases ------------------------------------
class Ref:
    """inputs and expected outputs of one shape (kq_form_cases.shapes()); `ratio` = the oracle's worst error / bound against float64"""


def _seed(s):
    return [s.op_id, s.types[0] * 31 + len(s.types) * 7 + s.types[-1], s.K, s.nt, s.nrows, s.row0] + [int(v) for _, v in s.setup]


def gemv_ref(L, s):
    """LOP_GEMV (GEMV_KQ, GEMM_KQ_MFMA): slabs bit for bit, their sum against float64 within bound_gemm"""
    from test_gpu_linear import _acts
    r = Ref()
    rng = np.random.default_rng(_seed(s))
    r.W, r.W_twin = weights(rng, s.types, s.rows, s.K)
    r.xq, r.xd = _acts(rng, s.nt, s.K)
    r.want = R.oracle_slabs(L, r.W_twin, s.K, s.row0, s.nrows, r.xq[:s.nt], r.xd[:s.nt])
    a, b = decode(r.W, s.K)
    r.a, r.b = a[s.row0:s.row0 + s.nrows], b[s.row0:s.row0 + s.nrows]
    r.x64 = R.dequant_act(r.xq[:s.nt], r.xd[:s.nt])
    r.y64 = r.x64 @ (r.a - r.b).T
    r.bound = R.bound_gemm(r.a, r.b, r.x64)
    r.ratio = ratio(np.abs(R.sum_slabs(r.want).astype(np.float64) - r.y64), r.bound)
    return r


def gateup_ref(L, s):
    """LOP_GATEUP (GU_KQ_MFMA): aq / ad bit for bit, dequantised against SwiGLU of the float64 products within bound_swiglu_e2e"""
    from test_gpu_linear import _acts
    r = Ref()
    ff = s.nrows // 2
    rng = np.random.default_rng(_seed(s))
    r.W, r.W_twin = weights(rng, s.types, s.rows, s.K)
    r.xq, r.xd = _acts(rng, s.nt, s.K)
    gu = R.sum_slabs(R.oracle_slabs(L, r.W_twin, s.K, 0, 2 * ff, r.xq[:s.nt], r.xd[:s.nt]))
    _, r.aq, r.ad = R.oracle_swiglu_quant(L, gu[:, :ff], gu[:, ff:])
    a, b = decode(r.W, s.K)
    x64 = R.dequant_act(r.xq[:s.nt], r.xd[:s.nt])
    r.G64, r.U64 = x64 @ (a[:ff] - b[:ff]).T, x64 @ (a[ff:] - b[ff:]).T
    r.eg, r.eu = R.bound_gemm(a[:ff], b[:ff], x64), R.bound_gemm(a[ff:], b[ff:], x64)
    r.ratio = swiglu_ratio(r, r.aq, r.ad)
    return r


def swiglu_ratio(r, aq, ad):
    return ratio(np.abs(R.dequant_act(aq, ad) - R.swiglu64(r.G64, r.U64)), R.bound_swiglu_e2e(r.G64, r.U64, r.eg, r.eu, ad))


def _norm(L, s, rng, r):
    from test_gpu_linear import _norm_inputs
    st = dict(s.setup)
    r.f, r.h, r.g = _norm_inputs(rng, s.K, s.nt, st["nparts"], keys=bool(st["keys"]), slab_extra=16)
    r.xn, r.xq, r.xd = R.oracle_norm(L, r.h, r.g, 1e-6)


def norm_gemv_ref(L, s):
    """LOP_NORM_GEMV (GEMV_NORM): logits, h_out and xn_out bit for bit; the logits against unquantised float64 math within bound_e2e"""
    r = Ref()
    rng = np.random.default_rng(_seed(s))
    r.W, r.W_twin = weights(rng, s.types, s.rows, s.K)
    _norm(L, s, rng, r)
    r.want = R.oracle_slabs(L, r.W_twin, s.K, s.row0, s.nrows, r.xq, r.xd)[0]
    a, b = decode(r.W, s.K)
    a, b = a[s.row0:s.row0 + s.nrows], b[s.row0:s.row0 + s.nrows]
    xn64 = R.rmsnorm64(r.h, r.g, 1e-6)
    blk = np.abs(r.xn.reshape(s.nt, s.K // 32, 32)).max(-1) / 127
    r.y64 = xn64 @ (a - b).T
    r.bound = R.bound_e2e(a - b, xn64, r.xn - xn64, blk, a, b, R.dequant_act(r.xq, r.xd))
    r.ratio = ratio(np.abs(r.want - r.y64), r.bound)
    return r


def norm_gateup_ref(L, s):
    """LOP_NORM_GATEUP (GU_SWIGLU_NORM): aq / ad and h_out bit for bit"""
    r = Ref()
    ff = s.nrows // 2
    rng = np.random.default_rng(_seed(s))
    r.W, r.W_twin = weights(rng, s.types, s.rows, s.K)
    _norm(L, s, rng, r)
    gu = R.oracle_slabs(L, r.W_twin, s.K, 0, 2 * ff, r.xq, r.xd)[0]
    _, r.aq, r.ad = R.oracle_swiglu_quant(L, gu[:, :ff], gu[:, ff:])
    a, b = decode(r.W, s.K)
    x64 = R.dequant_act(r.xq, r.xd)
    r.G64, r.U64 = x64 @ (a[:ff] - b[:ff]).T, x64 @ (a[ff:] - b[ff:]).T
    r.eg, r.eu = R.bound_gemm(a[:ff], b[:ff], x64), R.bound_gemm(a[ff:], b[ff:], x64)
    r.ratio = swiglu_ratio(r, r.aq, r.ad)
    return r


ARGMAX_TIES = 4   # four tokens of an argmax case carry one tie each; the others are plain


def argmax_ref(L, s):
    """LOP_NORM_ARGMAX (GEMV_NORM_ARGMAX, lpr 2: 32 rows per workgroup).  Ties need no hand-built quants: the raw bytes of a token's best row,
    copied over a row of another 32-row group, give two bit-equal logits that are the token's maximum.  Tie i goes to the first token whose
    best row no earlier tie uses (r.toks[i]):
      tie 0: the copy is a valid row                              -> the lower index
      tie 1: the same, and the lower index is masked              -> the higher index
      tie 2: the copy lies beyond nrows_valid                     -> the original
      tie 3: the same, and the original is masked                 -> the best row of the others (the copy would win without the valid-row limit)
    -> r.toks, r.pairs[i] = (original, copy), r.mask, r.keys (linear_ref.greedy_key on the oracle's logits), r.logits"""
    r = Ref()
    st = dict(s.setup)
    nv, add = st["nrows_valid"], st["idx_add"]
    n = s.rows[0]
    assert len(s.types) == 1 and s.row0 == 0 and s.nrows == n and n - nv >= 2
    rng = np.random.default_rng(_seed(s))
    r.W, _ = weights(rng, s.types, s.rows, s.K)
    _norm(L, s, rng, r)
    logits = lambda: R.oracle_slabs(L, twins(r.W), s.K, 0, n, r.xq, r.xd)[0]
    armed = R.pack_key(-np.inf, 0)
    r.toks, r.pairs, used = [], [], set()
    for t in range(s.nt):
        i = len(r.pairs)
        if i == ARGMAX_TIES:
            break
        best = R.key_code(R.greedy_key(logits()[t, :nv], -1, 0, armed))
        if best in used:
            continue
        if i < 2:   # a valid row of another 32-row group that no earlier tie uses
            dst = next(c for c in ((best + 32 * j + 5) % nv for j in range(1, 4)) if c // 32 != best // 32 and c not in used)
        else:
            dst = nv + i - 2
        copy_row(r.W, s.K, best, dst)
        used.update((best, dst)); r.toks.append(t); r.pairs.append((best, dst))
    assert len(r.pairs) == ARGMAX_TIES, "too few tokens with a best row of their own: pick another seed"
    r.W_twin = twins(r.W)
    r.logits = logits()
    mask = np.full(s.nt, -1, np.int32)
    mask[r.toks[1]] = min(r.pairs[1]) + add; mask[r.toks[3]] = r.pairs[3][0] + add
    r.mask = mask
    r.armed = armed
    r.keys = [R.greedy_key(r.logits[t, :nv], int(mask[t]), add, armed) for t in range(s.nt)]
    return r


REF = {"GEMV": gemv_ref, "GATEUP": gateup_ref, "NORM_GEMV": norm_gemv_ref, "NORM_ARGMAX": argmax_ref, "NORM_GATEUP": norm_gateup_ref}


def reference(L, s):
    return REF[s.op](L, s)
