"""Each talker / predictor linear-layer form (q3tts_op_linear) against the oracle composition, bit for bit, and against float64 with the derived
bounds of tests/linear_ref.py.  Every form of an op must give the same bits; AUTO must equal the form it reports; bytes outside the logical
outputs (NaN-poisoned) must stay untouched; a forced form whose preconditions fail is refused with the outputs untouched."""
import numpy as np
import pytest

import linear_ref as R
import q3tts as Q

pytestmark = pytest.mark.gpu
POISON = np.uint32(0x7FC0DEAD)


def _poison(n):
    return np.full(n, POISON, np.uint32).view(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    """bit-equal, or NaN in both (NaN payloads are not part of the contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def _acts(rng, nt, k, a_rows=None):
    """int8 activations through the oracle's quantiser, with edge blocks: all-zero, one dominant element, tiny (f16-subnormal scale), -0;
    rows past ntok carry NaN scales"""
    from q3oracle import quant_act
    x = (rng.standard_normal((nt, k)) * rng.uniform(0.2, 3)).astype(np.float32)
    x[0, :32] = 0.0
    if k >= 128:
        x[-1, 32:64] = 0.0; x[-1, 40] = 50.0
        x[0, 64:96] = rng.standard_normal(32).astype(np.float32) * 1e-6
        x[0, 96:128] = -0.0
    a_rows = a_rows or nt + 2
    xq = np.zeros((a_rows, k), np.int8); xd = np.full((a_rows, k // 32), 0x7E00, np.uint16)
    xq[nt:] = 77
    for t in range(nt):
        xq[t], xd[t] = quant_act(x[t])
    return xq, xd


def _weights(rng, types, rows, k):
    return [(R.rand_rows(rng, t, n, k), t, n) for t, n in zip(types, rows)]


def _gu_weights(rng, qtype, ff, k):
    """gate rows then up rows: one Q8_0 tensor in the Q8_0 file layout, or two K-quant tensors of one type"""
    W = _weights(rng, [qtype] * 2, [ff, ff], k)
    return [(np.concatenate([W[0][0], W[1][0]]), 8, 2 * ff)] if qtype == 8 else W


GEMV_CASES = [  # (types, rows per tensor, K, ntok, row0, nrows, kq_layout)
    ([8], [32], 256, 1, 0, 32, 0), ([8], [33], 512, 3, 0, 33, 0), ([8], [100], 768, 5, 0, 100, 0), ([8], [96], 1024, 9, 32, 64, 0),
    ([8], [64], 2048, 17, 0, 64, 0), ([8], [128], 3072, 33, 64, 64, 0), ([8], [64], 6144, 13, 0, 64, 0), ([8], [4096], 2048, 2, 0, 4096, 0),
    ([8], [64], 1024, 129, 0, 64, 0), ([8], [128], 512, 64, 0, 128, 0), ([8], [32], 1024, 193, 0, 32, 0), ([8], [2048], 6144, 16, 0, 2048, 0),
    ([8], [64], 1024, 15, 0, 64, 0), ([8], [64], 2048, 128, 0, 64, 0), ([8], [32], 1024, 160, 0, 32, 0), ([8], [64], 768, 192, 0, 64, 0),
    ([8], [32], 512, 256, 0, 32, 0), ([8], [32], 256, 300, 0, 32, 0), ([13, 14], [32, 32], 1024, 300, 0, 64, 1),
    ([13], [64], 1024, 4, 0, 64, 1), ([14], [64], 3072, 32, 0, 64, 1), ([13, 14, 8], [32, 32, 64], 2048, 8, 0, 128, 1),
    ([13, 14, 8], [32, 32, 32], 6144, 40, 32, 64, 1), ([8], [64], 512, 2, 0, 64, 1),
    ([13, 8, 14], [32, 32, 32], 256, 2, 0, 96, 1), ([13, 14, 13], [32, 32, 32], 256, 17, 0, 96, 1),  # a Q8_0 tensor between two others; a type that returns
]


def _gemv_forms(types, k, nt, nrows, kq, stride, off):
    if kq:
        return [("GEMV_KQ", dict(lpr=2, mt=1)), ("GEMV_KQ", dict(lpr=4, mt=8)), ("GEMV_KQ", dict(lpr=8, mt=2)), ("GEMM_KQ_MFMA", dict(ztiles=1))]
    f = [("GEMV_Q8", dict(lpr=2, mt=4)), ("GEMV_Q8", dict(lpr=8, mt=1)), ("GEMV_Q8", dict(lpr=4, mt=8)), ("GEMM_Q8_TOK", {}),
         ("GEMM_Q8_MFMA", dict(ztiles=1)), ("GEMM_Q8_MFMA", dict(ztiles=(nt + 31) // 32))]
    if k <= 1024 and nrows % 4 == 0 and stride % 4 == 0 and off % 4 == 0:
        f.append(("GEMM_Q8_TILE1", {}))
    return f


@pytest.mark.parametrize("case", GEMV_CASES, ids=lambda c: "k%d_n%d_t%d_%s" % (c[2], c[5], c[3], "-".join(map(str, c[0]))))
def test_gemv_forms(gpu, oracle, case):
    types, rows, k, nt, row0, nrows, kq = case
    rng = np.random.default_rng(k * 7 + nt)
    W = _weights(rng, types, rows, k)
    xq, xd = _acts(rng, nt, k)
    nss = (k // 256 + 7) // 8
    # odd token counts: out_off 3 (4-byte, not 16-byte aligned: AUTO must fall back from tile1)
    stride, off = (nrows + 4 if nrows % 4 == 0 else nrows + 5), (3 if nt % 2 else 4)
    want = R.oracle_slabs(oracle.lib(), W, k, row0, nrows, xq[:nt], xd[:nt])
    a, b = R.decode_parts(W, k)
    a, b = a[row0:row0 + nrows], b[row0:row0 + nrows]
    x64 = R.dequant_act(xq[:nt], xd[:nt])
    y = R.sum_slabs(want).astype(np.float64)
    assert (np.abs(y - x64 @ (a - b).T) <= R.bound_gemm(a, b, x64)).all()
    first = None
    for form, kw in [("AUTO", {})] + _gemv_forms(types, k, nt, nrows, kq, stride, off):
        out = _poison(off + nss * nt * stride + 7)
        ran = Q.op_linear(Q.LOP_GEMV, form, W, K=k, row0=row0, nrows=nrows, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], out=out,
                          out_off=off, out_stride=stride, kq_layout=kq, **kw)
        got = out[off:off + nss * nt * stride].reshape(nss, nt, stride)
        assert np.array_equal(_bits(got[:, :, :nrows]), _bits(want)), (form, kw, ran)
        pad = np.concatenate([out[:off], out[off + nss * nt * stride:], got[:, :, nrows:].reshape(-1)])
        assert (_bits(pad) == POISON).all(), (form, "stray write")
        if form != "AUTO":
            assert ran[0] == form
        if first is None:
            first = _bits(got[:, :, :nrows]).copy()
        assert np.array_equal(_bits(got[:, :, :nrows]), first), (form, "differs from AUTO")


GU_CASES = [([8], 1024, 64, 16), ([8], 2048, 96, 33), ([8], 1024, 32, 129), ([13], 1024, 64, 40), ([14], 2048, 32, 17), ([8], 2048, 6144, 16),
            ([8], 1024, 64, 300), ([8], 1024, 32, 5)]


@pytest.mark.parametrize("case", GU_CASES, ids=lambda c: "k%d_ff%d_t%d_%d" % (c[1], c[2], c[3], c[0][0]))
def test_gateup_forms(gpu, oracle, case):
    types, k, ff, nt = case
    kq = types[0] != 8
    rng = np.random.default_rng(k + ff + nt)
    W = _gu_weights(rng, types[0], ff, k)
    xq, xd = _acts(rng, nt, k)
    sl = R.oracle_slabs(oracle.lib(), W, k, 0, 2 * ff, xq[:nt], xd[:nt])
    gu = R.sum_slabs(sl)
    act, aq_w, ad_w = R.oracle_swiglu_quant(oracle.lib(), gu[:, :ff], gu[:, ff:])
    # (c) for gate/up: the quantised activations against SwiGLU of the float64 products of the same int8 inputs
    a, b = R.decode_parts(W, k)
    x64 = R.dequant_act(xq[:nt], xd[:nt])
    G64, U64 = x64 @ (a[:ff] - b[:ff]).T, x64 @ (a[ff:] - b[ff:]).T
    eg, eu = R.bound_gemm(a[:ff], b[:ff], x64), R.bound_gemm(a[ff:], b[ff:], x64)
    err = np.abs(R.dequant_act(aq_w, ad_w) - R.swiglu64(G64, U64))
    assert (err <= R.bound_swiglu_e2e(G64, U64, eg, eu, ad_w)).all()
    ntiles = (nt + 31) // 32
    forms = [("AUTO", {}), ("GU_UNFUSED", {})]
    forms += [("GU_KQ_MFMA", dict(ztiles=ntiles)), ("GU_KQ_MFMA", dict(ztiles=(ntiles + 3) // 4))] if kq else \
             [("GU_Q8_TILE1", {}), ("GU_Q8_MFMA", dict(ztiles=(ntiles + 3) // 4)), ("GU_Q8_MFMA", dict(ztiles=ntiles))]
    for form, kw in forms:
        aq = np.full((nt, ff), 55, np.int8); ad = np.full((nt, ff // 32), 0x7E00, np.uint16)
        ran = Q.op_linear(Q.LOP_GATEUP, form, W, K=k, nrows=2 * ff, ff=ff, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], aq=aq, ad=ad,
                          kq_layout=int(kq), **kw)
        assert np.array_equal(aq, aq_w) and np.array_equal(ad, ad_w), (form, kw, ran)


def _norm_inputs(rng, d, nt, nparts, keys=False, idx=False, slab_extra=0):
    hrows = nt + 3
    h_in = (rng.standard_normal((hrows, d)) * rng.uniform(0.1, 10)).astype(np.float32)
    h_in[1] = 0.0
    sel = np.arange(nt)
    f = {}
    if keys or idx:
        sel = rng.integers(0, hrows, nt); sel[-1] = sel[0]
        f["idx_stride"] = 2
        if keys:
            k = np.zeros(2 * nt, np.uint64); k[::2] = [R.pack_key(1.0, int(s)) for s in sel]; f["idx_keys"] = k
        else:
            ii = np.zeros(2 * nt, np.int32); ii[::2] = sel; f["idx"] = ii
    pstride = d + 8
    slab = nt * pstride + slab_extra
    parts = (rng.standard_normal(max(nparts, 1) * slab + 4) * 0.5).astype(np.float32)
    if nparts:
        f.update(parts=parts, nparts=nparts, parts_stride=pstride, parts_slab=slab)
    P = np.stack([np.stack([parts[s * slab + t * pstride:s * slab + t * pstride + d] for t in range(nt)]) for s in range(nparts)]) if nparts else None
    h = R.residual(h_in[sel], P, nparts)
    g = rng.uniform(0.5, 1.5, d).astype(np.float32)
    f.update(h_in=h_in, h_stride=d, g=g)
    return f, h, g


NORM_CASES = [(256, 1, 0, "", 1e-6), (512, 3, 1, "keys", 1e-5), (1024, 9, 2, "", 1e-6), (2048, 5, 3, "idx", 1e-6), (1024, 17, 5, "", 1e-5),
              (2048, 33, 1, "keys", 1e-6)]


@pytest.mark.parametrize("d,nt,nparts,sel,eps", NORM_CASES)
def test_norm_forms(gpu, oracle, d, nt, nparts, sel, eps):
    rng = np.random.default_rng(d + nt + nparts)
    f, h, g = _norm_inputs(rng, d, nt, nparts, keys=sel == "keys", idx=sel == "idx")
    xn_w, xq_w, xd_w = R.oracle_norm(oracle.lib(), h, g, eps)
    xn64 = R.rmsnorm64(h, g, eps)
    assert (np.abs(xn_w - xn64) <= R.bound_norm(xn64, d)).all()
    assert R.quant_check(xn_w, xq_w, xd_w)
    for form in ["AUTO", "NORM"] + (["NORM_WG"] if sel != "idx" else []):
        xq = np.full((nt, d), 9, np.int8); xd = np.zeros((nt, d // 32), np.uint16); hout = _poison(nt * d); xn = _poison(nt * d)
        Q.op_linear(Q.LOP_NORM, form, K=d, nrows=1, ntok=nt, eps=eps, xq_out=xq, xd_out=xd, h_out=hout, xn_out=xn, **f)
        assert np.array_equal(xq, xq_w) and np.array_equal(xd, xd_w), form
        assert np.array_equal(_bits(hout.reshape(nt, d)), _bits(h)) and np.array_equal(_bits(xn.reshape(nt, d)), _bits(xn_w)), form


NORM_GEMV_CASES = [([8], 1024, 96, 1, 3, (1,)), ([8], 2048, 64, 5, 1, (1, 4, 8)), ([8], 256, 33, 13, 0, (8,)), ([13, 14, 8], 2048, 96, 3, 2, (2, 4)),
                   ([8], 1024, 16384, 2, 1, (2,)), ([8], 512, 100, 9, 2, (8,))]


@pytest.mark.parametrize("types,d,rows,nt,nparts,mts", NORM_GEMV_CASES)
def test_gemv_norm(gpu, oracle, types, d, rows, nt, nparts, mts):
    rng = np.random.default_rng(d + rows + nt)
    kq = int(len(types) > 1)
    per = [rows // len(types)] * len(types) if kq else [rows]
    W = _weights(rng, types, per, d)
    f, h, g = _norm_inputs(rng, d, nt, nparts, keys=nt > 2, slab_extra=16)
    xn_w, xq_w, xd_w = R.oracle_norm(oracle.lib(), h, g, 1e-6)
    want = R.oracle_slabs(oracle.lib(), W, d, 0, rows, xq_w, xd_w)[0]
    # (c): the fused chain against unquantised float64 math
    a, b = R.decode_parts(W, d)
    xn64 = R.rmsnorm64(h, g, 1e-6)
    blk = np.abs(xn_w.reshape(nt, d // 32, 32)).max(-1) / 127
    err = np.abs(want - xn64 @ (a - b).T)
    assert (err <= R.bound_e2e(a - b, xn64, xn_w - xn64, blk, a, b, R.dequant_act(xq_w, xd_w))).all()
    stride = rows + 3
    for form, kw in [("AUTO", {})] + [("GEMV_NORM", dict(lpr=l, mt=m)) for l in (2, 4, 8) for m in mts]:
        out = _poison(5 + nt * stride)
        hout = _poison(nt * d); xn = _poison(nt * d)
        ran = Q.op_linear(Q.LOP_NORM_GEMV, form, W, K=d, nrows=rows, ntok=nt, eps=1e-6, out=out, out_off=5, out_stride=stride, h_out=hout,
                          xn_out=xn, kq_layout=kq, **kw, **f)
        got = out[5:].reshape(nt, stride)
        assert np.array_equal(_bits(got[:, :rows]), _bits(want)), (form, kw, ran)
        assert (_bits(got[:, rows:]) == POISON).all() and (_bits(out[:5]) == POISON).all()
        assert np.array_equal(_bits(hout.reshape(nt, d)), _bits(h)) and np.array_equal(_bits(xn.reshape(nt, d)), _bits(xn_w))


@pytest.mark.parametrize("types,d,ff,nt,nparts", [([8], 1024, 64, 1, 1), ([8], 2048, 96, 2, 3), ([8], 512, 32, 7, 0), ([13], 1024, 64, 3, 2),
                                                  ([14], 2048, 32, 5, 1)])
def test_gateup_swiglu_norm(gpu, oracle, types, d, ff, nt, nparts):
    rng = np.random.default_rng(d + ff + nt)
    kq = int(types[0] != 8)
    W = _gu_weights(rng, types[0], ff, d)
    f, h, g = _norm_inputs(rng, d, nt, nparts, keys=True)
    xn_w, xq_w, xd_w = R.oracle_norm(oracle.lib(), h, g, 1e-6)
    gu = R.oracle_slabs(oracle.lib(), W, d, 0, 2 * ff, xq_w, xd_w)[0]
    act, aq_w, ad_w = R.oracle_swiglu_quant(oracle.lib(), gu[:, :ff], gu[:, ff:])
    for form, kw in [("AUTO", {}), ("GU_SWIGLU_NORM", dict(mt=1)), ("GU_SWIGLU_NORM", dict(mt=2)), ("GU_SWIGLU_NORM", dict(mt=4))]:
        aq = np.full((nt, ff), 55, np.int8); ad = np.zeros((nt, ff // 32), np.uint16); hout = _poison(nt * d)
        ran = Q.op_linear(Q.LOP_NORM_GATEUP, form, W, K=d, nrows=2 * ff, ff=ff, ntok=nt, eps=1e-6, aq=aq, ad=ad, h_out=hout, kq_layout=kq, **kw, **f)
        assert np.array_equal(aq, aq_w) and np.array_equal(ad, ad_w), (form, kw, ran)
        assert np.array_equal(_bits(hout.reshape(nt, d)), _bits(h))


def _q8_row(q, scale):
    """one raw Q8_0 row from int8 quants q [K] and per-block f16 scales (scalar or [K/32])"""
    k = q.size
    raw = np.zeros((k // 32, 34), np.uint8)
    raw[:, :2] = np.broadcast_to(np.asarray(scale, np.float16), (k // 32,)).copy().view(np.uint8).reshape(-1, 2)
    raw[:, 2:] = q.astype(np.int8).view(np.uint8).reshape(-1, 32)
    return raw.reshape(-1)


ARGMAX_ROWS, ARGMAX_NV, C_PINF, C_NINF = 256, 200, 300, 700


def argmax_problem(rng, d=1024, nt=5):
    """weights and inputs built so that each token exercises one rule of the epilogue (LPR 2: 32 rows per workgroup):
    t0: equal maxima in rows 5 and 150 (two workgroups)            -> 5
    t1: equal maxima in rows 40 and 41, row 40 masked              -> 41
    t2: equal maxima in rows 70 and 190, row 70 masked             -> 190
    t3: row 100 is +inf (one block with an inf f16 scale and an isum > 0), a finite maximum at 120   -> 100
    t4: row 10 is -inf, the maximum at 230 is a padding row past nrows_valid, the runner-up at 12     -> 12
    The inf-scale blocks see a zero isum (-> NaN) for every other token: h is zero in that column there."""
    h = (rng.standard_normal((nt, d)) * 2).astype(np.float32)
    h[:, C_PINF] = 0.0; h[3, C_PINF] = 8.0
    h[:, C_NINF] = 0.0; h[4, C_NINF] = 8.0
    g = rng.uniform(0.5, 1.5, d).astype(np.float32)
    from q3oracle import lib
    _, xq, _ = R.oracle_norm(lib(), h, g, 1e-6)
    raw = R.rand_rows(rng, 8, ARGMAX_ROWS, d, scale=0.1).reshape(ARGMAX_ROWS, -1)
    dom = lambda t, s=0.05: _q8_row(127 * np.sign(xq[t]).astype(np.int64), s)
    for t, rows in ((0, (5, 150)), (1, (40, 41)), (2, (70, 190)), (3, (120,)), (4, (230,))):
        for r in rows:
            raw[r] = dom(t)
    raw[12] = dom(4, 0.025)
    for r, t, c, sign in ((100, 3, C_PINF, 1), (10, 4, C_NINF, -1)):
        q = np.zeros(d, np.int64); q[c] = sign * 127 * np.sign(xq[t, c])
        sc = np.full(d // 32, 0.01); sc[c // 32] = np.inf
        raw[r] = _q8_row(q, sc)
    raw[3] = _q8_row(rng.integers(-127, 128, d), np.nan)   # a NaN row for every token
    mask = np.array([-1, 40, 70, -1, -1], np.int32)
    return raw.reshape(-1), h, g, mask, [5, 41, 190, 100, 12]


@pytest.mark.parametrize("idx_add", [0, 7])
def test_argmax_epilogue(gpu, oracle, idx_add):
    d, nt = 1024, 5
    rng = np.random.default_rng(11)
    raw, h, g, mask, winners = argmax_problem(rng, d, nt)
    W = [(raw, 8, ARGMAX_ROWS)]
    _, xq_w, xd_w = R.oracle_norm(oracle.lib(), h, g, 1e-6)
    logits = R.oracle_slabs(oracle.lib(), W, d, 0, ARGMAX_ROWS, xq_w, xd_w)[0]
    # the situations the problem is built for really occur
    assert logits[0, 5] == logits[0, 150] and logits[1, 40] == logits[1, 41] and logits[2, 70] == logits[2, 190]
    assert logits[3, 100] == np.inf and logits[4, 10] == -np.inf and np.isnan(logits[np.arange(nt) != 3, 100]).all()
    assert logits[4, 230] > logits[4, 12] and np.isnan(logits[:, 3]).all()
    armed = R.pack_key(-np.inf, 0)
    # the mask names the true maximum of t1 / t2, and without the valid-row limit t4 would take the padding row
    assert [R.key_code(R.greedy_key(logits[t, :ARGMAX_NV], -1, 0, armed)) for t in (1, 2)] == [40, 70]
    assert R.key_code(R.greedy_key(logits[4], -1, 0, armed)) == 230
    masks = np.where(mask >= 0, mask + idx_add, -1).astype(np.int32)
    want = [R.greedy_key(logits[t, :ARGMAX_NV], int(masks[t]), idx_add, armed) for t in range(nt)]
    assert [R.key_code(k) - idx_add for k in want] == winners
    f = dict(h_in=h, h_stride=d, g=g)
    for form, kw in [("AUTO", {}), ("GEMV_NORM_ARGMAX", dict(mt=1)), ("GEMV_NORM_ARGMAX", dict(mt=4))]:
        keys = np.full(3 * nt, armed, np.uint64)
        Q.op_linear(Q.LOP_NORM_ARGMAX, form, W, K=d, nrows=ARGMAX_ROWS, nrows_valid=ARGMAX_NV, ntok=nt, eps=1e-6, keys=keys, key_stride=3,
                    idx_add=idx_add, mask_per_tok=masks, **kw, **f)
        got = keys.reshape(nt, 3)
        assert [int(k) for k in got[:, 0]] == want, (form, kw, [R.key_code(int(k)) - idx_add for k in got[:, 0]])
        assert (got[:, 1:] == armed).all()
    # the same form's EPI = 0 logits are the oracle's
    out = np.zeros(nt * ARGMAX_ROWS, np.float32)
    Q.op_linear(Q.LOP_NORM_GEMV, "GEMV_NORM", W, K=d, nrows=ARGMAX_ROWS, ntok=nt, eps=1e-6, out=out, out_stride=ARGMAX_ROWS, lpr=2, **f)
    assert _same(out.reshape(nt, ARGMAX_ROWS), logits)


def test_argmax_all_masked_keeps_armed_key(gpu):
    """contract (kernels.h ArgmaxEpi): a token with no eligible row keeps the armed key (code 0), whatever idx_add is"""
    d, rows = 256, 32
    rng = np.random.default_rng(1)
    raw = R.rand_rows(rng, 8, rows, d).reshape(rows, d // 32, 34)
    raw[:, :, :2] = np.array([np.nan] * (d // 32), np.float16).view(np.uint8).reshape(-1, 2)
    f, h, g = _norm_inputs(rng, d, 2, 0)
    armed = R.pack_key(-np.inf, 0)
    keys = np.full(2, armed, np.uint64)
    Q.op_linear(Q.LOP_NORM_ARGMAX, "AUTO", [(raw.reshape(-1), 8, rows)], K=d, nrows=rows, nrows_valid=rows, ntok=2, eps=1e-6, keys=keys, key_stride=1,
                idx_add=40, **f)
    assert (keys == armed).all()


@pytest.mark.parametrize("wtype,k,rows,nt,row0", [(0, 256, 64, 1, 0), (1, 1024, 128, 5, 64), (30, 2048, 192, 33, 0), (30, 1024, 128, 100, 64),
                                                   (1, 512, 64, 130, 0), (0, 3072, 64, 16, 0)])
def test_float_forms(gpu, oracle, wtype, k, rows, nt, row0):
    rng = np.random.default_rng(wtype + k + nt)
    w = (rng.standard_normal((rows + row0, k)) * 0.05).astype(np.float32)
    raw = w if wtype == 0 else w.astype(np.float16) if wtype == 1 else (w.view(np.uint32) >> 16).astype(np.uint16)
    x = np.zeros(nt * (k + 4) + 4, np.float32)
    X = (rng.standard_normal((nt, k))).astype(np.float32)
    X[0, :8] = [0.0, -0.0, 1e-40, -1e-40, 0, 0, 0, 0]
    for t in range(nt):
        x[4 + t * (k + 4):4 + t * (k + 4) + k] = X[t]
    nrows = rows
    want = R.oracle_float(oracle.lib(), np.ascontiguousarray(raw), wtype, k, row0, nrows, X)
    wd = raw.astype(np.float64) if wtype != 30 else (raw.astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    y64 = X.astype(np.float64) @ wd[row0:row0 + nrows].T
    assert (np.abs(want - y64) <= R.gamma(k // 8 + 16) * (np.abs(X) @ np.abs(wd[row0:row0 + nrows]).T)).all()
    for form in ["AUTO", "F_GEMV", "F_MFMA16", "F_MFMA"]:
        out = _poison(nt * (nrows + 2) + 1)
        Q.op_linear(Q.LOP_F_GEMV, form, [(raw, wtype, rows + row0)], K=k, row0=row0, nrows=nrows, ntok=nt, x=x, x_off=4, x_stride=k + 4,
                    out=out, out_off=1, out_stride=nrows + 2)
        got = out[1:].reshape(nt, nrows + 2)
        assert np.array_equal(_bits(got[:, :nrows]), _bits(want)), form
        assert (_bits(got[:, nrows:]) == POISON).all()
    # gate/up + SwiGLU over the same matrix split in two halves
    if row0 == 0 and rows % 32 == 0:
        ff = rows // 2
        act_w, _, _ = R.oracle_swiglu_quant(oracle.lib(), want[:, :ff], want[:, ff:])
        for form in ["AUTO", "F_GU_MFMA16", "F_GU_UNFUSED"]:
            out = _poison(nt * ff)
            Q.op_linear(Q.LOP_F_GATEUP, form, [(raw, wtype, rows)], K=k, nrows=rows, ff=ff, ntok=nt, x=x, x_off=4, x_stride=k + 4, out=out,
                        out_stride=ff)
            assert np.array_equal(_bits(out.reshape(nt, ff)), _bits(act_w)), form


def test_refusals_leave_outputs_untouched(gpu):
    rng = np.random.default_rng(5)
    W = [(R.rand_rows(rng, 8, 36, 2048), 8, 36)]
    xq, xd = _acts(rng, 40, 2048)
    out = _poison(2 * 40 * 40)
    bad = [("GEMM_Q8_TILE1", dict(K=2048, nrows=36)),                  # K > 1024 and nrows % 4 != 0
           ("GEMV_KQ", dict(K=2048, nrows=36)),                        # Q8_0 layout
           ("GEMM_Q8_MFMA", dict(K=2048, nrows=36, ztiles=3)),         # ztiles > token tiles
           ("GEMV_Q8", dict(K=2048, nrows=36, lpr=16)),
           ("GEMV_Q8", dict(K=2048, nrows=37)),                        # rows past the matrix
           ("GEMV_NORM", dict(K=2048, nrows=36))]                      # wrong op for the form
    for form, kw in bad:
        with pytest.raises(RuntimeError):
            Q.op_linear(Q.LOP_GEMV, form, W, ntok=40, xq=xq, xd=xd, a_rows=xq.shape[0], out=out, out_stride=40, **kw)
        assert (_bits(out) == POISON).all(), form
    with pytest.raises(RuntimeError):   # tile1 with a 4-byte aligned but not 16-byte aligned out
        Q.op_linear(Q.LOP_GEMV, "GEMM_Q8_TILE1", [(R.rand_rows(rng, 8, 32, 1024), 8, 32)], K=1024, nrows=32, ntok=20, xq=xq[:, :1024].copy(),
                    xd=xd[:, :32].copy(), a_rows=xq.shape[0], out=out, out_off=1, out_stride=32)
    assert (_bits(out) == POISON).all()
    f, h, g = _norm_inputs(rng, 1024, 3, 0, idx=True)
    with pytest.raises(RuntimeError):   # int32 row indices: NORM only
        Q.op_linear(Q.LOP_NORM, "NORM_WG", K=1024, nrows=1, ntok=3, eps=1e-6, xq_out=np.zeros((3, 1024), np.int8), xd_out=np.zeros((3, 32), np.uint16), **f)
    fw = [((rng.standard_normal((64, 256)) * 0.1).astype(np.float32), 0, 64)]
    x = np.zeros(4 * 256 + 1, np.float32)
    with pytest.raises(RuntimeError):   # float matrix cores need a 16-byte x
        Q.op_linear(Q.LOP_F_GEMV, "F_MFMA16", fw, K=256, nrows=64, ntok=4, x=x, x_off=1, x_stride=256, out=out, out_stride=64)
    aq, ad = np.full((40, 32), 55, np.int8), np.full((40, 1), 77, np.uint16)
    gu = dict(nrows=64, ff=32, ntok=40, a_rows=xq.shape[0], aq=aq, ad=ad)
    for form, K, kw in [("GU_Q8_MFMA", 512, {}),                   # fused gate/up needs K in {1024, 2048}
                        ("GU_Q8_TILE1", 1024, dict(ztiles=1)),      # tile1: ztiles == token tiles (2)
                        ("GU_Q8_MFMA", 1024, dict(ztiles=3)),       # ztiles above the token tiles
                        ("GU_UNFUSED", 3072, {}),                   # k_swiglu_quant reads one super-segment slab: K <= 2048
                        ("GU_KQ_MFMA", 1024, {})]:                  # Q8_0 layout
        with pytest.raises(RuntimeError):
            Q.op_linear(Q.LOP_GATEUP, form, [(R.rand_rows(rng, 8, 64, K), 8, 64)], K=K, xq=np.zeros((42, K), np.int8),
                        xd=np.zeros((42, K // 32), np.uint16), **gu, **kw)
        assert (aq == 55).all() and (ad == 77).all(), form
    f3, _, _ = _norm_inputs(rng, 3072, 2, 0)
    with pytest.raises(RuntimeError):   # the norm prologue holds K <= 2048
        Q.op_linear(Q.LOP_NORM_GEMV, "GEMV_NORM", [(R.rand_rows(rng, 8, 32, 3072), 8, 32)], K=3072, nrows=32, ntok=2, eps=1e-6, out=out,
                    out_stride=32, **f3)
    f1, _, _ = _norm_inputs(rng, 1024, 2, 0)
    with pytest.raises(RuntimeError):   # gate and up rows of two tensor types
        Q.op_linear(Q.LOP_NORM_GATEUP, "GU_SWIGLU_NORM", [(R.rand_rows(rng, 13, 32, 1024), 13, 32), (R.rand_rows(rng, 14, 32, 1024), 14, 32)],
                    K=1024, nrows=64, ff=32, ntok=2, eps=1e-6, aq=aq, ad=ad, kq_layout=1, **f1)
    assert (aq == 55).all() and (ad == 77).all()
    xa = np.zeros(4 * 256, np.float32)
    fw2 = [((rng.standard_normal((160, 256)) * 0.1).astype(np.float32), 0, 160)]
    with pytest.raises(RuntimeError):   # F_GU_MFMA16: ff % 16 == 0
        Q.op_linear(Q.LOP_F_GATEUP, "F_GU_MFMA16", [(fw2[0][0][:80].copy(), 0, 80)], K=256, nrows=80, ff=40, ntok=4, x=xa, x_stride=256, out=out,
                    out_stride=40)
    with pytest.raises(RuntimeError):   # float matrix cores: row0 % 64 == 0
        Q.op_linear(Q.LOP_F_GEMV, "F_MFMA", fw2, K=256, row0=32, nrows=64, ntok=4, x=xa, x_stride=256, out=out, out_stride=64)
    assert (_bits(out) == POISON).all()
