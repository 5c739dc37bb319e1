"""The numpy restatement of the ggml-mode arithmetic (tests/ggml_mode_ref.py) against the oracle (oracle/q3o_ggml.c), bit for bit, on every
case the GPU file runs (tests/ggml_mode_cases.py); and the oracle alone inside the float64 bounds.  No GPU.

Should the two ever disagree, the one outside the float64 bound on dequantised operands is wrong; with both inside, ggml_ref's dequantisers
(the block-format reading the rest of the suite already trusts) decide.  The worst ratio to each bound is printed per family; DESIGN.md
("ggml-mode kernel tests") records them."""
import ctypes as C

import numpy as np
import pytest

import ggml_mode_cases as K
import ggml_mode_ref as R
import ggml_ref
import linear_ref as LR

F = np.float32
_WORST = {}


def _note(family, ratio):
    _WORST[family] = max(_WORST.get(family, 0.0), float(ratio))
    print("worst |err| / bound, %s: %.3f (this case %.3f)" % (family, _WORST[family], ratio))


def _ratio(y, y64, bound):
    err = np.abs(np.asarray(y, np.float64) - y64)
    assert np.all(err <= bound), (float(err.max()), float((err / bound).max()))
    return float((err / bound).max())


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def L(oracle):
    lib = oracle.lib()
    lib.q3o_quant_q8_0_ggml.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    lib.q3o_quant_q8_K_ggml.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.q3o_matvec_ggml.argtypes = [C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
    lib.q3o_rmsnorm_ggml.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p]
    lib.q3o_swiglu_ggml.restype = C.c_float
    lib.q3o_swiglu_ggml.argtypes = [C.c_float, C.c_float]
    return lib


def oracle_quantize(lib, x):
    nt, k = x.shape
    q8 = np.zeros((nt, k), np.int8); d8 = np.zeros((nt, k // 32), np.uint16)
    qk = np.zeros((nt, k), np.int8); dk = np.zeros((nt, k // 256), F); bs = np.zeros((nt, k // 16), np.int16)
    for t in range(nt):
        xt = np.ascontiguousarray(x[t], F)
        lib.q3o_quant_q8_0_ggml(_p(xt), k, _p(q8[t]), _p(d8[t]))
        lib.q3o_quant_q8_K_ggml(_p(xt), k, _p(qk[t]), _p(dk[t]), _p(bs[t]))
    return q8, d8, qk, dk, bs


def oracle_swiglu(lib, g, u):
    return np.array([lib.q3o_swiglu_ggml(float(a), float(b)) for a, b in zip(g, u)], F)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("k,ntok", K.QUANT_CASES)
def test_quantisers_equal_the_oracle(L, k, ntok):
    x, names = K.quant_case(k, ntok)
    ref, orc = K.quant_ref(k, ntok), oracle_quantize(L, x)
    for name, a, b in zip(("q8", "d8", "qk", "dk", "bs"), ref, orc):
        assert _same(a, b), (name, names)
    # and each quantiser alone keeps its contract on the values it wrote: |x - q d| <= d / 2 (1 + 1e-5), d the f32 scale before it is stored (Q8_0
    # stores f16(d), which may underflow to 0: compared above by bits); Q8_K's d = -max / 127, so the element that set it comes back as -127 d
    q8, d8, qk, dk, bs = ref
    dd = np.repeat(np.abs(x.astype(np.float64)).reshape(ntok, k // 32, 32).max(-1) / 127, 32, axis=-1)
    assert np.all(np.abs(x - q8 * dd) <= dd * (0.5 + 127e-5))
    ddk = np.repeat(np.abs(dk.astype(np.float64)), 256, axis=-1)
    assert np.all(np.abs(x - qk * np.repeat(dk.astype(np.float64), 256, axis=-1)) <= ddk * (0.5 + 127e-5))
    assert np.array_equal(bs, qk.astype(np.int32).reshape(ntok, k // 16, 16).sum(-1))


def test_edge_blocks_are_what_they_claim():
    """every edge of the list is in some case, and does what its name says in the restatement's output"""
    seen = set()
    for k, ntok in K.QUANT_CASES:
        x, names = K.quant_case(k, ntok)
        q8, d8, qk, dk, bs = K.quant_ref(k, ntok)
        for t in range(ntok):
            for s, name in enumerate(names[t]):
                seen.add(name)
                xs, q8s, qks = x[t, 256 * s:256 * s + 256], q8[t, 256 * s:256 * s + 256], qk[t, 256 * s:256 * s + 256]
                d8s = d8[t, 8 * s:8 * s + 8].view(np.float16)
                if name == "zero_super":
                    assert dk[t, s] == 0 and not qks.any() and not bs[t, 16 * s:16 * s + 16].any() and not d8s.any()
                elif name == "zero_block":
                    assert d8s[2] == 0 and not q8s[64:96].any() and dk[t, s] != 0
                elif name == "tiny":
                    assert not d8[t, 8 * s:8 * s + 8].any() and dk[t, s] != 0 and (xs != 0).sum() > 200   # the f16 scale underflowed
                    assert (np.abs(xs[xs != 0]) < 1.2e-38).sum() > 200
                elif name == "neg_max":
                    assert dk[t, s] > 0 and qks[100] == -127 and q8s[100] == -127     # iscale = -127 / max > 0, d = 1 / iscale
                elif name == "equal_opposite":
                    assert qks[5] == -127 and qks[200] == 127 and dk[t, s] < 0
                elif name == "tie_q8_0":
                    assert np.all(d8s == np.float16(0.125)) and dk[t, s] == F(-0.125) and qks[0] == -127 and qks[31] == 127
                elif name == "tie_q8_K":
                    assert np.all(d8s == np.float16(4)) and dk[t, s] == F(4) and qks[0] == -127 and qks[31] == 127
                elif name == "neg_zero":
                    assert np.signbit(xs[32:64]).all() and not q8s[32:64].any() and d8s[1] == 0
    assert seen >= set(K.EDGE_NAMES), set(K.EDGE_NAMES) - seen


def test_tie_rows_separate_the_two_rounding_rules():
    """roundf (Q8_0: half away from zero) and nearest_int (Q8_K: half to even) must not be interchangeable on the tie rows"""
    x = K.tie_rows()
    even = lambda v: np.rint(np.asarray(v, F)).astype(F)
    q_away, d_away = R.quantize_row_q8_0(x)
    q_even, d_even = R.quantize_row_q8_0(x, rnd=even)
    assert np.array_equal(d_away, d_even)
    diff = q_away != q_even
    assert diff.sum() >= 100 and np.all(np.abs(q_away[diff].astype(int)) == np.abs(q_even[diff].astype(int)) + 1)   # away from zero is one further out
    k_even = R.quantize_row_q8_K(x)
    k_away = R.quantize_row_q8_K(x, rnd=lambda v: R.roundf(v).astype(np.int64))
    assert np.array_equal(k_even[1], k_away[1]) and (k_even[0] != k_away[0]).sum() >= 100
    assert not np.array_equal(k_even[2], k_away[2])
    # every non-maximum element really is a tie: x * id has fraction one half exactly
    for row, scale in ((x[0], F(8)), (x[1], F(0.25))):
        v = row * scale
        assert np.all((np.abs(v) == 127) | (np.abs(v - np.trunc(v)) == 0.5))
    # the rules themselves, on the bare numbers
    assert R.roundf(np.array([0.5, 1.5, 2.5, -0.5, -2.5, 0.49999997], F)).tolist() == [1, 2, 3, -1, -3, 0]
    assert R.nearest_int(np.array([0.5, 1.5, 2.5, -0.5, -2.5, -3.5], F)).tolist() == [0, 2, 2, 0, -2, -4]


def test_case_set_holds_negative_q6k_scales():
    assert K.n_negative_q6k_scales() > 0
    print("negative Q6_K sub-block scales in the dot cases: %d" % K.n_negative_q6k_scales())


@pytest.mark.parametrize("qtype,n,k,row0,nrows,ntok", K.DOT_CASES)
def test_dots_equal_the_oracle_and_float64(L, qtype, n, k, row0, nrows, ntok):
    raw, x = K.dot_case(qtype, n, k, row0, nrows, ntok)
    act, y = K.dot_ref(qtype, n, k, row0, nrows, ntok)
    rb = R.ROW_BYTES[qtype](k)
    rows = np.ascontiguousarray(raw.reshape(n, rb)[row0:row0 + nrows])
    yo = np.zeros((ntok, nrows), F)
    for t in range(ntok):
        xt = np.ascontiguousarray(x[t], F)
        L.q3o_matvec_ggml(qtype, _p(rows), nrows, k, _p(xt), _p(yo[t]))
    assert _same(y, yo), np.argwhere(y.view(np.uint32) != yo.view(np.uint32))[:4]
    y64, bound = K.dot_f64(qtype, n, k, row0, nrows, ntok)
    _note("dot type %d" % qtype, _ratio(yo, y64, bound))
    # the split of linear_ref.decode agrees with ggml_ref's dequantisers (f32 products of the same fields), so both readings of the blocks are one
    a, b = LR.decode(raw, qtype, n, k)
    deq = {8: ggml_ref.deq_q8_0, 13: ggml_ref.deq_q5_k, 14: ggml_ref.deq_q6_k}[qtype](np.asarray(raw), k)
    assert np.all(np.abs((a - b) - deq) <= 3 * 2.0 ** -24 * (np.abs(a) + np.abs(b)) + 1e-40)
    # gg_matvec alone on given arrays has no oracle entry; the restatement is held to float64 there
    y2 = K.dot_given(qtype, n, k, row0, nrows, ntok)[1]
    y64g, bg = K.dot_f64(qtype, n, k, row0, nrows, ntok, True)
    _note("dot type %d, given arrays (restatement)" % qtype, _ratio(y2, y64g, bg))
    assert not _same(y, y2)


@pytest.mark.parametrize("d,ntok", K.NORM_CASES)
def test_rmsnorm_equals_the_oracle_and_float64(L, d, ntok):
    x, g, kinds = K.norm_case(d, ntok)
    y = K.norm_ref(d, ntok)
    yo = np.zeros((ntok, d), F)
    for t in range(ntok):
        L.q3o_rmsnorm_ggml(_p(np.ascontiguousarray(x[t])), _p(np.ascontiguousarray(g)), d, C.c_float(K.NORM_EPS), _p(yo[t]))
    assert _same(y, yo), kinds
    over = R.squares_overflow(x)
    assert [bool(o) for o in over] == [kd in ("big", "spike") for kd in kinds]
    assert not yo[over].any()                                   # the overflow path: scale = 1 / inf = 0
    if ntok == 3:   # row 0 tells f32 squares from squares taken in double: by the mean's last bit, or by a square only f32 loses to inf
        wrong = R.rmsnorm(x[0], g, K.NORM_EPS, np.float64)
        assert kinds[0] in ("lowbit", "spike") and not np.array_equal(wrong, y[0]) and np.isfinite(wrong).all()
        assert kinds[0] == "lowbit" or wrong.any()
    for t, kd in enumerate(kinds):
        if kd == "zero":
            assert not yo[t].any()
        if kd == "subnormal":                                   # squares underflow: scale = 1 / sqrtf(eps)
            assert _same(yo[t], ((x[t] * (F(1) / np.sqrt(F(K.NORM_EPS)))).astype(F) * g).astype(F)) and yo[t].any()
    keep = ~over
    if keep.any():
        _note("rmsnorm", _ratio(yo[keep], R.rmsnorm64(x[keep], g, K.NORM_EPS), R.bound_rmsnorm(x[keep], g, K.NORM_EPS)))


@pytest.mark.parametrize("n", K.FLAT_NS)
def test_swiglu_oracle_within_float64(L, n):
    g, u = K.swiglu_case(n)
    yo = oracle_swiglu(L, g, u)
    assert np.isfinite(yo).all()
    _note("swiglu", _ratio(yo, R.swiglu64(g, u), R.bound_swiglu(g, u)))
    for gv, want in ((-104.0, 0.0), (104.0, 104.0)):            # expf saturates: silu(-104) = -0, silu(104) = 104 exactly
        hit = g == F(gv)
        assert np.array_equal(yo[hit], (F(want) * u[hit]).astype(F))


def test_load_rows_and_add_restatements():
    for d, form, stride in K.LOAD_CASES:
        x, rows, idx = K.load_case(d, form, stride)
        h = R.load_rows(x, rows, d)
        assert h.shape == (K.LOAD_NTOK, d) and all(np.array_equal(h[t], x[rows[t], :d]) for t in range(K.LOAD_NTOK))
        if form == "keys":
            assert [LR.key_code(v) for v in idx[::stride]] == list(rows)
    for n in K.ADD_NS:
        h, o = K.add_case(n)
        assert np.array_equal(R.add(h, o), h + o) and np.abs(R.add(h, o) - (h.astype(np.float64) + o)).max() <= 2.0 ** -24 * np.abs(h.astype(np.float64) + o).max()
