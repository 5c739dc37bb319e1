"""The six ggml-mode kernels that the attention tests do not reach -- k_gg_load_rows, k_gg_add, k_gg_rmsnorm, k_gg_quant, k_gg_matvec,
k_gg_swiglu (csrc/ggml_mode.hip) -- through q3tts_op_ggml: one launcher of ggml_mode.h per call on guarded buffers that come back whole.

Every run is checked three ways: the WHOLE buffer, bit for bit, against tests/ggml_mode_ref.py (numpy; SwiGLU's bits come from the oracle,
whose expf restates glibc's), so guards, stride padding and rows past ntok must still hold their poison; the float64 bounds of
ggml_mode_ref on dequantised operands; and refusals and no-ops write nothing.  The cases are tests/ggml_mode_cases.py, and
tests/test_ggml_mode_ref_cpu.py holds the restatement against oracle/q3o_ggml.c on the same cases without a GPU.

Then the model level: hidden rows and logits of the tiny talker and predictor with Q3_SPEC=ggml against oracle.Model in its ggml mode, bit
for bit, over a prefill that crosses a 64-position KV page in 16-token chunks and a logit row count that goes through the head's row clamp.

What is not claimed: llama.cpp itself is absent, so this pins the device to the project's restatement of ggml's generic kernels and to
float64, not to the binary."""
import ctypes as C
import os

import numpy as np
import pytest

import ggml_mode_cases as K
import ggml_mode_ref as R
import linear_ref as LR

pytestmark = pytest.mark.gpu
F = np.float32
NAN = F(np.nan)
POISON = {"q8": 0x5A, "d8": 0xBEEF, "qk": 0x5B, "dk": NAN, "bs": 0x7A7B}
DT = {"q8": np.int8, "d8": np.uint16, "qk": np.int8, "dk": F, "bs": np.int16}
PER = {"q8": 1, "d8": 32, "qk": 1, "dk": 256, "bs": 16}
NAMES = ("q8", "d8", "qk", "dk", "bs")


def _raw(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    g, w = _raw(got), _raw(want)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w) // got.dtype.itemsize
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r"
                             % (what, np.unique(bad).size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]]))


def _guard(gpu, rows, width, poison, dtype, fill=None):
    """a whole guarded buffer [rows][width] of poison, the first rows of it from fill [n][w <= width]"""
    core = np.full((rows, width), poison, dtype)
    if fill is not None:
        core[:fill.shape[0], :fill.shape[1]] = fill
    return gpu.glue_guarded(core, poison, dtype)


def _act_bufs(gpu, ntok, k, fill=None):
    """the five quantised arrays, one poisoned row past ntok; fill = (q8, d8, qk, dk, bs) to pre-load"""
    return {n: _guard(gpu, ntok + 1, k // PER[n], POISON[n], DT[n], None if fill is None else np.asarray(fill[i]).reshape(ntok, -1))
            for i, n in enumerate(NAMES)}


def _within(y, y64, bound, what):
    err = np.abs(np.asarray(y, np.float64) - y64)
    assert np.all(err <= bound), (what, float(err.max()), float((err / bound).max()))


# ---------------------------------------------------------------- k_gg_quant ---------------------------------------------------------------
@pytest.mark.parametrize("k,ntok", K.QUANT_CASES)
def test_quant(gpu, k, ntok):
    x, names = K.quant_case(k, ntok)
    ref = K.quant_ref(k, ntok)
    got = _act_bufs(gpu, ntok, k)
    gpu.op_ggml(gpu.GG_QUANT, ntok=ntok, k=k, x=x, **got)
    want = _act_bufs(gpu, ntok, k, ref)
    for n in NAMES:
        _same(got[n], want[n], "k_gg_quant %s k=%d ntok=%d %r" % (n, k, ntok, names))


# ---------------------------------------------------------------- k_gg_matvec --------------------------------------------------------------
def _out_want(gpu, y, ntok, nrows):
    return _guard(gpu, ntok + 1, nrows + 3, NAN, F, y)


@pytest.mark.parametrize("qtype,n,k,row0,nrows,ntok", K.DOT_CASES)
def test_linear_chain(gpu, qtype, n, k, row0, nrows, ntok):
    """gg_quant then gg_matvec on f32 activations, as Transformer::gg_linear: out_stride = nrows + 3 inside a NaN buffer"""
    raw, x = K.dot_case(qtype, n, k, row0, nrows, ntok)
    act, y = K.dot_ref(qtype, n, k, row0, nrows, ntok)
    got = _act_bufs(gpu, ntok, k)
    out = _guard(gpu, ntok + 1, nrows + 3, NAN, F)
    gpu.op_ggml(gpu.GG_LINEAR, ntok=ntok, k=k, x=x, w=raw, type=qtype, rows=n, row0=row0, nrows=nrows, out_stride=nrows + 3, out=out, **got)
    what = "type %d n=%d k=%d row0=%d nrows=%d ntok=%d" % (qtype, n, k, row0, nrows, ntok)
    _same(out, _out_want(gpu, y, ntok, nrows), "k_gg_matvec (chained) " + what)
    want = _act_bufs(gpu, ntok, k, act)
    for nm in NAMES:
        _same(got[nm], want[nm], "k_gg_quant (chained) %s %s" % (nm, what))
    y64, bound = K.dot_f64(qtype, n, k, row0, nrows, ntok)
    _within(gpu.glue_core(out, (ntok + 1, nrows + 3))[:ntok, :nrows], y64, bound, what)


@pytest.mark.parametrize("qtype,n,k,row0,nrows,ntok", K.DOT_CASES)
def test_matvec_on_given_arrays(gpu, qtype, n, k, row0, nrows, ntok):
    """gg_matvec alone: int8 values of -128, block sums that are not the sums of qk, a negated super-block scale -- all taken as given, none written"""
    raw, _ = K.dot_case(qtype, n, k, row0, nrows, ntok)
    act, y = K.dot_given(qtype, n, k, row0, nrows, ntok)
    bufs = _act_bufs(gpu, ntok, k, act)
    before = {nm: b.copy() for nm, b in bufs.items()}
    out = _guard(gpu, ntok + 1, nrows + 3, NAN, F)
    gpu.op_ggml(gpu.GG_MATVEC, ntok=ntok, k=k, w=raw, type=qtype, rows=n, row0=row0, nrows=nrows, out_stride=nrows + 3, out=out, **bufs)
    what = "type %d n=%d k=%d row0=%d nrows=%d ntok=%d" % (qtype, n, k, row0, nrows, ntok)
    _same(out, _out_want(gpu, y, ntok, nrows), "k_gg_matvec (given arrays) " + what)
    for nm in NAMES:
        _same(bufs[nm], before[nm], "activations after gg_matvec, %s %s" % (nm, what))
    y64, bound = K.dot_f64(qtype, n, k, row0, nrows, ntok, True)
    _within(gpu.glue_core(out, (ntok + 1, nrows + 3))[:ntok, :nrows], y64, bound, what)


def test_refusals_and_no_ops_write_nothing(gpu):
    qtype, n, k, row0, nrows, ntok = K.DOT_CASES[1]
    raw, x = K.dot_case(qtype, n, k, row0, nrows, ntok)
    act = K.dot_ref(qtype, n, k, row0, nrows, ntok)[0]

    def run(op, **over):
        bufs = _act_bufs(gpu, ntok, k, act)
        out = _guard(gpu, ntok + 1, nrows + 3, NAN, F)
        before = {nm: b.copy() for nm, b in bufs.items()}
        a = dict(ntok=ntok, k=k, x=x, w=raw, type=qtype, rows=n, row0=row0, nrows=nrows, out_stride=nrows + 3)
        a.update(over)
        if op == gpu.GG_MATVEC:
            a.pop("x")
        try:
            gpu.op_ggml(op, out=out, **a, **bufs)
            raised = None
        except gpu.Q3Error as ex:
            raised = str(ex)
        _same(out, _guard(gpu, ntok + 1, nrows + 3, NAN, F), "out after %r" % (over,))
        for nm in NAMES:
            _same(bufs[nm], before[nm], "%s after %r" % (nm, over))
        return raised

    for op in (gpu.GG_MATVEC, gpu.GG_LINEAR):
        # what gg_matvec refuses: the type, the row range
        assert "Q8_0 / Q5_K / Q6_K" in run(op, type=12)
        assert "Q8_0 / Q5_K / Q6_K" in run(op, type=0)
        assert "row range" in run(op, row0=n - nrows + 1)
        assert "row range" in run(op, row0=-1)
        assert "row range" in run(op, nrows=-1)
        assert "row range" in run(op, nrows=n + 1, row0=0, out_stride=n + 1)
        # no-ops
        assert run(op, nrows=0) is None
        assert run(op, ntok=0) is None
        assert run(op, row0=n, nrows=0) is None
        # the op's own: a buffer that cannot hold the shape
        assert "out_stride" in run(op, out_stride=nrows - 1)
        assert "too small" in run(op, out_stride=nrows + 40)
        assert "does not hold ntok rows" in run(op, ntok=ntok + 2)
    assert "k % 256" in run(gpu.GG_QUANT, k=k - 32)
    assert "does not hold [ntok][k]" in run(gpu.GG_QUANT, x=x[:, :-1])
    assert "unknown ggml-mode op" in run(7)
    # row loads: an index outside the table, both index forms at once
    xt, rows, idx = K.load_case(256, "int32", 1)
    for bad in (dict(idx=np.array([0, K.LOAD_ROWS, 1], np.int32)), dict(idx=np.array([0, -1, 1], np.int32)),
                dict(idx_keys=np.array([LR.pack_key(0.0, K.LOAD_ROWS)] * 3, np.uint64)),
                dict(idx=idx, idx_keys=np.zeros(3, np.uint64)), dict(idx=idx[:2]), dict(x_rows=K.LOAD_ROWS + 1)):
        out = _guard(gpu, 4, 256, NAN, F)
        a = dict(ntok=3, k=256, x=xt, x_stride=xt.shape[1], x_rows=K.LOAD_ROWS, idx_stride=1, idx=idx)
        if "idx_keys" in bad and "idx" not in bad:
            a.pop("idx")
        a.update(bad)
        with pytest.raises(gpu.Q3Error):
            gpu.op_ggml(gpu.GG_LOAD_ROWS, out=out, **a)
        _same(out, _guard(gpu, 4, 256, NAN, F), "out after %r" % (sorted(bad),))


# ---------------------------------------------------------------- k_gg_rmsnorm -------------------------------------------------------------
@pytest.mark.parametrize("d,ntok", K.NORM_CASES)
def test_rmsnorm(gpu, d, ntok):
    x, g, kinds = K.norm_case(d, ntok)
    y = K.norm_ref(d, ntok)
    out = _guard(gpu, ntok + 1, d, NAN, F)
    gpu.op_ggml(gpu.GG_RMSNORM, ntok=ntok, k=d, x=x, u=g, eps=K.NORM_EPS, out=out)
    _same(out, _guard(gpu, ntok + 1, d, NAN, F, y), "k_gg_rmsnorm d=%d %r" % (d, kinds))
    got = gpu.glue_core(out, (ntok + 1, d))[:ntok]
    over = R.squares_overflow(x)
    assert not got[over].any()      # f32 squares reach inf: scale 0, output 0, as ggml's
    if (~over).any():
        _within(got[~over], R.rmsnorm64(x[~over], g, K.NORM_EPS), R.bound_rmsnorm(x[~over], g, K.NORM_EPS), kinds)


# ---------------------------------------------------------------- k_gg_swiglu, k_gg_add, k_gg_load_rows ------------------------------------
@pytest.mark.parametrize("n", K.FLAT_NS)
def test_swiglu(gpu, oracle, n):
    g, u = K.swiglu_case(n)
    L = oracle.lib()
    L.q3o_swiglu_ggml.restype = C.c_float
    L.q3o_swiglu_ggml.argtypes = [C.c_float, C.c_float]
    y = np.array([L.q3o_swiglu_ggml(float(a), float(b)) for a, b in zip(g, u)], F)
    out = _guard(gpu, 1, n + 300, NAN, F)
    gpu.op_ggml(gpu.GG_SWIGLU, n=n, x=g, u=u, out=out)
    _same(out, _guard(gpu, 1, n + 300, NAN, F, y[None]), "k_gg_swiglu n=%d" % n)
    _within(gpu.glue_core(out)[:n], R.swiglu64(g, u), R.bound_swiglu(g, u), n)


@pytest.mark.parametrize("n", K.ADD_NS)
def test_add(gpu, n):
    h, o = K.add_case(n)
    out = _guard(gpu, 1, n + 300, NAN, F, h[None])
    gpu.op_ggml(gpu.GG_ADD, n=n, x=o, out=out)
    _same(out, _guard(gpu, 1, n + 300, NAN, F, R.add(h, o)[None]), "k_gg_add n=%d" % n)
    assert np.all(np.abs(gpu.glue_core(out)[:n] - (h.astype(np.float64) + o)) <= 2.0 ** -24 * np.abs(h.astype(np.float64) + o))   # one rounding


@pytest.mark.parametrize("d,form,stride", K.LOAD_CASES)
def test_load_rows(gpu, d, form, stride):
    x, rows, idx = K.load_case(d, form, stride)
    a = dict(ntok=K.LOAD_NTOK, k=d, x=x, x_stride=x.shape[1], x_rows=K.LOAD_ROWS, idx_stride=stride)
    if form == "int32":
        a["idx"] = idx
    elif form == "keys":
        assert [gpu.argmax_key(v, int(r)) for v, r in zip((-2.5, 0.0, 7e9), rows)] == [int(v) for v in idx[::stride]]   # the keys are the library's own
        a["idx_keys"] = idx
    out = _guard(gpu, K.LOAD_NTOK + 1, d, NAN, F)
    gpu.op_ggml(gpu.GG_LOAD_ROWS, out=out, **a)
    ref = R.load_rows(x, rows, d)
    _same(out, _guard(gpu, K.LOAD_NTOK + 1, d, NAN, F, ref), "k_gg_load_rows d=%d %s stride %d" % (d, form, stride))
    assert np.array_equal(gpu.glue_core(out, (K.LOAD_NTOK + 1, d))[:K.LOAD_NTOK].astype(np.float64), x.astype(np.float64)[rows, :d])   # a copy: exact in float64 too


# ---------------------------------------------------------------- the model level ----------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _model_parity(gpu, oracle, path, n_pre, n_dec, rows):
    """test_gpu_parity._tf_parity's comparison -- hidden rows and logits of every position against oracle.Model, bit for bit -- in the ggml mode
    on both sides: a chunked prefill (16 tokens per launch), single-token decode steps, and a restart after clear()"""
    old = os.environ.get("Q3_SPEC")
    om = gm = None
    try:
        os.environ["Q3_SPEC"] = "ggml"
        oracle.set_arith_mode(1)
        rng = np.random.default_rng(9)
        om = oracle.Model(path, 4096)
        gm = gpu.TfContext(path, 4096, 16)
        d = gm.n_embd
        xs = (rng.standard_normal((n_pre + n_dec, d)) * 0.3).astype(F)
        pos = np.array([[t, t, t, 0] for t in range(n_pre + n_dec)], np.int32)
        hg, lg = gm.eval(xs[:n_pre], pos[:n_pre], 0, rows)
        for t in range(n_pre):
            ho, lo = om.eval(xs[t], pos[t], d, 0, rows)
            assert np.array_equal(_bits(ho), _bits(hg[t])), ("hidden", t, int((_bits(ho) != _bits(hg[t])).sum()))
            assert np.array_equal(_bits(lo), _bits(lg[t])), ("logits", t, int((_bits(lo) != _bits(lg[t])).sum()))
        for t in range(n_pre, n_pre + n_dec):
            h1, l1 = gm.eval(xs[t:t + 1], pos[t:t + 1], 0, rows)
            ho, lo = om.eval(xs[t], pos[t], d, 0, rows)
            assert np.array_equal(_bits(ho), _bits(h1[0])) and np.array_equal(_bits(lo), _bits(l1[0])), ("decode", t)
        gm.clear(); om.clear()
        h2, _ = gm.eval(xs[:1], pos[:1], 0, 0)
        ho, _ = om.eval(xs[0], pos[0], d, 0, 0)
        assert np.array_equal(_bits(ho), _bits(h2[0]))
    finally:
        oracle.set_arith_mode(0)
        if old is None:
            os.environ.pop("Q3_SPEC", None)
        else:
            os.environ["Q3_SPEC"] = old
        if gm is not None:
            gm.close()
        if om is not None:
            om.close()


@pytest.mark.parametrize("sub", ["gguf_q8_0", "gguf_q5_k_m"])
def test_talker_hidden_and_logits_match_oracle_in_ggml_mode(gpu, oracle, tiny_model, sub):
    """70 prompt positions = five 16-token chunks, the last across the 64-position KV page; 3 decode steps; 2160 logit rows (no multiple of 64,
    and past the head's 32-row padding the row clamp nr = min(nrows, n - row0) decides)"""
    _model_parity(gpu, oracle, os.path.join(tiny_model, sub, "qwen3_tts_talker.gguf"), 70, 3, 2160)


@pytest.mark.parametrize("sub", ["gguf_q8_0", "gguf_q5_k_m"])
def test_predictor_hidden_and_logits_match_oracle_in_ggml_mode(gpu, oracle, tiny_model, sub):
    _model_parity(gpu, oracle, os.path.join(tiny_model, sub, "qwen3_tts_predictor.gguf"), 18, 3, 2048)
