"""Every K-quant linear form at each weight type, lane split and tile walk of tests/kq_form_cases.py (q3tts_op_linear): k_gemv_kq<LPR, MT, TS>,
k_gemv_q8_norm<LPR, MT, EPI, TS>, k_gateup_swiglu<MT, NS, TS> and k_gemm_kq_mfma<GU, TS> are compiled once per TS and choose a body per weight
type inside, so an instantiation that no test launches can differ from those that are launched.  One test per shape of the table: weights and
references are built once, every forced form of the shape and AUTO run on them.  The assertions are those of test_gpu_linear.py /
test_gpu_q3k.py / test_gpu_q4k.py: bit for bit against the CPU oracle on the twin rows (Q3_K as Q6_K, Q4_K as Q5_K), poison in every byte the
launch must not write, h_out / xn_out bit-equal to the oracle's, the form that ran, and float64 within the derived bounds of linear_ref.py.
Each test prints the worst error / bound it saw (-s shows them); RAN records what AUTO chose."""
import numpy as np
import pytest

import kq_form_cases as C
import kq_ref as KR
import linear_ref as R
import q3tts as Q
from test_gpu_linear import POISON, _bits, _poison

pytestmark = pytest.mark.gpu
RAN = {}     # (form, shape) -> what AUTO ran for it: (form, lpr, mt, z)
WORST = {}   # form -> worst err / bound so far


def _param(form):
    return pytest.mark.parametrize("shape,cases", C.shapes(form), ids=[C.shape_id(s) for s, _ in C.shapes(form)])


def _forms(form, shape, cases):
    return [("AUTO", {}, None)] + [(form, C.launch(c), c) for c in cases if not c.params.get("refuse")]


def _note(form, shape, ran, worst=None):
    if ran is not None:
        RAN[(form, shape)] = ran
    if worst is not None:
        WORST[form] = max(WORST.get(form, 0.0), worst)
    print("%s %s: AUTO ran %s, worst err / bound %s (family so far %s)" % (form, C.shape_id(shape), RAN.get((form, shape)),
                                                                          "-" if worst is None else "%.3g" % worst, "%.3g" % WORST.get(form, 0.0)))


def _run_gemv(form, shape, cases, oracle):
    s, r = shape, KR.reference(oracle.lib(), shape)
    nss = (s.K // 256 + 7) // 8
    stride, off = s.nrows + 4, (3 if s.nt % 2 else 4)
    worst, auto = r.ratio, None
    assert worst <= 1.0
    for f, kw, case in _forms(form, shape, cases):
        out = _poison(off + nss * s.nt * stride + 7)
        ran = Q.op_linear(Q.LOP_GEMV, f, r.W, K=s.K, row0=s.row0, nrows=s.nrows, ntok=s.nt, xq=r.xq, xd=r.xd, a_rows=r.xq.shape[0], out=out, out_off=off,
                          out_stride=stride, kq_layout=1, **kw)
        got = out[off:off + nss * s.nt * stride].reshape(nss, s.nt, stride)
        assert np.array_equal(_bits(got[:, :, :s.nrows]), _bits(r.want)), (f, kw, ran)
        pad = np.concatenate([out[:off], out[off + nss * s.nt * stride:], got[:, :, s.nrows:].reshape(-1)])
        assert (_bits(pad) == POISON).all(), (f, kw, "stray write")
        if f == "AUTO":
            auto = ran
        else:
            assert ran[0] == f and all(ran[1 + ("lpr", "mt", "ztiles").index(k)] == v for k, v in kw.items()), (f, kw, ran)
        err = np.abs(R.sum_slabs(got[:, :, :s.nrows]).astype(np.float64) - r.y64)
        worst = max(worst, KR.ratio(err, r.bound))
        assert (err <= r.bound).all(), (f, kw)
    _note(form, shape, auto, worst)


@_param("GEMV_KQ")
def test_gemv_kq(gpu, oracle, shape, cases):
    _run_gemv("GEMV_KQ", shape, cases, oracle)


@_param("GEMM_KQ_MFMA")
def test_gemm_kq_mfma(gpu, oracle, shape, cases):
    _run_gemv("GEMM_KQ_MFMA", shape, cases, oracle)


@_param("GU_KQ_MFMA")
def test_gu_kq_mfma(gpu, oracle, shape, cases):
    s, r = shape, KR.reference(oracle.lib(), shape)
    ff = s.nrows // 2
    worst, auto = r.ratio, None
    assert worst <= 1.0
    call = lambda f, aq, ad, kw: Q.op_linear(Q.LOP_GATEUP, f, r.W, K=s.K, nrows=2 * ff, ff=ff, ntok=s.nt, xq=r.xq, xd=r.xd, a_rows=r.xq.shape[0], aq=aq,
                                             ad=ad, kq_layout=1, **kw)
    for f, kw, case in _forms("GU_KQ_MFMA", shape, cases):
        aq = np.full((s.nt, ff), 55, np.int8); ad = np.full((s.nt, ff // 32), 0x7E00, np.uint16)
        ran = call(f, aq, ad, kw)
        assert np.array_equal(aq, r.aq) and np.array_equal(ad, r.ad), (f, kw, ran)
        if f == "AUTO":
            auto = ran
        else:
            assert ran[0] == f and ran[3] == kw["ztiles"], (f, kw, ran)
        worst = max(worst, KR.swiglu_ratio(r, aq, ad))
    for case in cases:
        if case.params.get("refuse"):   # more gate tiles than a workgroup parks: refused on the host, the outputs as they were
            aq = np.full((s.nt, ff), 55, np.int8); ad = np.full((s.nt, ff // 32), 0x7E00, np.uint16)
            with pytest.raises(Q.Q3Error):
                call("GU_KQ_MFMA", aq, ad, C.launch(case))
            assert (aq == 55).all() and (ad == 0x7E00).all()
    _note("GU_KQ_MFMA", shape, auto, worst)


@_param("GEMV_NORM")
def test_gemv_norm(gpu, oracle, shape, cases):
    s, r = shape, KR.reference(oracle.lib(), shape)
    stride = s.nrows + 3
    worst, auto = r.ratio, None
    assert worst <= 1.0
    for f, kw, case in _forms("GEMV_NORM", shape, cases):
        out = _poison(5 + s.nt * stride)
        hout = _poison(s.nt * s.K); xn = _poison(s.nt * s.K)
        ran = Q.op_linear(Q.LOP_NORM_GEMV, f, r.W, K=s.K, row0=s.row0, nrows=s.nrows, ntok=s.nt, eps=1e-6, out=out, out_off=5, out_stride=stride,
                          h_out=hout, xn_out=xn, kq_layout=1, **kw, **r.f)
        got = out[5:].reshape(s.nt, stride)
        assert np.array_equal(_bits(got[:, :s.nrows]), _bits(r.want)), (f, kw, ran)
        assert (_bits(got[:, s.nrows:]) == POISON).all() and (_bits(out[:5]) == POISON).all(), (f, kw, "stray write")
        assert np.array_equal(_bits(hout.reshape(s.nt, s.K)), _bits(r.h)) and np.array_equal(_bits(xn.reshape(s.nt, s.K)), _bits(r.xn)), (f, kw)
        if f == "AUTO":
            auto = ran
        else:
            assert ran[:3] == (f, kw["lpr"], kw["mt"]), (f, kw, ran)
        err = np.abs(got[:, :s.nrows].astype(np.float64) - r.y64)
        worst = max(worst, KR.ratio(err, r.bound))
        assert (err <= r.bound).all(), (f, kw)
    _note("GEMV_NORM", shape, auto, worst)


@_param("GEMV_NORM_ARGMAX")
def test_gemv_norm_argmax(gpu, oracle, shape, cases):
    s, r = shape, KR.reference(oracle.lib(), shape)
    st = dict(s.setup)
    auto = None
    for f, kw, case in _forms("GEMV_NORM_ARGMAX", shape, cases):
        keys = np.full(2 * s.nt, r.armed, np.uint64)
        hout = _poison(s.nt * s.K)
        ran = Q.op_linear(Q.LOP_NORM_ARGMAX, f, r.W, K=s.K, nrows=s.nrows, nrows_valid=st["nrows_valid"], ntok=s.nt, eps=1e-6, keys=keys, key_stride=2,
                          idx_add=st["idx_add"], mask_per_tok=r.mask, h_out=hout, kq_layout=1, **kw, **r.f)
        assert [int(x) for x in keys[::2]] == r.keys, (f, kw, [R.key_code(int(x)) - st["idx_add"] for x in keys[::2]], r.pairs)
        assert (keys[1::2] == r.armed).all(), (f, kw, "stray key")
        assert np.array_equal(_bits(hout.reshape(s.nt, s.K)), _bits(r.h)), (f, kw)
        if f == "AUTO":
            auto = ran
        else:
            assert ran[:3] == (f, 2, kw["mt"]), (f, kw, ran)
    _note("GEMV_NORM_ARGMAX", shape, auto)


@_param("GU_SWIGLU_NORM")
def test_gu_swiglu_norm(gpu, oracle, shape, cases):
    s, r = shape, KR.reference(oracle.lib(), shape)
    ff = s.nrows // 2
    auto = None
    for f, kw, case in _forms("GU_SWIGLU_NORM", shape, cases):
        aq = np.full((s.nt, ff), 55, np.int8); ad = np.zeros((s.nt, ff // 32), np.uint16); hout = _poison(s.nt * s.K)
        ran = Q.op_linear(Q.LOP_NORM_GATEUP, f, r.W, K=s.K, nrows=2 * ff, ff=ff, ntok=s.nt, eps=1e-6, aq=aq, ad=ad, h_out=hout, kq_layout=1, **kw, **r.f)
        assert np.array_equal(aq, r.aq) and np.array_equal(ad, r.ad), (f, kw, ran)
        assert np.array_equal(_bits(hout.reshape(s.nt, s.K)), _bits(r.h)), (f, kw)
        if f == "AUTO":
            auto = ran
        else:
            assert ran[0] == f and ran[2] == kw["mt"], (f, kw, ran)
    _note("GU_SWIGLU_NORM", shape, auto, r.ratio)
