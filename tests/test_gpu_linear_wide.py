"""The wide int8 GEMM forms for prompt chunks above 256 tokens (k_gemm_q8_wide: GEMM_Q8_WIDE, GU_Q8_WIDE), forced through q3tts_op_linear at the
smallest shapes at which they can go wrong, bit for bit against the same call forced to GEMM_Q8_MFMA / GU_Q8_MFMA and against the oracle
composition of tests/test_gpu_linear.py (whose helpers this file reuses).  A wave carries one token tile, so there is no per-wave tile grouping
to leave partial; the token counts leave partial tiles (33, 130, 257) and cross the dispatch threshold (257, 512); the row counts leave a workgroup
with missing row groups (160 rows, ff 160: 5 groups over workgroups of 4), a partial group (33 rows of a matrix padded to 64) and start at row0 = 32; K covers one segment, part of a
super-segment, a whole one and three output slabs, each slab compared on its own.  Plain outputs lie in a NaN-poisoned buffer with an offset
and a stride above nrows; the op itself guards the gate/up outputs on the device and refuses a form that writes outside [ntok][ff].

The forms store single floats, so there is no output alignment for them to refuse: every out / out_stride the op accepts runs (the odd token
counts below use an offset of 3 floats).  What they do refuse -- K-quant weights, a K the fused gate/up does not serve, a ztiles other than the
token tiles, the wrong op -- leaves the outputs untouched.

One engine-level case: prompts whose rows sum past 256 travel as one wide chunk, and codes equal those of the same engine with
Q3_PREFILL_WIDE=0 (256-token chunks on the old forms); PCM agrees within what two runs of the switched-off engine differ by."""
import os

import numpy as np
import pytest

import linear_ref as R
import q3tts as Q
import test_gpu_linear as T

pytestmark = pytest.mark.gpu

WIDE_CASES = [  # (rows of the matrix, K, ntok, row0, nrows)
    (32, 256, 33, 0, 32), (32, 768, 96, 0, 32), (32, 1024, 33, 0, 32), (96, 2048, 96, 32, 64), (160, 1024, 130, 0, 160), (33, 2048, 257, 0, 33),
    (64, 6144, 96, 0, 64), (96, 6144, 257, 0, 96), (32, 1024, 512, 0, 32),
]


@pytest.mark.parametrize("case", WIDE_CASES, ids=lambda c: "k%d_n%d_t%d_r%d" % (c[1], c[4], c[2], c[3]))
def test_wide_gemm(gpu, oracle, case):
    rows, k, nt, row0, nrows = case
    rng = np.random.default_rng(k * 11 + nt + nrows)
    W = T._weights(rng, [8], [rows], k)
    xq, xd = T._acts(rng, nt, k)
    nss = (k // 256 + 7) // 8
    stride, off = (nrows + 4 if nrows % 4 == 0 else nrows + 5), (3 if nt % 2 else 4)
    want = R.oracle_slabs(oracle.lib(), W, k, row0, nrows, xq[:nt], xd[:nt])          # [slab][token][row]: every slab on its own
    ntiles = (nt + 31) // 32

    def run(form, **kw):
        out = T._poison(off + nss * nt * stride + 7)
        ran = Q.op_linear(Q.LOP_GEMV, form, W, K=k, row0=row0, nrows=nrows, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], out=out, out_off=off,
                          out_stride=stride, **kw)
        got = out[off:off + nss * nt * stride].reshape(nss, nt, stride)
        pad = np.concatenate([out[:off], out[off + nss * nt * stride:], got[:, :, nrows:].reshape(-1)])
        assert (T._bits(pad) == T.POISON).all(), (form, kw, "stray write")
        return T._bits(got[:, :, :nrows]).copy(), ran

    old, _ = run("GEMM_Q8_MFMA", ztiles=1)
    assert np.array_equal(old, T._bits(want))
    got, ran = run("GEMM_Q8_WIDE")
    assert (ran[0], ran[3]) == ("GEMM_Q8_WIDE", ntiles), ran
    for s in range(nss):
        assert np.array_equal(got[s], T._bits(want[s])), "slab %d differs from the oracle" % s
    assert np.array_equal(got, old), "differs from GEMM_Q8_MFMA"
    got, ran = run("AUTO")
    assert (ran[0] == "GEMM_Q8_WIDE") == (nt > 256), ran                            # the dispatch: above 256 tokens only
    assert np.array_equal(got, old), "AUTO"


GU_WIDE_CASES = [(1024, 64, 33), (2048, 96, 96), (1024, 96, 130), (2048, 64, 257), (2048, 160, 96), (1024, 64, 96), (1024, 32, 512)]   # (K, ff, ntok)


@pytest.mark.parametrize("case", GU_WIDE_CASES, ids=lambda c: "k%d_ff%d_t%d" % c)
def test_wide_gateup(gpu, oracle, case):
    k, ff, nt = case
    rng = np.random.default_rng(k + 3 * ff + nt)
    W = T._gu_weights(rng, 8, ff, k)
    xq, xd = T._acts(rng, nt, k)
    gu = R.sum_slabs(R.oracle_slabs(oracle.lib(), W, k, 0, 2 * ff, xq[:nt], xd[:nt]))
    _, aq_w, ad_w = R.oracle_swiglu_quant(oracle.lib(), gu[:, :ff], gu[:, ff:])
    ntiles = (nt + 31) // 32

    def run(form, **kw):
        aq = np.full((nt, ff), 55, np.int8); ad = np.full((nt, ff // 32), 0x7E00, np.uint16)
        ran = Q.op_linear(Q.LOP_GATEUP, form, W, K=k, nrows=2 * ff, ff=ff, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], aq=aq, ad=ad, **kw)
        return aq, ad, ran

    aq_o, ad_o, _ = run("GU_Q8_MFMA", ztiles=ntiles)
    assert aq_o.tobytes() == aq_w.tobytes() and ad_o.tobytes() == ad_w.tobytes()
    aq, ad, ran = run("GU_Q8_WIDE")
    assert (ran[0], ran[3]) == ("GU_Q8_WIDE", ntiles), ran
    assert aq.tobytes() == aq_w.tobytes() and ad.tobytes() == ad_w.tobytes(), "differs from the oracle"
    assert aq.tobytes() == aq_o.tobytes() and ad.tobytes() == ad_o.tobytes(), "differs from GU_Q8_MFMA"
    aq, ad, ran = run("AUTO")
    assert (ran[0] == "GU_Q8_WIDE") == (nt > 256), ran
    assert aq.tobytes() == aq_w.tobytes() and ad.tobytes() == ad_w.tobytes(), "AUTO"


def test_wide_refusals_leave_outputs_untouched(gpu):
    rng = np.random.default_rng(6)
    xq, xd = T._acts(rng, 40, 2048)
    out = T._poison(2 * 40 * 40)
    q8 = [(R.rand_rows(rng, 8, 36, 2048), 8, 36)]
    kq = [(R.rand_rows(rng, 13, 32, 2048), 13, 32), (R.rand_rows(rng, 14, 32, 2048), 14, 32)]
    bad = [(Q.LOP_GEMV, "GEMM_Q8_WIDE", kq, dict(nrows=64, kq_layout=1)),        # K-quant weights
           (Q.LOP_GEMV, "GEMM_Q8_WIDE", q8, dict(nrows=36, kq_layout=1)),        # Q8_0 tensors in the K-quant layout
           (Q.LOP_GEMV, "GEMM_Q8_WIDE", q8, dict(nrows=36, ztiles=1)),           # 40 tokens = 2 tiles
           (Q.LOP_GEMV, "GEMM_Q8_WIDE", q8, dict(nrows=36, ztiles=3)),
           (Q.LOP_GEMV, "GEMM_Q8_WIDE", q8, dict(nrows=37)),                     # rows past the matrix
           (Q.LOP_GEMV, "GU_Q8_WIDE", q8, dict(nrows=36))]                       # wrong op for the form
    for op, form, W, kw in bad:
        with pytest.raises(RuntimeError):
            Q.op_linear(op, form, W, K=2048, ntok=40, xq=xq, xd=xd, a_rows=xq.shape[0], out=out, out_stride=40, **kw)
        assert (T._bits(out) == T.POISON).all(), (form, kw)
    aq, ad = np.full((40, 32), 55, np.int8), np.full((40, 1), 77, np.uint16)
    gu = dict(nrows=64, ff=32, ntok=40, a_rows=42, aq=aq, ad=ad)
    for K, W, kw in [(512, None, {}),                                            # fused gate/up serves K 1024 and 2048
                     (3072, None, {}),
                     (1024, None, dict(ztiles=1)),
                     (1024, [(R.rand_rows(rng, 13, 32, 1024), 13, 32), (R.rand_rows(rng, 13, 32, 1024), 13, 32)], dict(kq_layout=1))]:   # K-quant weights
        W = W or [(R.rand_rows(rng, 8, 64, K), 8, 64)]
        with pytest.raises(RuntimeError):
            Q.op_linear(Q.LOP_GATEUP, "GU_Q8_WIDE", W, K=K, xq=np.zeros((42, K), np.int8), xd=np.zeros((42, K // 32), np.uint16), **gu, **kw)
        assert (aq == 55).all() and (ad == 77).all(), (K, kw)


def _rms(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


def test_engine_wide_chunk_equals_narrow_chunks(gpu, tiny_model, vivian):
    """4 prompts of 90 .. 120 rows (406 in all) are one wave: one 406-row chunk on the wide forms, or 256 + 150 rows on the old ones"""
    def run(wide):
        old = os.environ.get("Q3_PREFILL_WIDE")
        os.environ["Q3_PREFILL_WIDE"] = "1" if wide else "0"
        try:
            ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=12, load_codec=True)
            assert ge.prefill_width() == (512 if wide else 256)
            prompts = [ge.assets.build_core(np.random.default_rng(40 + i).integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)
                       for i, n in enumerate((80, 90, 100, 110))]
            assert sum(p.shape[0] for p in prompts) > 256 and all(p.shape[0] < 256 for p in prompts)
            res = ge.generate_batch(prompts, max_steps=8, temperature=0.0, seed=42, mask_eos=True, want_pcm=True)
            ge.close()
            return res
        finally:
            if old is None:
                del os.environ["Q3_PREFILL_WIDE"]
            else:
                os.environ["Q3_PREFILL_WIDE"] = old

    narrow, narrow2, wide = run(False), run(False), run(True)
    for a, b, c in zip(narrow, narrow2, wide):
        assert a["codes"].shape == (8, 16)
        assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(a["codes"], c["codes"])
        assert a["pcm"].shape == c["pcm"].shape
        noise = _rms(a["pcm"], b["pcm"])
        print("pcm rms: narrow vs narrow %.3g, narrow vs wide %.3g" % (noise, _rms(a["pcm"], c["pcm"])))
        assert _rms(a["pcm"], c["pcm"]) <= noise
