"""Q5_0 weights on the device, held to their Q8_0 twin {d, int8 (u - 16)}: every linear form on a Q5_0 tensor equals, bit for bit, the same form
on the twin rows as type 8 in the K-quant layout (a path tests/test_gpu_kq_forms.py holds to the oracle) and lies within linear_ref.bound_gemm of
the float64 product; a tiny q3synth Q5_0 engine equals oracle.Engine and the device's Q8_0 engine on the twin file.  Random bytes put all 32
levels and both values of the fifth bit into every byte position, so a wrong plane bit index or polarity changes the bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linear_ref as R
import q3tts as Q
import synth_models
from test_gpu_linear import POISON, _bits, _poison
from test_gpu_q40 import CASES, ROOT, _inputs   # the Q4_0 cases and inputs: K, rows, tokens, the extreme case (here I_b = 32 * 16 * 127), window, fused
from test_q50_cpu import dec_q5_0, rand_rows, widen

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=lambda c: "k%d_n%s_t%d%s" % (c["k"], "+".join(map(str, c["rows"])), c["nt"], "_x" if c.get("extreme") else ""))
def test_linear_forms(gpu, oracle, case):
    k, nt, rows = case["k"], case["nt"], case["rows"]
    row0, nrows = case.get("row0", 0), case.get("nrows", sum(rows))
    rng = np.random.default_rng(k * 7 + nt)
    W = [(rand_rows(rng, n, k), 6, n) for n in rows]
    if case.get("extreme"):
        W[0][0].reshape(-1, 22)[:, 2:] = 0   # every u = 0: q = -16; d stays
    W8 = [(widen(raw), 8, n) for raw, _, n in W]
    a = np.concatenate([dec_q5_0(raw, n, k) for raw, _, n in W])[row0:row0 + nrows]
    xq, xd, f = _inputs(rng, oracle, k, nt, case.get("extreme"))
    x64 = R.dequant_act(xq[:nt], xd[:nt])
    ntiles, nss = (nt + 31) // 32, (k // 256 + 7) // 8
    forms = [(Q.LOP_GEMV, "AUTO", {})] + [(Q.LOP_GEMV, "GEMV_KQ", dict(lpr=l, mt=m)) for l in (2, 4, 8) for m in (1, 2, 4, 8)]
    forms += [(Q.LOP_GEMV, "GEMM_KQ_MFMA", dict(ztiles=z)) for z in sorted({1, min(3, ntiles), ntiles})]
    if f is not None:
        forms += [(Q.LOP_NORM_GEMV, "GEMV_NORM", dict(lpr=l, mt=m)) for l in (2, 4, 8) for m in (1, 2, 4, 8)]
    stride, off = nrows + 4, (3 if nt % 2 else 4)
    bound = R.bound_gemm(a, 0 * a, x64)
    for op, form, kw in forms:
        ns = nss if op == Q.LOP_GEMV else 1
        io = dict(xq=xq, xd=xd, a_rows=xq.shape[0]) if op == Q.LOP_GEMV else dict(eps=1e-6, **f)
        got = {}
        for name, w in (("q5_0", W), ("twin", W8)):
            out = _poison(off + ns * nt * stride + 7)
            hk = {} if op == Q.LOP_GEMV else dict(h_out=_poison(nt * k))
            ran = Q.op_linear(op, form, w, K=k, row0=row0, nrows=nrows, ntok=nt, out=out, out_off=off, out_stride=stride, kq_layout=1, **io, **hk, **kw)
            y = out[off:off + ns * nt * stride].reshape(ns, nt, stride)
            pad = np.concatenate([out[:off], out[off + ns * nt * stride:], y[:, :, nrows:].reshape(-1)])
            assert (_bits(pad) == POISON).all(), (form, kw, name, "stray write")
            assert form == "AUTO" or ran[0] == form, (form, ran)
            got[name] = y[:, :, :nrows].copy()
        assert np.array_equal(_bits(got["q5_0"]), _bits(got["twin"])), (form, kw)
        assert (np.abs(R.sum_slabs(got["q5_0"]).astype(np.float64) - x64 @ a.T) <= bound).all(), (form, kw)


@pytest.mark.parametrize("k,ff,nt", [(256, 32, 1), (512, 96, 3), (1024, 96, 16), (2048, 32, 33), (1024, 32, 97)])
def test_gateup_forms(gpu, oracle, k, ff, nt):
    """the fused gate/up forms against SwiGLU + quantisation (the oracle's, type-blind) of the GEMV output that test_linear_forms pins to the twin"""
    rng = np.random.default_rng(k + ff + nt)
    W = [(rand_rows(rng, ff, k), 6, ff) for _ in range(2)]
    xq, xd, f = _inputs(rng, oracle, k, nt)
    gu = np.zeros((nt, 2 * ff), np.float32)
    Q.op_linear(Q.LOP_GEMV, "GEMV_KQ", W, K=k, nrows=2 * ff, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], out=gu, out_stride=2 * ff, kq_layout=1, lpr=4)
    _, aq_w, ad_w = R.oracle_swiglu_quant(oracle.lib(), gu[:, :ff], gu[:, ff:])
    ntiles = (nt + 31) // 32
    forms = [(Q.LOP_GATEUP, "AUTO", {}), (Q.LOP_GATEUP, "GU_UNFUSED", {})] + [(Q.LOP_NORM_GATEUP, "GU_SWIGLU_NORM", dict(mt=m)) for m in (1, 2, 4)]
    if k in (1024, 2048):
        forms += [(Q.LOP_GATEUP, "GU_KQ_MFMA", dict(ztiles=z)) for z in sorted({ntiles, (ntiles + 3) // 4})]
    for op, form, kw in forms:
        aq = np.full((nt, ff), 55, np.int8); ad = np.full((nt, ff // 32), 0x7E00, np.uint16)
        io = dict(xq=xq, xd=xd, a_rows=xq.shape[0]) if op == Q.LOP_GATEUP else dict(eps=1e-6, h_out=_poison(nt * k), **f)
        ran = Q.op_linear(op, form, W, K=k, nrows=2 * ff, ff=ff, ntok=nt, aq=aq, ad=ad, kq_layout=1, **io, **kw)
        assert np.array_equal(aq, aq_w) and np.array_equal(ad, ad_w) and (form == "AUTO" or ran[0] == form), (form, kw, ran)


@pytest.fixture(scope="module")
def q50_model(tiny_model):
    return synth_models.ensure(tiny_model, [["--preset", "tiny", "--quant", "q5_0", "--what", "3"]], tag="q5_0")


@pytest.fixture(scope="module")
def twin_model(q50_model):
    """the same model with every Q5_0 tensor as Q8_0 blocks, in a directory of its own (its gguf_q8_0 is not the tiny model's)"""
    return synth_models.ensure(synth_models.model_dir("pytest_tiny_q5_0_twin"), [["--preset", "tiny", "--quant", "q5_0", "--q5_0-as-q8_0"]])


def test_engine_matches_oracle_on_twin(gpu, oracle, q50_model, twin_model, vivian):
    """graph / eager, 17 slots / single requests, greedy and sampled: the oracle on the twin, the device's Q8_0 engine on the twin, PCM"""
    rng = np.random.default_rng(17)
    ids = [rng.integers(0, 4000, 2 + i).astype(np.int32) for i in range(17)]
    kw = dict(max_steps=4, temperature=[0.0, 0.7] * 8 + [0.0], top_k=30, top_p=0.9, seed=list(range(5, 22)), mask_eos=True)
    eng = gpu.Engine(q50_model, "q5_0", max_batch=17, max_steps=8, load_codec=True)
    prompts = [eng.assets.build_core(t, lang_id=2055, spk_emb=vivian) for t in ids]
    wide = eng.generate_batch(prompts, **kw)
    st = eng.stats()
    assert st["slot_frames"] / max(st["graph_frames"], 1) >= 16, "the matrix-core widths were not exercised"
    pcm = eng.generate_batch(prompts[:2], **dict(kw, temperature=[0.0, 0.7], seed=[5, 6], want_pcm=True))
    eng.close()
    for i in (0, 1):
        assert np.array_equal(pcm[i]["codes"], wide[i]["codes"]) and np.isfinite(pcm[i]["pcm"]).all() and pcm[i]["pcm"].size == 4 * 1920, i
    oe = oracle.Engine(os.path.join(twin_model, "gguf_q8_0"), os.path.join(twin_model, "onnx", "q3tts_codec.gguf"), 4)
    for i in (0, 1, 8, 15, 16):
        oc = oe.generate(prompts[i], max_steps=4, temperature=kw["temperature"][i], top_k=30, top_p=0.9, seed=kw["seed"][i], mask_eos=True)[0]
        assert np.array_equal(oc, wide[i]["codes"]), ("oracle on the twin", i)
    oe.close()
    for model, quant, use_graph in ((q50_model, "q5_0", True), (q50_model, "q5_0", False), (twin_model, "q8_0", True)):
        eng = gpu.Engine(model, quant, max_batch=1, max_steps=8, load_codec=False, use_graph=use_graph)
        for i in (0, 1, 8, 15, 16):
            one = eng.generate_batch([prompts[i]], **dict(kw, temperature=kw["temperature"][i], seed=kw["seed"][i]))[0]
            assert np.array_equal(one["codes"], wide[i]["codes"]), (quant, use_graph, i)
        eng.close()


def test_tf_context_chunking(gpu, q50_model):
    """70 prompt tokens in one call per 64 + 6, 33 + 37 and 70 x 1: the same hidden rows (the MFMA forms against the GEMV forms)"""
    x = (np.random.default_rng(70).standard_normal((70, 2048)) * 0.5).astype(np.float32)
    pos = np.stack([np.arange(70)] * 3 + [np.zeros(70, np.int64)], axis=1).astype(np.int32)
    ctx = gpu.TfContext(os.path.join(q50_model, "gguf_q5_0", "qwen3_tts_talker.gguf"), n_ctx=128, max_tok=64)
    runs = []
    for cuts in ([0, 64, 70], [0, 33, 70], list(range(71))):
        ctx.clear()
        runs.append(np.concatenate([ctx.eval(x[a:b], pos[a:b])[0] for a, b in zip(cuts, cuts[1:])]))
    ctx.close()
    assert np.isfinite(runs[0]).all() and np.abs(runs[0]).max() > 0
    assert np.array_equal(_bits(runs[0]), _bits(runs[1])) and np.array_equal(_bits(runs[0]), _bits(runs[2]))


def test_ggml_mode_refuses_q5_0_at_load(gpu, q50_model):
    code = ("import sys; sys.path[:0] = %r\nimport q3tts as Q\ntry:\n    Q.Engine(%r, 'q5_0', max_batch=1, max_steps=8, load_codec=False)\n"
            "except Q.Q3Error as e:\n    print('LOADERR', e)\n" % ([os.path.join(ROOT, "tests"), os.path.join(ROOT, "qwen3-tts-rust_amd", "python")], q50_model))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, Q3_SPEC="ggml"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOADERR" in r.stdout and "Q5_0" in r.stdout, (r.returncode, r.stdout, r.stderr[-400:])
