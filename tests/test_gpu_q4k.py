"""Q4_K weights on the device.  Op level: every linear form that takes a K-quant tensor, bit for bit against the CPU oracle on the Q5_K twin of
the same rows (q4k_ref.widen: zero high-bit plane, spec S3) and against float64 within linear_ref.bound_gemm.  Engine level: a tiny Q4_K_M
model against its Q5_K twin files on the device and in the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import linear_ref as R
import q3tts as Q
import synth_models
from kq_ref import decode as _decode, weights as _weights
from test_gpu_linear import POISON, _acts, _bits, _norm_inputs, _poison

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GEMV_CASES = [([12], [32], 256, 1, 0, 32), ([12], [64], 2048, 3, 32, 32), ([12], [64], 2304, 9, 0, 64), ([12], [64], 1024, 17, 0, 64),
              ([12], [32], 512, 33, 0, 32), ([12, 14], [32, 32], 1024, 40, 0, 64), ([12, 14, 8], [32, 32, 32], 256, 2, 0, 96),
              ([12, 13, 12], [32, 32, 32], 256, 17, 0, 96)]
GEMV_FORMS = [("AUTO", {}), ("GEMV_KQ", dict(lpr=2, mt=1)), ("GEMV_KQ", dict(lpr=4, mt=8)), ("GEMV_KQ", dict(lpr=8, mt=2)), ("GEMM_KQ_MFMA", dict(ztiles=1))]


@pytest.mark.parametrize("case", GEMV_CASES, ids=lambda c: "k%d_n%d_t%d_%s" % (c[2], c[5], c[3], "-".join(map(str, c[0]))))
def test_gemv_forms(gpu, oracle, case):
    types, rows, k, nt, row0, nrows = case
    rng = np.random.default_rng(k * 7 + nt)
    W, W5 = _weights(rng, types, rows, k)
    xq, xd = _acts(rng, nt, k)
    nss = (k // 256 + 7) // 8
    stride, off = nrows + 4, (3 if nt % 2 else 4)
    want = R.oracle_slabs(oracle.lib(), W5, k, row0, nrows, xq[:nt], xd[:nt])
    a, b = _decode(W, k)
    a, b = a[row0:row0 + nrows], b[row0:row0 + nrows]
    x64 = R.dequant_act(xq[:nt], xd[:nt])
    for form, kw in GEMV_FORMS:
        out = _poison(off + nss * nt * stride + 7)
        ran = Q.op_linear(Q.LOP_GEMV, form, W, K=k, row0=row0, nrows=nrows, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], out=out, out_off=off,
                          out_stride=stride, kq_layout=1, **kw)
        got = out[off:off + nss * nt * stride].reshape(nss, nt, stride)
        assert np.array_equal(_bits(got[:, :, :nrows]), _bits(want)), (form, kw, ran)
        pad = np.concatenate([out[:off], out[off + nss * nt * stride:], got[:, :, nrows:].reshape(-1)])
        assert (_bits(pad) == POISON).all(), (form, "stray write")
        assert form == "AUTO" or ran[0] == form
        y = R.sum_slabs(got[:, :, :nrows]).astype(np.float64)
        assert (np.abs(y - x64 @ (a - b).T) <= R.bound_gemm(a, b, x64)).all(), form


@pytest.mark.parametrize("k,ff,nt", [(1024, 64, 40), (2048, 32, 17)])
def test_gateup_forms(gpu, oracle, k, ff, nt):
    rng = np.random.default_rng(k + ff + nt)
    W, W5 = _weights(rng, [12, 12], [ff, ff], k)
    xq, xd = _acts(rng, nt, k)
    gu = R.sum_slabs(R.oracle_slabs(oracle.lib(), W5, k, 0, 2 * ff, xq[:nt], xd[:nt]))
    _, aq_w, ad_w = R.oracle_swiglu_quant(oracle.lib(), gu[:, :ff], gu[:, ff:])
    ntiles = (nt + 31) // 32
    for form, kw in [("AUTO", {}), ("GU_UNFUSED", {}), ("GU_KQ_MFMA", dict(ztiles=ntiles)), ("GU_KQ_MFMA", dict(ztiles=(ntiles + 3) // 4))]:
        aq = np.full((nt, ff), 55, np.int8); ad = np.full((nt, ff // 32), 0x7E00, np.uint16)
        ran = Q.op_linear(Q.LOP_GATEUP, form, W, K=k, nrows=2 * ff, ff=ff, ntok=nt, xq=xq, xd=xd, a_rows=xq.shape[0], aq=aq, ad=ad, kq_layout=1, **kw)
        assert np.array_equal(aq, aq_w) and np.array_equal(ad, ad_w), (form, kw, ran)


@pytest.mark.parametrize("nt", [1, 4])
@pytest.mark.parametrize("op", ["NORM_GEMV", "NORM_ARGMAX", "NORM_GATEUP"])
def test_fused_decode_ops(gpu, oracle, op, nt):
    d, rows = 1024, 64
    rng = np.random.default_rng(d + rows + nt)
    W, W5 = _weights(rng, [12, 12] if op == "NORM_GATEUP" else [12], [rows // 2] * 2 if op == "NORM_GATEUP" else [rows], d)
    f, h, g = _norm_inputs(rng, d, nt, 1, keys=nt > 2)
    xn_w, xq_w, xd_w = R.oracle_norm(oracle.lib(), h, g, 1e-6)
    want = R.oracle_slabs(oracle.lib(), W5, d, 0, rows, xq_w, xd_w)[0]
    hout = _poison(nt * d)
    if op == "NORM_GEMV":
        out = _poison(5 + nt * (rows + 3))
        Q.op_linear(Q.LOP_NORM_GEMV, "AUTO", W, K=d, nrows=rows, ntok=nt, eps=1e-6, out=out, out_off=5, out_stride=rows + 3, h_out=hout, kq_layout=1, **f)
        got = out[5:].reshape(nt, rows + 3)
        assert np.array_equal(_bits(got[:, :rows]), _bits(want)) and (_bits(got[:, rows:]) == POISON).all() and (_bits(out[:5]) == POISON).all()
    elif op == "NORM_ARGMAX":
        armed = R.pack_key(-np.inf, 0)
        keys = np.full(2 * nt, armed, np.uint64)
        Q.op_linear(Q.LOP_NORM_ARGMAX, "AUTO", W, K=d, nrows=rows, nrows_valid=rows - 3, ntok=nt, eps=1e-6, keys=keys, key_stride=2, idx_add=7, h_out=hout,
                    kq_layout=1, **f)
        assert [int(x) for x in keys[::2]] == [R.greedy_key(want[t, :rows - 3], -1, 7, armed) for t in range(nt)] and (keys[1::2] == armed).all()
    else:
        ff = rows // 2
        _, aq_w, ad_w = R.oracle_swiglu_quant(oracle.lib(), want[:, :ff], want[:, ff:])
        aq = np.full((nt, ff), 55, np.int8); ad = np.zeros((nt, ff // 32), np.uint16)
        Q.op_linear(Q.LOP_NORM_GATEUP, "AUTO", W, K=d, nrows=rows, ff=ff, ntok=nt, eps=1e-6, aq=aq, ad=ad, h_out=hout, kq_layout=1, **f)
        assert np.array_equal(aq, aq_w) and np.array_equal(ad, ad_w)
    assert np.array_equal(_bits(hout.reshape(nt, d)), _bits(h))


@pytest.fixture(scope="module")
def q4k_models(tiny_model):
    """(the tiny model directory with gguf_q4_k_m added, a second directory that holds the same weights as Q5_K blocks in gguf_q5_k_m)"""
    synth_models.ensure(tiny_model, [["--preset", "tiny", "--quant", "q4_k_m", "--what", "3"]], tag="q4_k_m")
    twin = synth_models.ensure(synth_models.model_dir("pytest_tiny_q4k_twin"), [["--preset", "tiny", "--quant", "q4_k_m", "--what", "7", "--q4k-as-q5k"]])
    return tiny_model, twin


def _requests(eng, vivian):
    rng = np.random.default_rng(12)
    return [eng.assets.build_core(np.arange(100, 109, dtype=np.int32), lang_id=2055, spk_emb=vivian),
            eng.assets.build_clone(rng.integers(0, 4000, 5).astype(np.int32), rng.integers(0, 2048, 3 * 16), rng.integers(0, 4000, 2), vivian)]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_engine_matches_twin_and_oracle(gpu, oracle, q4k_models, vivian, use_graph):
    model, twin = q4k_models
    kw = dict(max_steps=6, temperature=[0.0, 0.7], top_k=30, top_p=0.9, seed=[5, 6], mask_eos=True, want_pcm=True)
    runs = []
    for mdir, quant in ((model, "q4_k_m"), (twin, "q5_k_m")):
        eng = gpu.Engine(mdir, quant, max_batch=2, max_steps=16, load_codec=True, use_graph=use_graph)
        prompts = _requests(eng, vivian)
        runs.append(eng.generate_batch(prompts, **kw))
        eng.close()
    oe = oracle.Engine(os.path.join(twin, "gguf_q5_k_m"), None, 4)
    for i, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a["codes"], b["codes"]) and np.array_equal(_bits(a["pcm"]), _bits(b["pcm"])), i
        oc, _ = oe.generate(prompts[i], max_steps=6, temperature=kw["temperature"][i], top_k=30, top_p=0.9, seed=kw["seed"][i], mask_eos=True)
        assert np.array_equal(oc, a["codes"]), i
    oe.close()


def test_engine_batch_of_17_matches_twin(gpu, q4k_models, vivian):
    rng = np.random.default_rng(17)
    ids = [rng.integers(0, 4000, 2 + i).astype(np.int32) for i in range(17)]
    runs = []
    for mdir, quant in zip(q4k_models, ("q4_k_m", "q5_k_m")):
        eng = gpu.Engine(mdir, quant, max_batch=17, max_steps=8, load_codec=False)
        runs.append(eng.generate_batch([eng.assets.build_core(t, lang_id=2055, spk_emb=vivian) for t in ids], max_steps=4, mask_eos=True))
        st = eng.stats()
        assert st["slot_frames"] / max(st["graph_frames"], 1) >= 16, "the matrix-core widths were not exercised"
        eng.close()
    for i, (a, b) in enumerate(zip(*runs)):
        assert np.array_equal(a["codes"], b["codes"]), i


def test_ggml_mode_refuses_q4k_at_load(gpu, q4k_models):
    code = ("import sys; sys.path[:0] = %r\nimport q3tts as Q\ntry:\n    Q.Engine(%r, 'q4_k_m', max_batch=1, max_steps=8, load_codec=False)\n"
            "except Q.Q3Error as e:\n    print('LOADERR', e)\n" % ([os.path.join(ROOT, "tests"), os.path.join(ROOT, "qwen3-tts-rust_amd", "python")], q4k_models[0]))
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, Q3_SPEC="ggml"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "LOADERR" in r.stdout and "Q4_K" in r.stdout, (r.returncode, r.stdout, r.stderr[-400:])
