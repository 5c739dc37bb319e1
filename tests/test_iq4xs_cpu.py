"""IQ4_XS on the host: the float64 decode of spec S3 (written out here, shared with tests/test_gpu_iq4xs.py), the packed layout plan and the
refusals of the older type sets, q3synth's encoder, that bound (a) sees one level in one block, and the no-device error.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import ggml_ref as G
import linear_ref as R
import test_weight_layout_cpu as WL
from test_gpu_linear import _acts
from test_q3k_cpu import plan as plan_q3k            # noqa: F401  (fixtures: the drivers of the older type sets)
from test_weight_layout_cpu import plan as plan_default   # noqa: F401

KV = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.float64)


def fields(raw):
    """raw IQ4_XS rows -> d [nb][1], s_b [nb][8], level index [nb][8][32] of the nb super-blocks"""
    blk = np.ascontiguousarray(raw, np.uint8).reshape(-1, 136)
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float64)
    sh = blk[:, 2:4].copy().view(np.uint16).astype(np.int64)
    b = np.arange(8)
    ls = ((blk[:, 4 + b // 2].astype(np.int64) >> (4 * (b % 2))) & 15) | (((sh >> (2 * b)) & 3) << 4)
    qs = blk[:, 8:].astype(np.int64).reshape(-1, 8, 16)
    return d, ls - 32, np.concatenate([qs & 15, qs >> 4], axis=2)


def dec_iq4_xs(raw, n, k):
    d, s, idx = fields(raw)
    return (d[:, :, None] * s[:, :, None] * KV[idx]).reshape(n, k)


def rand_rows(rng, n, k):
    """every byte pattern is a valid block; d is drawn in f16 from [2^-8, 2^-4]"""
    blk = rng.integers(0, 256, (n * k // 256, 136), dtype=np.uint8)
    blk[:, 0:2] = (2.0 ** rng.uniform(-8, -4, (len(blk), 1))).astype(np.float16).view(np.uint8)
    return blk.reshape(-1)


@pytest.fixture(scope="module")
def plan_iq4(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wlayout_iq4xs") / "wlayout_iq4xs_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(WL.ROOT, "tests", "host", "wlayout_iq4xs_main.cpp")])

    def run(tensors, N, K):
        text = "%d %d 1 %d " % (N, K, len(tensors)) + " ".join("%d %d %d" % t for t in tensors) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        return dict(zip(WL.SCALARS, (int(x) for x in out[0].split()))), [int(x) for x in out[1].split()], [int(x) for x in out[2].split()], int(out[3])
    return run


@pytest.mark.parametrize("types", [[23], [23, 23, 13]])
def test_wlayout_and_plan(plan_iq4, q3, types):
    tensors, n = WL.stacked([(t, 64) for t in types])
    s, rg_types, offs, row_bytes = plan_iq4(tensors, n, 512)
    assert row_bytes == 2 * 136 and rg_types == [t for t in types for _ in range(2)] and s["nparts"] == len(set(types))
    assert offs[:2] == [0, 2 * 4096 // 16] and s["qbytes"] == sum(2 * 2 * {23: 4096, 13: 5120}[t] for t in types)   # the nibble plane alone
    assert s["meta_bytes"] == n * 2 * 16 and s["sc_bytes"] == n * 16 * 2
    W = [(np.zeros(64 * 2 * 136, np.uint8), t, 64) for t in types]   # the dispatch takes the type through the K-quant forms
    assert q3.linear_plan(q3.LOP_GEMV, W, K=512, nrows=n, ntok=1, kq_layout=1)[0] == "GEMV_KQ"
    assert q3.linear_plan(q3.LOP_GEMV, W, K=512, nrows=n, ntok=33, kq_layout=1)[0] == "GEMM_KQ_MFMA"


def test_older_type_sets_keep_refusing(plan_default, plan_q3k):
    for run in (plan_default, plan_q3k("default"), plan_q3k("kq4"), plan_q3k("kq3")):
        assert "unsupported weight type" in run([(23, 0, 32)], 32, 256)
        assert "unsupported weight type" in run([(13, 0, 32), (23, 32, 32)], 64, 256)


def test_q3synth_file_decodes_to_its_source_within_a_level_step(synth_tool, tmp_path, monkeypatch):
    monkeypatch.setitem(G.ROW_BYTES, 23, lambda k: k // 256 * 136)
    subprocess.check_call([synth_tool, "--out", str(tmp_path), "--preset", "tiny", "--what", "1", "--quant", "iq4_xs"])
    subprocess.check_call([synth_tool, "--out", str(tmp_path), "--preset", "tiny", "--what", "1", "--quant", "f32"])   # the same seeds: the source
    q = G.read_gguf(str(tmp_path / "gguf_iq4_xs" / "qwen3_tts_talker.gguf"))[1]
    f = G.read_gguf(str(tmp_path / "gguf" / "qwen3_tts_talker.gguf"))[1]
    ty = lambda nm: q["blk.%s.weight" % nm][0]
    assert [ty("0.attn_q"), ty("1.attn_k"), ty("0.attn_output"), ty("0.ffn_gate"), ty("1.ffn_up"), ty("1.ffn_down")] == [23] * 6
    assert (ty("0.attn_v"), ty("1.attn_v"), q["output.weight"][0]) == (13, 13, 14)
    for nm in ("blk.0.attn_q.weight", "blk.1.ffn_down.weight"):
        t, ne, raw = q[nm]
        src = np.array(f[nm][2]).view(np.float32).reshape(ne[1], ne[0]).astype(np.float64)
        d, s, _ = fields(np.array(raw))
        step = np.repeat((24 * d * np.abs(s)).reshape(ne[1], -1), 32, axis=1)   # 24: the widest gap between two levels
        assert (np.abs(dec_iq4_xs(np.array(raw), ne[1], ne[0]) - src) <= step).all() and s.min() > 0, nm


def test_bound_sees_one_level_in_one_block(oracle):
    """the inputs of the GPU test leave bound (a) something to say: one block of one row decoded one level off exceeds it (K = 256)"""
    rng = np.random.default_rng(256 * 7 + 3)
    raw = rand_rows(rng, 32, 256)
    xq, xd = _acts(rng, 3, 256)
    x64 = R.dequant_act(xq[:3], xd[:3])
    d, s, idx = fields(raw)
    a = dec_iq4_xs(raw, 32, 256)
    b = 4 + int(np.argmax(np.abs(s[0, 4:])))   # (blocks 0..3 of the activations hold the zero and tiny edge blocks)
    off = a.copy()
    off[0, 32 * b:32 * b + 32] = d[0, 0] * s[0, b] * KV[np.where(idx[0, b] < 15, idx[0, b] + 1, 14)]
    assert (np.abs(x64 @ off.T - x64 @ a.T)[:, 0] > R.bound_gemm(a, 0 * a, x64)[:, 0]).all()


def test_fails_cleanly_without_a_device(q3):
    if q3.device_count() > 0:
        return   # with a device present the no-device path cannot be observed (the suite's convention)
    xq = np.zeros((1, 256), np.int8); xd = np.zeros((1, 8), np.uint16); out = np.zeros(32, np.float32)
    with pytest.raises(q3.Q3Error, match="no HIP device"):
        q3.op_linear(q3.LOP_GEMV, "AUTO", [(rand_rows(np.random.default_rng(0), 32, 256), 23, 32)], K=256, nrows=32, ntok=1, xq=xq, xd=xd, a_rows=1,
                     out=out, out_stride=32, kq_layout=1)
