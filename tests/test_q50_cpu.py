"""Q5_0 on the host: the float64 decode of spec S3 and the Q8_0 twin (written out here, shared with tests/test_gpu_q50.py) against the oracle's
Q8_0 dequantiser, the packed layout plan and the refusals, q3synth's encoder and twin file, and the no-device error.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import ggml_ref as G
import linear_ref as R
import test_weight_layout_cpu as WL
from test_q3k_cpu import plan as plan_q3k            # noqa: F401  (fixtures: the drivers of the older type sets)
from test_q40_cpu import plan_q40                    # noqa: F401
from test_weight_layout_cpu import plan as plan_default   # noqa: F401


def fields(raw):
    """raw Q5_0 rows -> d [nb][1] (float64), q = u - 16 [nb][32] of the nb blocks, in weight order"""
    blk = np.ascontiguousarray(raw, np.uint8).reshape(-1, 22)
    qs, qh = blk[:, 6:].astype(np.int64), blk[:, 2:6].copy().view("<u4").astype(np.int64)
    return blk[:, 0:2].copy().view(np.float16).astype(np.float64), (np.concatenate([qs & 15, qs >> 4], axis=1) | ((qh >> np.arange(32)) & 1) << 4) - 16


def dec_q5_0(raw, n, k):
    d, q = fields(raw)
    return (d * q).reshape(n, k)


def widen(raw):
    """the Q8_0 twin: the same d over int8 (u - 16)"""
    out = np.zeros((len(raw) // 22, 34), np.uint8)
    out[:, :2] = np.ascontiguousarray(raw, np.uint8).reshape(-1, 22)[:, :2]
    out[:, 2:] = fields(raw)[1].astype(np.int8).view(np.uint8)
    return out.reshape(-1)


def rand_rows(rng, n, k):
    """every byte pattern is a valid block; d is drawn in f16 from +-[2^-8, 2^-4] (ggml's encoder writes either sign)"""
    blk = rng.integers(0, 256, (n * k // 32, 22), dtype=np.uint8)
    blk[:, 0:2] = (2.0 ** rng.uniform(-8, -4, (len(blk), 1)) * rng.choice([-1.0, 1.0], (len(blk), 1))).astype(np.float16).view(np.uint8)
    return blk.reshape(-1)


@pytest.mark.parametrize("k", [256, 2304])
def test_decoder_equals_oracle_dequant_of_the_twin(oracle, k):
    n = 3
    raw = rand_rows(np.random.default_rng(k), n, k)
    a = dec_q5_0(raw, n, k)
    twin = widen(raw).reshape(n, -1)
    got = np.zeros((n, k), np.float32)
    for r in range(n):
        row = np.ascontiguousarray(twin[r])
        oracle.lib().q3o_dequant_row(8, row.ctypes.data, k, got[r].ctypes.data)
    assert np.array_equal(a.astype(np.float32), got) and np.array_equal(R.dec_q8_0(twin.reshape(-1), n, k)[0], a)
    assert sorted(set(fields(raw)[1].reshape(-1))) == list(range(-16, 16))


@pytest.fixture(scope="module")
def plan_q50(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wlayout_q50") / "wlayout_q50_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(WL.ROOT, "tests", "host", "wlayout_q50_main.cpp")])

    def run(tensors, N, K):
        text = "%d %d 1 %d " % (N, K, len(tensors)) + " ".join("%d %d %d" % t for t in tensors) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        if out[0].startswith("error "):
            return out[0][6:]
        return dict(zip(WL.SCALARS, (int(x) for x in out[0].split()))), [int(x) for x in out[1].split()], [int(x) for x in out[2].split()], int(out[3])
    return run


@pytest.mark.parametrize("rows,k", [([32], 256), ([96], 512), ([64, 32, 32], 512)])
def test_wlayout_and_plan(plan_q50, q3, rows, k):
    tensors, n = WL.stacked([(6, r) for r in rows])
    s, rg_types, offs, row_bytes = plan_q50(tensors, n, k)
    nseg = k // 256
    assert row_bytes == k // 32 * 22 and rg_types == [6] * (n // 32) and s["nparts"] == 1 and s["p0_type"] == 6   # a fused q,k,v is one run
    assert offs == [i * nseg * 5120 // 16 for i in range(n // 32)] and s["qbytes"] == s["qs_bytes"] == n // 32 * nseg * 5120   # Q5_K's footprint
    assert s["sc_bytes"] == n * (k // 32) * 2 and s["meta_bytes"] == n * nseg * 16   # a scale per block, where Q8_0 keeps it; meta exists, unread
    W = [(np.zeros(r * k // 32 * 22, np.uint8), 6, r) for r in rows]   # the dispatch takes the type through the K-quant forms
    assert q3.linear_plan(q3.LOP_GEMV, W, K=k, nrows=n, ntok=1, kq_layout=1)[0] == "GEMV_KQ"
    assert q3.linear_plan(q3.LOP_GEMV, W, K=k, nrows=n, ntok=33, kq_layout=1)[0] == "GEMM_KQ_MFMA"


def test_refusals(plan_q50, plan_q40, plan_default, plan_q3k):
    for run in (plan_default, plan_q3k("default"), plan_q3k("kq4"), plan_q3k("kq3"), lambda *a: plan_q40(*a, "iq4"), plan_q40):
        assert "unsupported weight type" in run([(6, 0, 32)], 32, 256)
    for other in (13, 8, 12, 2):
        assert "Q5_0 tensors only" in plan_q50([(6, 0, 32), (other, 32, 32)], 64, 256)
        assert "Q5_0 tensors only" in plan_q50([(other, 0, 32), (6, 32, 32)], 64, 256)


def test_q3synth_file_round_trip_and_twin(synth_tool, tmp_path, monkeypatch):
    monkeypatch.setitem(G.ROW_BYTES, 6, lambda k: k // 32 * 22)
    for args in (["--quant", "q5_0"], ["--quant", "q5_0", "--q5_0-as-q8_0"], ["--quant", "f32"]):   # the same seeds: file, twin, source
        subprocess.check_call([synth_tool, "--out", str(tmp_path / args[-1].strip("-")), "--preset", "tiny", "--what", "1"] + args)
    q = G.read_gguf(str(tmp_path / "q5_0" / "gguf_q5_0" / "qwen3_tts_talker.gguf"))[1]
    t8 = G.read_gguf(str(tmp_path / "q5_0-as-q8_0" / "gguf_q8_0" / "qwen3_tts_talker.gguf"))[1]
    f = G.read_gguf(str(tmp_path / "f32" / "gguf" / "qwen3_tts_talker.gguf"))[1]
    ty = lambda nm: q["blk.%s.weight" % nm][0]
    assert [ty("0.attn_q"), ty("1.attn_k"), ty("0.attn_v"), ty("0.attn_output"), ty("0.ffn_gate"), ty("1.ffn_up"), ty("1.ffn_down")] == [6] * 7
    assert q["output.weight"][0] == 14
    seen = 0
    for nm, (t, ne, raw) in q.items():
        raw, (tt, net, rawt) = np.array(raw), t8[nm]
        if t != 6:   # the same bytes for every other tensor
            assert tt == t and np.array_equal(np.array(rawt), raw), nm
            continue
        w = dec_q5_0(raw, ne[1], ne[0])
        assert tt == 8 and net == ne and np.array_equal(np.array(rawt), widen(raw)) and np.array_equal(R.dec_q8_0(np.array(rawt), ne[1], ne[0])[0], w), nm
        # ggml's rounding: half a step, plus half a step more at level 31, where the encoder clips 32 to it (a value near -max), plus the f16
        # rounding of d (relative 2^-11 on up to 16 steps) and the f32 rounding of x / d + 16.5 (below 2^-18 of a step)
        src = np.array(f[nm][2]).view(np.float32).reshape(ne[1], ne[0]).astype(np.float64)
        d, qq = fields(raw)
        step = np.abs(np.repeat(d.reshape(ne[1], -1), 32, axis=1))
        clip = (qq.reshape(ne[1], ne[0]) == 15) * 0.5
        assert (np.abs(w - src) <= step * (0.5 + clip + 16 * 2.0 ** -11 + 2.0 ** -18)).all() and qq.min() == -16, nm
        seen += 1
    assert seen >= 14


def test_fails_cleanly_without_a_device(q3):
    if q3.device_count() > 0:
        return   # with a device present the no-device path cannot be observed (the suite's convention)
    xq = np.zeros((1, 256), np.int8); xd = np.zeros((1, 8), np.uint16); out = np.zeros(32, np.float32)
    with pytest.raises(q3.Q3Error, match="no HIP device"):
        q3.op_linear(q3.LOP_GEMV, "AUTO", [(rand_rows(np.random.default_rng(0), 32, 256), 6, 32)], K=256, nrows=32, ntok=1, xq=xq, xd=xd, a_rows=1,
                     out=out, out_stride=32, kq_layout=1)
