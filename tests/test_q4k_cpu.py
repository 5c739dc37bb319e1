"""Q4_K on the host: the float64 decoder against the Q5_K one on the widened bytes, the packed layout plan, the dispatch plan, and q3synth's
encoder with its Q5_K twin.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import ggml_ref as G
import linear_ref as R
import q3tts as Q
import q4k_ref as K4
import test_weight_layout_cpu as WL


def test_decoder_equals_q5k_decoder_on_the_twin():
    raw = K4.rand_rows_q4k(np.random.default_rng(4), 5, 768)
    a, b = K4.dec_q4_k(raw, 5, 768)
    a5, b5 = R.dec_q5_k(K4.widen(raw), 5, 768)
    assert np.array_equal(a, a5) and np.array_equal(b, b5) and a.max() > 0


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan_wlayout with the type set of the engine's builders (tests/host/wlayout_main.cpp plans with the default set, which has no Q4_K)"""
    exe = str(tmp_path_factory.mktemp("wlayout_q4k") / "wlayout_q4k_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(WL.ROOT, "tests", "host", "wlayout_q4k_main.cpp")])

    def run(tensors, N, K, force=0):
        text = "%d %d %d %d " % (N, K, force, len(tensors)) + " ".join("%d %d %d" % t for t in tensors) + "\n"
        out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
        if out[0].startswith("error "):
            return out[0][6:]
        return dict(zip(WL.SCALARS, (int(x) for x in out[0].split()))), [int(x) for x in out[1].split()], [int(x) for x in out[2].split()]
    return run


@pytest.mark.parametrize("types", [[12], [12, 14], [12, 14, 8]])
def test_wlayout(plan, types, monkeypatch):
    monkeypatch.setitem(WL.SEG_BYTES, 12, 4096)   # the documented size: the nibble plane [8][2][32][8 B] and nothing after it
    tensors, n = WL.stacked([(t, 64) for t in types])
    s, rg_types, offs = WL.check(plan, tensors, n, 512)
    assert s["nparts"] == len(types) and rg_types == [t for t in types for _ in range(2)]
    assert offs[:2] == [0, 2 * 4096 // 16] and s["qbytes"] == sum(2 * 2 * WL.SEG_BYTES[t] for t in types)
    assert s["meta_bytes"] == n * 2 * 16


@pytest.mark.parametrize("op,K,nrows,ff", [(Q.LOP_GEMV, 2048, 2048, 0), (Q.LOP_GEMV, 3072, 1024, 0), (Q.LOP_GEMV, 1024, 64, 0), (Q.LOP_GATEUP, 2048, 12288, 6144),
                                           (Q.LOP_NORM_GEMV, 2048, 4096, 0), (Q.LOP_NORM_ARGMAX, 1024, 2048, 0), (Q.LOP_NORM_GATEUP, 1024, 6144, 3072)])
def test_plan_gives_q4k_the_forms_of_q5k(q3, op, K, nrows, ff):
    for nt in (1, 8, 16, 300):
        got = [Q.linear_plan(op, weights=[(np.zeros(0, np.uint8), t, nrows)], K=K, nrows=nrows, ntok=nt, ff=ff, out_stride=nrows, kq_layout=1)
               for t in (12, 13)]
        assert got[0] == got[1], (nt, got)
    # (K = 1024, 64 rows: few enough row groups for 8 lanes per row, which Q6_K matrices are capped out of)
    if nrows == 64:
        assert Q.linear_plan(op, weights=[(np.zeros(0, np.uint8), 12, 64)], K=K, nrows=64, ntok=1, kq_layout=1)[:2] == ("GEMV_KQ", 8)


@pytest.fixture(scope="module")
def synth3(synth_tool, tmp_path_factory):
    """blk.0.attn_q.weight of the tiny talker three times from one seed: f32, Q4_K, and the Q5_K twin"""
    out = {}
    mp = pytest.MonkeyPatch()
    mp.setitem(G.ROW_BYTES, 12, lambda k: k // 256 * 144)   # read_gguf sizes tensors by this table; undone below
    for name, args, sub in (("f32", ["--quant", "f32"], "gguf"), ("q4", ["--quant", "q4_k_m"], "gguf_q4_k_m"),
                            ("twin", ["--quant", "q4_k_m", "--q4k-as-q5k"], "gguf_q5_k_m")):
        d = str(tmp_path_factory.mktemp("q4k_" + name))
        subprocess.check_call([synth_tool, "--out", d, "--preset", "tiny", "--what", "1"] + args)
        ty, ne, raw = G.read_gguf(os.path.join(d, sub, "qwen3_tts_talker.gguf"))[1]["blk.0.attn_q.weight"]
        out[name] = (ty, ne, np.array(raw))
    mp.undo()
    return out


def test_q3synth_encoder_round_trip(synth3):
    """Interior values (q in 1..14) round-trip within half a step d * sc.  An end value (q = 0 or 15) may have been clamped: the 6-bit codes
    put the block's range off by at most dmin / 2 (the min) and 15 * d / 2 (fifteen steps, each off by d / 2), which is added there.
    1e-6 of the value covers the encoder's f32 arithmetic.  Few values may take that slack: a block's extremes are its only clamped values, and with
    steps of a fifteenth of the range the values within half a step of either extreme are 1/15 of a uniform block plus the two extremes themselves,
    (32 / 15 + 2) / 32 = 13 %; bell-shaped blocks have fewer.  At most 15 % end codes."""
    ty, ne, raw = synth3["q4"]
    assert ty == 12
    k, n = ne[0], ne[1]
    x = np.array(synth3["f32"][2]).view(np.float32).astype(np.float64).reshape(n, k)
    a, b = K4.dec_q4_k(np.array(raw), n, k)
    blk = np.array(raw).reshape(-1, 144)
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float64)[:, 0]; dmin = blk[:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]
    sc, _ = R._scale_min(blk[:, 4:16])
    step = np.repeat((d[:, None] * sc).reshape(-1), 32).reshape(n, k)
    q = np.where(step > 0, np.rint(a / np.where(step > 0, step, 1)), 0)
    slack = np.where((q == 0) | (q == 15), np.repeat(dmin / 2 + 7.5 * d, 256).reshape(n, k), 0)
    assert (np.abs(x - (a - b)) <= step / 2 + slack + 1e-6 * np.abs(x)).all()
    ends = (q == 0) | (q == 15)
    print("end codes %.4f, beyond half a step %.5f" % (ends.mean(), (np.abs(x - (a - b)) > step / 2 + 1e-6 * np.abs(x)).mean()))
    assert ends.mean() <= 0.15


def test_q3synth_twin_decodes_to_the_same_matrix(synth3):
    (t4, ne, raw4), (t5, ne5, raw5) = synth3["q4"], synth3["twin"]
    assert (t4, t5) == (12, 13) and ne == ne5
    assert np.array_equal(K4.widen(np.array(raw4)), np.array(raw5))
    a4, b4 = K4.dec_q4_k(np.array(raw4), ne[1], ne[0]); a5, b5 = R.dec_q5_k(np.array(raw5), ne[1], ne[0])
    assert np.array_equal(a4, a5) and np.array_equal(b4, b5)
