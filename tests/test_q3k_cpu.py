"""Q3_K on the host: the float64 decoder against the oracle's Q6_K dequantiser on the widened twin, the oracle's block chain on the twin against
float64, the packed layout plan, and q3synth's Q3_K_M file with its twin.  No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import ggml_ref as G
import linear_ref as R
import q3k_ref as K3
import test_weight_layout_cpu as WL
from test_gpu_linear import _acts


@pytest.mark.parametrize("k", [256, 2304])
def test_decoder_equals_oracle_dequant_of_the_twin(oracle, k):
    n = 3
    raw = K3.rand_rows_q3k(np.random.default_rng(k), n, k)
    a, b = K3.dec_q3_k(raw, n, k)
    twin = K3.widen_to_q6k(raw).reshape(n, -1)
    got = np.zeros((n, k), np.float32)
    for r in range(n):
        row = np.ascontiguousarray(twin[r])
        oracle.lib().q3o_dequant_row(14, row.ctypes.data, k, got[r].ctypes.data)
    assert np.array_equal(a.astype(np.float32), got) and not b.any() and np.abs(a).max() > 0
    assert np.array_equal(R.dec_q6_k(twin.reshape(-1), n, k)[0], a)


@pytest.mark.parametrize("k", [256, 2304])
def test_oracle_matvec_on_the_twin_is_within_bound_gemm(oracle, k):
    n, nt = 32, 3
    rng = np.random.default_rng(k + 1)
    raw = K3.rand_rows_q3k(rng, n, k)
    xq, xd = _acts(rng, nt, k)
    y = R.sum_slabs(R.oracle_slabs(oracle.lib(), [(K3.widen_to_q6k(raw), 14, n)], k, 0, n, xq[:nt], xd[:nt])).astype(np.float64)
    a, b = K3.dec_q3_k(raw, n, k)
    x64 = R.dequant_act(xq[:nt], xd[:nt])
    assert (np.abs(y - x64 @ a.T) <= R.bound_gemm(a, b, x64)).all()


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """plan_wlayout with a type set chosen per call: "kq3" is what the engine's builders pass"""
    exe = str(tmp_path_factory.mktemp("wlayout_q3k") / "wlayout_q3k_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(WL.ROOT, "tests", "host", "wlayout_q3k_main.cpp")])

    def make(types):
        def run(tensors, N, K, force=0):
            text = "%d %d %d %d " % (N, K, force, len(tensors)) + " ".join("%d %d %d" % t for t in tensors) + "\n"
            out = subprocess.run([exe, types], input=text, capture_output=True, text=True, check=True).stdout.splitlines()
            if out[0].startswith("error "):
                return out[0][6:]
            return dict(zip(WL.SCALARS, (int(x) for x in out[0].split()))), [int(x) for x in out[1].split()], [int(x) for x in out[2].split()]
        return run
    return make


@pytest.mark.parametrize("types", [[11], [11, 11, 13], [11, 11, 12]])
def test_wlayout(plan, types, monkeypatch):
    # the documented sizes: 2-bit plane [8][32][8 B] + bit plane [32][8][4 B] = 3072 B of quants; with 512 B of metadata and 64 B of d: 3648 B
    monkeypatch.setitem(WL.SEG_BYTES, 11, 2048 + 1024)
    monkeypatch.setitem(WL.SEG_BYTES, 12, 4096)
    tensors, n = WL.stacked([(t, 64) for t in types])
    s, rg_types, offs = WL.check(plan("kq3"), tensors, n, 512)
    assert s["nparts"] == len(set(types)) and rg_types == [t for t in types for _ in range(2)]
    assert offs[:2] == [0, 2 * 3072 // 16] and s["qbytes"] == sum(2 * 2 * WL.SEG_BYTES[t] for t in types)
    assert s["meta_bytes"] == n * 2 * 16
    if types == [11]:   # per (row group, segment): quants + metadata + one f16 d per row
        assert s["qs_bytes"] // 4 + s["meta_bytes"] // 4 + 32 * 2 == 3648


@pytest.mark.parametrize("which", ["default", "kq4"])
def test_wlayout_refuses_q3k_where_the_caller_has_no_body(plan, which):
    assert "unsupported weight type" in plan(which)([(11, 0, 32)], 32, 256)
    assert "unsupported weight type" in plan(which)([(13, 0, 32), (11, 32, 32)], 64, 256)


@pytest.fixture(scope="module")
def synth(synth_tool, tmp_path_factory):
    """the tiny talker from one seed as Q3_K_M, as its twin with Q3_K -> Q6_K, and as the oracle's twin with Q4_K -> Q5_K as well"""
    out = {}
    mp = pytest.MonkeyPatch()
    mp.setitem(G.ROW_BYTES, 11, lambda k: k // 256 * 110)   # read_gguf sizes tensors by this table; undone below
    mp.setitem(G.ROW_BYTES, 12, lambda k: k // 256 * 144)
    for name, args, sub in (("q3", [], "gguf_q3_k_m"), ("twin", ["--q3k-as-q6k"], "gguf_q4_k_m"), ("twin5", ["--q3k-as-q6k", "--q4k-as-q5k"], "gguf_q5_k_m")):
        d = str(tmp_path_factory.mktemp("q3k_" + name))
        subprocess.check_call([synth_tool, "--out", d, "--preset", "tiny", "--what", "1", "--quant", "q3_k_m"] + args)
        out[name] = {nm: (ty, ne, np.array(raw)) for nm, (ty, ne, raw) in G.read_gguf(os.path.join(d, sub, "qwen3_tts_talker.gguf"))[1].items()}
    mp.undo()
    return out


def test_q3synth_mix_and_twin(synth):
    q3, twin, twin5 = synth["q3"], synth["twin"], synth["twin5"]
    ty = lambda nm: q3["blk.%s.weight" % nm][0]
    assert [ty("0.attn_q"), ty("1.attn_k"), ty("0.ffn_gate"), ty("1.ffn_up")] == [11] * 4
    assert (ty("0.attn_v"), ty("1.attn_v"), ty("0.attn_output"), ty("1.ffn_down"), q3["output.weight"][0]) == (13, 13, 12, 12, 14)
    seen = 0
    for nm, (t, ne, raw) in q3.items():
        t6, ne6, raw6 = twin[nm]
        assert ne6 == ne and twin5[nm][0] == {11: 14, 12: 13}.get(t, t)
        if t != 11:   # the same bytes for every other tensor
            assert t6 == t and np.array_equal(raw6, raw), nm
            continue
        assert t6 == 14 and np.array_equal(K3.widen_to_q6k(raw), raw6) and np.array_equal(twin5[nm][2], raw6), nm
        a, _ = K3.dec_q3_k(raw, ne[1], ne[0])
        assert np.array_equal(a, R.dec_q6_k(raw6, ne[1], ne[0])[0]) and np.abs(a).max() > 0
        seen += 1
    assert seen >= 9   # q, k, gate, up of two layers and the token embedding
