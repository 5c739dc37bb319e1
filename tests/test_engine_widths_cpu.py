"""Host-only checks that keep the engine step-width sweep (tests/test_gpu_engine_widths.py) honest: the restated width rules of
tests/engine_width_cases.py, that its length patterns replay every width, and which linear and attention forms (q3tts_linear_plan,
q3tts_attention_plan) the case table reaches on the tiny model -- written out, with the forms it cannot reach named.  No GPU needed."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import engine_width_cases as W
import q3tts as Q
from test_linear_plan_cpu import _launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the width rules ------------------------------------------------------------
def test_graph_widths():
    assert W.graph_widths(1) == {1} and W.graph_widths(2) == {1, 2} and W.graph_widths(8) == {1, 2, 4, 8}
    assert W.graph_widths(9) == {1, 2, 4, 8, 9} and W.graph_widths(17) == {1, 2, 4, 8, 16, 17}
    assert W.graph_widths(129) == {1, 2, 4, 8, 16, 32, 64, 128, 129} and W.graph_widths(256) == {1, 2, 4, 8, 16, 32, 64, 128, 256}
    src = open(os.path.join(ROOT, "qwen3-tts-rust_amd", "csrc", "engine.cpp")).read()     # the rule restated is the rule compiled
    m = re.search(r"static int pick_width\(int hi, int W\) \{[^\n]*\n(.*?)\n\}", src, re.S)
    assert [l.strip() for l in m.group(1).splitlines()] == ["int w = 1;", "while (w < hi) w <<= 1;", "return std::min(w, W);"]
    assert "const int width = pick_width(hi, B_);" in src and "const int group = std::max(1, std::min(4, remaining));" in src


def test_lengths_formula():
    assert W.lengths(1) == [4] and W.lengths(2) == [8, 4] and W.lengths(4) == [12, 8, 4, 4]
    assert W.lengths(9) == [20, 16, 12, 12, 8, 8, 8, 8, 4]                       # B_ceil = 16
    L = W.lengths(256)
    assert L[0] == 36 and L[1] == 32 and L[15] == 20 and L[16] == 16 and L[127] == 8 and L[128] == 4 and L[255] == 4
    for B in sorted({c[1] for c in W.CASES}):
        bc = 1 << (B - 1).bit_length()
        assert W.lengths(B) == [min(36, 4 * (1 + int(np.floor(np.log2(bc / (b + 1)))))) for b in range(B)]
        assert max(W.lengths(B)) <= W.MAX_FRAMES and all(n % W.GROUP == 0 for n in W.lengths(B))


@pytest.mark.parametrize("c", W.CASES, ids=[W.case_id(c) for c in W.CASES])
def test_patterns_replay_the_widths(c):
    _, B, pattern, _, _ = c
    ran = W.simulate(W.PATTERNS[pattern](B))
    if pattern == "lengths":
        assert set(ran) == W.graph_widths(B) and ran[0] == B and ran == sorted(ran, reverse=True)
    else:
        assert ran == [B, B, B]                                                  # two groups with B - 2 dead slots between the live ends


def test_case_table():
    table = {}
    for quant, B, pattern, codec, flavour in W.CASES:
        table.setdefault((quant, pattern, flavour), []).append(B)
    assert table == {("q8_0", "lengths", "plain"): [9, 15, 16, 17, 33, 64, 65, 96, 97, 128, 129, 193, 256],
                     ("q5_k_m", "lengths", "plain"): [15, 16, 17, 33, 129, 256],
                     ("bf16", "lengths", "plain"): [8, 95, 96, 129, 256],
                     ("q8_0", "holes", "plain"): [129, 256], ("q5_k_m", "holes", "plain"): [129],
                     ("q8_0", "lengths", "all_variants"): [129, 256], ("q5_k_m", "lengths", "all_variants"): [129]}
    assert sorted((c[0], c[1]) for c in W.CASES if c[3]) == [("bf16", 96), ("q8_0", 33), ("q8_0", 256)]
    assert len(W.CASES) == len(set(W.CASES)) == 30
    for i in range(256):
        assert W.text_ids(i).size == 3 + (7 * i) % 23
    o = [W.options(i, "all_variants") for i in range(12)]
    assert [i for i in range(12) if o[i]["temperature"] > 0] == [2, 7] and [i for i in range(12) if "trailing_ids" in o[i]] == [0, 4, 8]
    assert [i for i in range(12) if o[i].get("repetition_penalty") == 1.1 and o[i].get("predictor_temperature") == 0.9] == [0, 3, 6, 9]
    assert all(set(W.options(i, "plain")) == {"temperature", "top_k", "top_p", "seed", "mask_eos"} for i in range(12))


# ------------------------------------------------------------------ which forms the table reaches ----------------------------------------------
def _tiny_dims():
    """talker / predictor dimensions of the tiny synthetic model, read from tools/q3synth.c as test_linear_plan_cpu reads the full-size ones"""
    src = open(os.path.join(ROOT, "tools", "q3synth.c")).read()
    m = re.search(r'if \(!strcmp\(preset, "tiny"\)\).*?talker = \(tfcfg\)\{([^}]*)\};\s*pred = \(tfcfg\)\{([^}]*)\};', src, re.S)
    out = []
    for grp in m.groups():
        d, nl, nh, nkv, ff, nv, _ = [int(x) for x in grp.split(",")]
        out.append(dict(d=d, nh=nh, nkv=nkv, ff=ff, nv=nv))
    return out


TILED = ("GEMM_Q8_MFMA", "GEMM_Q8_TILE1", "GEMM_KQ_MFMA", "GU_Q8_TILE1", "GU_Q8_MFMA", "GU_KQ_MFMA")   # forms with a token-tile grid dimension z
TL_STRIDE = 2176   # rows of the talker head launch: Q3_SAMPLE_END = 2160 padded to 32 (Engine::tl_stride_)


def _plan(entry, quant, ntok):
    op, K, row0, nrows, ff, tensors = entry
    if quant == "q8_0" and tensors:
        tensors = [(8, sum(n for _, n in tensors))]
    weights = [(np.zeros(0, np.uint8), t, n) for t, n in tensors]
    return Q.linear_plan(op, weights=weights, K=K, row0=row0, nrows=nrows, ntok=ntok, ff=ff, x_stride=K, out_stride=nrows,
                         kq_layout=int(quant == "q5_k_m"))


def _step_forms(quant, w):
    """(linear plans "FORM" or "FORM/z<ntiles", attention forms) of one frame at step width w, following Engine::record_frame: the predictor's
    two-row pass over 2 w tokens (same_seq) and its head over w, fourteen predictor passes over w tokens and their heads, the talker step over
    w tokens and its head; Transformer::forward takes the 5-launch walk for quantised weights up to 8 tokens, the unfused walk otherwise"""
    talker, pred = _tiny_dims()
    flt = quant == "bf16"
    lin, att = set(), set()

    def add(entry, ntok):
        f, _, _, z = _plan(entry, quant, ntok)
        lin.add(f + ("/z<ntiles" if f in TILED and z < (ntok + 31) // 32 else ""))

    def walk(c, head_rows, head_row0, ntok, head_tok, **attn):
        L = _launches(c, quant, head_rows, head_row0)
        fused = not flt and ntok <= 8
        names = ["qkv_norm", "o", "gu_norm", "down"] if fused else ["norm", "qkv", "o", "gate_up", "down"]
        names += [n + s for n in names for s in ("_v6", "_q6") if n + s in L]
        for n in names:
            add(L[n], ntok)
        if fused:                                          # the final norm is the head GEMV's prologue: logits or the argmax epilogue
            add(L["head"], head_tok); add(L["head_argmax"], head_tok)
        else:                                              # the output matrix over the final norm's rows (one matmul by mode)
            op, K, row0, nrows, ff, tensors = L["head"]
            add((Q.LOP_F_GEMV if flt else Q.LOP_GEMV, K, row0, nrows, ff, tensors), head_tok)
        att.add(Q.attention_plan(ntok, n_head=c["nh"], n_kv=c["nkv"], float_mode=flt, **attn))

    walk(pred, 2048, 0, 2 * w, w, short_attn_min=8, same_seq=True)
    walk(pred, 2048, 2048, w, w, short_attn_min=8)
    walk(talker, TL_STRIDE, 0, w, w)
    return lin, att


def _reached(quant):
    lin, att = set(), set()
    for B in sorted({c[1] for c in W.CASES if c[0] == quant}):
        for w in W.graph_widths(B):
            l, a = _step_forms(quant, w)
            lin |= l; att |= a
    return lin, att


# written out by hand from plan_linear / plan_attention and the tiny dimensions (talker K = 2048, 256 q + 2 x 128 kv rows, ff 512; predictor
# K = 256, ff 512): a change of the dispatch or of the case table that loses a form fails here
REACHED = {
    "q8_0": ({"GEMV_NORM", "GEMV_NORM_ARGMAX", "GU_SWIGLU_NORM", "GEMV_Q8",            # the 5-launch walk, steps of 1..8 tokens
              "NORM_WG", "GEMM_Q8_TOK",                                                  # 9..15 tokens: the unfused walk (its norm below 9 tokens, NORM, is float-only)
              "GEMM_Q8_MFMA", "GEMM_Q8_TILE1", "GU_UNFUSED", "GU_Q8_TILE1",              # from 16 tokens; GU_UNFUSED: the predictor (K = 256)
              "GEMM_Q8_WIDE"},                                                           # the two-row pass of steps above 128 slots: 2 w > 256
             {"FUSED", "UNFUSED", "SHORT1", "SHORT2"}),
    "q5_k_m": ({"GEMV_NORM", "GEMV_NORM_ARGMAX", "GU_SWIGLU_NORM", "GEMV_KQ", "NORM_WG", "GEMM_KQ_MFMA", "GU_UNFUSED", "GU_KQ_MFMA"},
               {"FUSED", "UNFUSED", "SHORT1", "SHORT2"}),
    "bf16": ({"NORM", "NORM_WG", "F_GEMV", "F_MFMA16", "F_MFMA", "F_GU_UNFUSED", "F_GU_MFMA16"}, {"UNFUSED", "SHORT1", "SHORT2"}),
}

# forms plan_linear can return for a decode step of at most 256 slots that the tiny dimensions never reach, and why
UNREACHED = {
    "GEMM_Q8_MFMA/z<ntiles": "tiny matrices have at most 68 row groups: mfma_ztiles gives z == ntiles; the Q3_MFMA_WGS=16 child run forces z = 1",
    "GEMM_KQ_MFMA/z<ntiles": "as GEMM_Q8_MFMA; the child run covers it",
    "GU_Q8_MFMA": "at z == ntiles only for activations off a 4-byte boundary, which the engine's buffers never are",
    "GU_Q8_MFMA/z<ntiles": "tiny ff / 32 = 16 workgroups per tile: z == ntiles, which is GU_Q8_TILE1; the child run covers it at z = 2",
    "GU_KQ_MFMA/z<ntiles": "as GU_Q8_MFMA; the child run covers it",
    "GU_Q8_WIDE": "needs K = 1024 or 2048 above 256 tokens: only the predictor's two-row pass is that wide in decode, and the tiny predictor has K = 256",
}


@pytest.mark.parametrize("quant", sorted(REACHED))
def test_forms_reached(quant):
    lin, att = _reached(quant)
    assert lin == REACHED[quant][0], (sorted(lin - REACHED[quant][0]), sorted(REACHED[quant][0] - lin))
    assert att == REACHED[quant][1]


def test_unreached_forms_are_the_listed_ones():
    """every form name of the library, with the z < ntiles variants of the tiled int8 GEMMs, is reached by some case or listed with its reason"""
    everything = set(Q.LIN_FORMS[1:]) | {f + "/z<ntiles" for f in TILED}
    reached = set().union(*[REACHED[q][0] for q in REACHED])
    assert reached <= everything and set(UNREACHED) <= everything and not reached & set(UNREACHED)
    assert everything - reached - set(UNREACHED) == {"GEMM_Q8_TILE1/z<ntiles", "GU_Q8_TILE1/z<ntiles"}   # no such plans: TILE1 means z == ntiles
    assert len(UNREACHED) <= 6


def test_boundaries_are_widths():
    """each dispatch boundary the table names is a width of some case, on both sides"""
    def widths(q):
        return set().union(*[W.graph_widths(c[1]) for c in W.CASES if c[0] == q])
    assert {8, 9, 15, 16, 17, 32, 33, 64, 65, 96, 97, 128, 129, 193, 256} <= widths("q8_0")
    assert {8, 15, 16, 17, 128, 129, 256} <= widths("q5_k_m") and {1, 2, 8, 64, 95, 96, 128, 129, 256} <= widths("bf16")
    talker, pred = _tiny_dims()
    gemv = _launches(pred, "q8_0", 2048, 2048)["o"]
    assert [_plan(gemv, "q8_0", n)[0] for n in (8, 9, 15, 16)] == ["GEMV_Q8", "GEMM_Q8_TOK", "GEMM_Q8_TOK", "GEMM_Q8_TILE1"]
    assert [_plan(_launches(talker, "q5_k_m", TL_STRIDE, 0)["o"], "q5_k_m", n)[0] for n in (15, 16)] == ["GEMV_KQ", "GEMM_KQ_MFMA"]
    f = _launches(talker, "bf16", TL_STRIDE, 0)
    assert [_plan(f["gate_up"], "bf16", n)[0] for n in (95, 96)] == ["F_GU_MFMA16", "F_GU_UNFUSED"]
    assert [_plan(f["qkv"], "bf16", n)[0] for n in (95, 96)] == ["F_MFMA16", "F_MFMA"]
    assert [Q.attention_plan(n, n_head=2, n_kv=1, short_attn_min=8) for n in (7, 8, 128, 129)] == ["FUSED", "SHORT1", "SHORT1", "SHORT2"]


Z1_CHILD = (
    "import sys, json, numpy as np\n"
    "sys.path[:0] = %r\n"
    "import test_engine_widths_cpu as T\n"
    "out = {}\n"
    "for quant in ('q8_0', 'q5_k_m'):\n"
    "    t, p = T._tiny_dims()\n"
    "    for model, c, rows, row0 in (('talker', t, T.TL_STRIDE, 0), ('predictor', p, 2048, 2048)):\n"
    "        L = T._launches(c, quant, rows, row0)\n"
    "        for n in ('qkv', 'o', 'gate_up', 'down'):\n"
    "            out['%%s %%s %%s' %% (quant, model, n)] = T._plan(L[n], quant, 256)\n"
    "print(json.dumps(out))\n"
)


def z1_plans():
    """{"quant model launch": [form, lpr, mt, z]} of the tiny model's 256-token GEMMs under Q3_MFMA_WGS=16, planned in a process of its own
    (the library reads the variable once)"""
    env = dict(os.environ, Q3_MFMA_WGS="16")
    path = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "qwen3-tts-rust_amd", "python")]
    r = subprocess.run([sys.executable, "-c", Z1_CHILD % (path,)], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    import json
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_child_environment_walks_all_token_tiles():
    """under Q3_MFMA_WGS=16 every tiled int8 GEMM of a 256-slot step with at least 16 row groups runs z = 1 (one workgroup walks all eight
    token tiles); the predictor's 256-row o- and down-projections (8 row groups) and the gate/up GEMMs (a workgroup parks at most four tiles
    of gate sums) run z = 2, four tiles per workgroup.  Without the variable all of them run z == ntiles == 8"""
    plans = z1_plans()
    talker, pred = _tiny_dims()
    for key, (form, _, _, z) in plans.items():
        quant, model, name = key.split()
        if name == "gate_up":
            want = ("GU_UNFUSED", 0) if model == "predictor" else ("GU_Q8_MFMA" if quant == "q8_0" else "GU_KQ_MFMA", 2)
        else:
            want = ("GEMM_Q8_MFMA" if quant == "q8_0" else "GEMM_KQ_MFMA", 2 if model == "predictor" and name in ("o", "down") else 1)
        assert (form, z) == want, key
        L = _launches(talker if model == "talker" else pred, quant, 2048, 0)
        if name != "gate_up" or model == "talker":
            assert _plan(L[name], quant, 256)[3] == 8, key
