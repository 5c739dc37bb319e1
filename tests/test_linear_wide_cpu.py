"""Host-only checks of the wide prompt-chunk GEMM forms (GEMM_Q8_WIDE / GU_Q8_WIDE, k_gemm_q8_wide): what q3tts_linear_plan answers above 256
tokens, and the register / scratch / LDS budget of the two kernel variants as cross-compiled for gfx950.  No GPU needed."""
import os
import re

import numpy as np
import pytest

import q3tts as Q
import test_isa_guard_cpu as G
import test_linear_plan_cpu as P


def _plan(c, quant, name, nt):
    op, K, row0, nrows, ff, tensors = P._launches(c, quant, c["nv"], 0)[name]
    if quant == "q8_0":
        tensors = [(8, sum(n for _, n in tensors))]
    weights = [(np.zeros(0, np.uint8), t, n) for t, n in tensors]
    return Q.linear_plan(op, weights=weights, K=K, row0=row0, nrows=nrows, ntok=nt, ff=ff, x_stride=K, out_stride=nrows, kq_layout=int(quant == "q5_k_m"))


def test_plan_above_256_tokens(monkeypatch):
    monkeypatch.delenv("Q3_PREFILL_WIDE", raising=False)
    talker = P._full_dims()[0]
    for name, form in (("qkv", "GEMM_Q8_WIDE"), ("o", "GEMM_Q8_WIDE"), ("down", "GEMM_Q8_WIDE"), ("gate_up", "GU_Q8_WIDE")):   # the talker's four Q8_0 shapes
        for nt, z in ((257, 9), (512, 16)):                                                                                       # ztiles = token tiles
            assert _plan(talker, "q8_0", name, nt) == (form, 0, 0, z), (name, nt)
        assert _plan(talker, "q8_0", name, 256)[0] in ("GEMM_Q8_MFMA", "GU_Q8_MFMA"), name          # at 256 tokens: what it was
    for name in ("qkv", "o", "down", "gate_up", "qkv_v6", "down_q6"):                                  # Q5_K_M files keep their forms at every width
        for nt in (257, 512):
            assert _plan(talker, "q5_k_m", name, nt)[0] in ("GEMM_KQ_MFMA", "GU_KQ_MFMA"), (name, nt)
    for quant in ("bf16", "f16"):
        for nt in (257, 512):
            assert _plan(talker, quant, "qkv", nt)[0] == "F_MFMA" and _plan(talker, quant, "gate_up", nt)[0] == "F_GU_UNFUSED"


def test_switch_restores_the_old_forms(monkeypatch):
    monkeypatch.setenv("Q3_PREFILL_WIDE", "0")
    talker = P._full_dims()[0]
    for name, form in (("qkv", "GEMM_Q8_MFMA"), ("o", "GEMM_Q8_MFMA"), ("down", "GEMM_Q8_MFMA"), ("gate_up", "GU_Q8_MFMA")):
        for nt in (257, 512):
            assert _plan(talker, "q8_0", name, nt)[0] == form, (name, nt)


@pytest.mark.skipif(not os.path.exists(G.HIPCC), reason="hipcc not installed")
def test_wide_kernels_use_no_scratch(tmp_path):
    """k_gemm_q8_wide is built for two waves per SIMD (256 registers) and two workgroups per CU (80 KiB of LDS each); the rule of
    test_hot_q8_kernels_use_no_scratch holds for it as well: no private segment"""
    text = G._asm(os.path.join(G.CSRC, "kernels.hip"), str(tmp_path))
    meta = text[text.index("amdhsa.kernels"):]
    seen = 0
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_gemm_q8_wide" in name:
            seen += 1
            assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
            assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 256, name
            assert int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1)) <= 80 * 1024, name
    assert seen == 2
