"""Register budget of the batched attention kernel (cross-compiled here, no GPU needed; code-object metadata only).

A 64-token talker step is 64 x 16 = 1024 workgroups of four waves.  They are co-resident in one round only at four waves per SIMD, i.e. at
most 128 VGPRs, and k_attention now holds a 256-chunk's K rows and up to 16 V row groups in registers while they are in flight.  One
prefetch batch too many tips the launch into two rounds (or into scratch, ~2 us per launch): that must fail here, not in the next bench."""
import os
import re

import pytest

from test_isa_guard_cpu import CSRC, HIPCC, _asm


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_batched_attention_fits_one_round_without_scratch(tmp_path):
    text = _asm(os.path.join(CSRC, "kernels.hip"), str(tmp_path))
    meta = text[text.index("amdhsa.kernels"):]
    seen = 0
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if not re.match(r"_ZN2q311k_attention[EI]", name):     # q3::k_attention and any instantiation of it; not k_attention_fused / _short
            continue
        seen += 1
        assert int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)) == 0, name
        # one body serves every token count (launch_attention has no second instantiation), so it is the one used for at most 128 tokens
        assert int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)) <= 128, name
    assert seen >= 1
