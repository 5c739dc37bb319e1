"""The batched attention pair (k_qk_rope_append + k_attention, form UNFUSED) at the widths and contexts where k_attention's load schedule
changes path: the kernel requests a 256-chunk's K rows and its V rows in four batches of 64 positions (one page each; four row groups of 16
per batch), runs one instance of the chunk per number of batches the token reaches, and inside the last batch clamps a row past the
token's last position to that position.  So every edge is a multiple of 16, 64 or 256: the contexts below sit at n - 1, n, n + 1 around them, mixed in one 64-token launch, on permuted
pages with everything the launch may not read set to NaN.  The head -> workgroup map (q heads of one kv head on one XCD) must be a
bijection for every head layout.  Bit for bit against the oracle and the clean-cache run, and within the float64 bound.  (-m gpu)"""
import numpy as np
import pytest

import attention_cases as AC
from attention_cases import expect, check_f64

pytestmark = pytest.mark.gpu

EDGES = [1, 2, 15, 16, 17, 63, 64, 65, 79, 80, 81, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 511, 512, 513]
GQA = [(4, 4), (4, 2), (8, 2), (16, 2), (16, 8), (2, 1)]


def _wide64():
    return AC.Problem("wide64_edges", 700, [(EDGES[i % len(EDGES)] - 1, 1) for i in range(64)], n_layer=2, layer=1, pos="distinct")


def _gqa(h, k):
    return AC.Problem("wide_gqa%d_%d" % (h, k), 710 + 8 * h + k, [(n - 1, 1) for n in (3, 70, 130, 300)] * 4, n_head=h, n_kv=k, n_layer=2,
                      layer=(h + k) % 2, pos="distinct")


def _prefill():
    return AC.Problem("prefill_edges", 720, [(60, 9), (124, 10), (250, 12), (0, 3)], n_layer=2, layer=1, pos="distinct")


def _run(q3, P, form, poison=True, **flags):
    args, kw = P.op_args(poison)
    kin, vin = args[3].copy(), args[4].copy()
    return q3.op_attention(*args, form=form, **kw, **flags), kin, vin


def _check(gpu, oracle, P, **flags):
    """UNFUSED on the poisoned cache: every output and both caches equal the oracle's and the clean-cache run's; float64 bound"""
    r, kin, vin = _run(gpu, P, "UNFUSED", **flags)
    assert r["form"] == "UNFUSED"
    e = expect(oracle, P, False, kin, vin)
    assert np.array_equal(r["att"].view(np.uint32), e["att"].view(np.uint32)), (P.name, "att")
    for key in ("aq", "ad", "k_cache", "v_cache"):
        assert np.array_equal(r[key], e[key]), (P.name, key)
    c, _, _ = _run(gpu, P, "UNFUSED", poison=False, **flags)
    for key in ("att", "aq", "ad"):
        assert np.all(np.isfinite(r[key])) and np.array_equal(r[key], c[key]), (P.name, key, "differs from the clean-cache run")
    worst, rel = check_f64(P, "UNFUSED", r)
    print("F64 UNFUSED  %-16s max|y-y64|/sum(p|v|) = %.3e  (%.3f of the bound)" % (P.name, worst, rel))
    return r


def test_wide64_edges(gpu, oracle):
    """64 tokens, one per sequence, 16 / 8 heads, every batch, page and chunk edge in one launch; FUSED computes the same bits"""
    P = _wide64()
    assert P.ntok == 64 and P.one_per_seq() and sorted(set((P.slot + 1).tolist())) == EDGES
    r = _check(gpu, oracle, P)
    f, _, _ = _run(gpu, P, "FUSED")
    assert f["form"] == "FUSED"
    for key in ("aq", "ad", "k_cache", "v_cache"):
        assert np.array_equal(f[key], r[key]), (P.name, "FUSED", key)


@pytest.mark.parametrize("h,k", GQA, ids=["%d_%d" % g for g in GQA])
def test_wide_gqa(gpu, oracle, h, k):
    """16 tokens for each head layout: every q head is computed once, against its own kv head"""
    P = _gqa(h, k)
    assert P.ntok == 16
    _check(gpu, oracle, P)


def test_prefill_edges(gpu, oracle):
    """several tokens of one sequence at consecutive slots across the 64 / 128 / 256 edges: a token sees the slots at or below its own"""
    P = _prefill()
    assert not P.one_per_seq()
    _check(gpu, oracle, P, same_seq=True)
