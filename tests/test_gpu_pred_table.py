"""The code predictor's layer-0 q/k/v table (q3tts_pred_table_bytes): for predictor passes 1..14 the engine builds layer 0's attention norm +
q/k/v projection of every projected codec row once at creation, and the frame reads rows of it.  An engine with the table and one created
under Q3_PRED_L0_TABLE=0 live side by side here and must emit the same codes and the same recorded log-probabilities, bit for bit: one slot
(the fused path, one token), 3 requests on 4 slots (the fused path), 12 on 12 (the batched path: short attention, workgroup norm), greedy and
with a sampled predictor; the K-quant and the float files at one width each.  (-m gpu)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAIT_MS = 120000.0
FRAMES = 6
WIDTHS = [("q8_0", 1, 1), ("q8_0", 4, 3), ("q8_0", 12, 12), ("q5_k_m", 4, 3), ("bf16", 12, 12)]


def _engine(gpu, monkeypatch, model, quant, max_batch, table):
    if table:
        monkeypatch.delenv("Q3_PRED_L0_TABLE", raising=False)
    else:
        monkeypatch.setenv("Q3_PRED_L0_TABLE", "0")
    return gpu.Engine(model, quant, max_batch=max_batch, max_steps=8, load_codec=False)


def _prompts(ge, vivian, n):
    rng = np.random.default_rng(1400 + n)
    return [ge.assets.build_core(rng.integers(0, 4000, 3 + i % 11).astype(np.int32), lang_id=2055, spk_emb=vivian) for i in range(n)]


def _recorded(ge, prompts, **kw):
    """every prompt through the scheduler at once, recording: [(codes, logprobs)]"""
    ge.set_logprobs(True)
    rids = [ge.submit(p, max_steps=FRAMES, seed=300 + i, mask_eos=True, **kw) for i, p in enumerate(prompts)]
    out = []
    for rid in rids:
        assert ge.wait(rid, WAIT_MS)
        r = ge.result(rid)
        out.append((r["codes"], r["logprobs"]))
    ge.set_logprobs(False)
    return out


@pytest.mark.parametrize("quant,max_batch,n", WIDTHS, ids=["%s-b%d-n%d" % w for w in WIDTHS])
def test_table_on_equals_table_off(gpu, tiny_model, vivian, monkeypatch, quant, max_batch, n):
    on = _engine(gpu, monkeypatch, tiny_model, quant, max_batch, True)
    off = _engine(gpu, monkeypatch, tiny_model, quant, max_batch, False)
    try:
        assert on.pred_table_bytes() > 0 and off.pred_table_bytes() == 0
        prompts = _prompts(on, vivian, n)
        seeds = list(range(40, 40 + n))
        for kw in (dict(), dict(predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.95)):
            a = on.generate_batch(prompts, max_steps=FRAMES, seed=seeds, mask_eos=True, **kw)
            b = off.generate_batch(prompts, max_steps=FRAMES, seed=seeds, mask_eos=True, **kw)
            for i, (x, y) in enumerate(zip(a, b)):
                assert x["codes"].shape == (FRAMES, 16) and np.array_equal(x["codes"], y["codes"]), (quant, max_batch, i, kw)
            ra, rb = _recorded(on, prompts, **kw), _recorded(off, prompts, **kw)
            for i, ((ca, la), (cb, lb)) in enumerate(zip(ra, rb)):
                assert ca.shape == (FRAMES, 16) and np.array_equal(ca, cb), (quant, max_batch, i, kw, "recording")
                assert la.shape == (FRAMES, 17) and np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (quant, max_batch, i, kw, "log-probabilities")
                if not kw:   # greedy: recording changes no code
                    assert np.array_equal(ca, a[i]["codes"]), (quant, max_batch, i)
    finally:
        on.close()
        off.close()


def test_ggml_mode_builds_no_table(gpu, tiny_model, monkeypatch):
    monkeypatch.delenv("Q3_PRED_L0_TABLE", raising=False)
    monkeypatch.setenv("Q3_SPEC", "ggml")
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    try:
        assert ge.pred_table_bytes() == 0
    finally:
        ge.close()
