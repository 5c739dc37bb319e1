"""[EXT] KV cache type Q8_0 above the kernel, bit for bit against the oracle (oracle/q3o_model.c with the Q8_0 cache type, itself held to
float64 by tests/test_kv_q8_oracle_cpu.py) on the tiny synthetic model -- the Q8_0 twin of test_gpu_parity.py's transformer and engine
tests.  What tests/test_gpu_kv_q8.py cannot see is pinned here: Transformer::set_kv_q8 and the layer walk's routing of qrot / aq / ad into
the o-projection, the KvCacheQ8 that KvPool::view_q8 builds (unit offsets per layer and kv head), page growth in a prefill and in a
decode, a slot's pages taken over from a finished request, and the engine's frame loop with and without the captured graph.  A wiring that
is wrong but deterministic (every layer appending into layer 0's unit, say) passes every invariance test and fails here.  (-m gpu)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
WAIT_MS = 60000.0
N_PRE, N_DEC = 70, 8
WEIGHTS = [("q8_0", 2160), ("q5_k_m", 2048)]   # (weight set, logits rows compared), as test_gpu_parity.py's F16 tests


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(n, seed, n_ctx):
    """n rows and M-RoPE positions whose four streams differ from the slot and from each other (attention_cases' pos="distinct")"""
    t = np.arange(n)
    xs = (np.random.default_rng(seed).standard_normal((n, 2048)) * 0.3).astype(np.float32)
    pos = np.stack([t, t // 2 + 3, np.maximum(t - 5, 0) * 3 % n_ctx, (t * 7 + 1) % n_ctx], 1).astype(np.int32)
    return xs, pos


_expected = {}


def _oracle_rows(oracle, path, n, seed, rows, n_ctx):
    """the Q8_0 oracle's (hidden [n][2048], logits [n][rows]) of the n inputs, one token at a time; computed once per file"""
    key = (path, n, seed, rows, n_ctx)
    if key not in _expected:
        xs, pos = _inputs(n, seed, n_ctx)
        om = oracle.Model(path, n_ctx, kv_type="q8_0")
        out = [om.eval(xs[t], pos[t], 2048, 0, rows) for t in range(n)]
        om.close()
        _expected[key] = (np.stack([h for h, _ in out]), np.stack([l for _, l in out]))
    return _expected[key]


@pytest.mark.parametrize("quant,rows", WEIGHTS, ids=[q for q, _ in WEIGHTS])
def test_tf_q8_matches_oracle(gpu, oracle, tiny_model, quant, rows):
    """70 prompt rows -- the page at slot 64 is crossed inside a prefill -- whole (launches of 64 + 6 tokens) and, after clear(), cut
    10 + 60, each followed by 8 single-token decodes: hidden and logits rows equal the oracle's"""
    path = os.path.join(tiny_model, "gguf_" + quant, "qwen3_tts_talker.gguf")
    n = N_PRE + N_DEC
    xs, pos = _inputs(n, 9, 4096)
    ho, lo = _oracle_rows(oracle, path, n, 9, rows, 4096)
    gm = gpu.TfContext(path, 4096, 64, kv_type="q8_0")
    for cuts in ((N_PRE,), (10, 60)):
        got, t0 = [], 0
        for c in cuts + (1,) * N_DEC:
            got.append(gm.eval(xs[t0:t0 + c], pos[t0:t0 + c], 0, rows))
            t0 += c
        hg, lg = np.concatenate([h for h, _ in got]), np.concatenate([l for _, l in got])
        for t in range(n):
            assert np.array_equal(_bits(hg[t]), _bits(ho[t])) and np.array_equal(_bits(lg[t]), _bits(lo[t])), (quant, cuts, t)
        gm.clear()
    gm.close()


def test_tf_q8_beyond_one_chunk(gpu, oracle, tiny_model):
    """a context past 256 positions: the M / L merge of two chunks inside the layer walk, in a prefill and in two decodes"""
    path = os.path.join(tiny_model, "gguf_q8_0", "qwen3_tts_talker.gguf")
    n = 300
    xs, pos = _inputs(n + 2, 10, 4096)
    ho, _ = _oracle_rows(oracle, path, n + 2, 10, 0, 4096)
    gm = gpu.TfContext(path, 4096, 64, kv_type="q8_0")
    hg, _ = gm.eval(xs[:n], pos[:n])
    for t in (0, 63, 64, 255, 256, 257, n - 1):
        assert np.array_equal(_bits(hg[t]), _bits(ho[t])), t
    for t in (n, n + 1):
        assert np.array_equal(_bits(gm.eval(xs[t:t + 1], pos[t:t + 1])[0][0]), _bits(ho[t])), t
    gm.close()


# ---------------- engine ----------------
def _prompt(e, vivian, seed, rows):
    """a prompt of exactly `rows` rows"""
    p = e.assets.build_core(np.random.default_rng(seed).integers(0, 4000, rows).astype(np.int32), lang_id=2055, spk_emb=vivian)
    assert p.shape[0] >= rows
    return np.ascontiguousarray(p[:rows])


_codes = {}


def _oracle_codes(oracle, tiny_model, quant, p, steps):
    """the Q8_0 oracle's greedy codes; computed once per (weight set, prompt, steps)"""
    key = (quant, p.tobytes(), steps)
    if key not in _codes:
        oe = oracle.Engine(os.path.join(tiny_model, "gguf_" + quant), None, 4, kv_type="q8_0")
        _codes[key] = oe.generate(p, max_steps=steps, mask_eos=True)[0]
        oe.close()
    return _codes[key]


def _run(e, prompts, steps):
    rids = [e.submit(p, max_steps=steps, mask_eos=True) for p in prompts]
    out = []
    for r in rids:
        assert e.wait(r, WAIT_MS)
        out.append(e.result(r)["codes"])
    return out


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
def test_engine_q8_matches_oracle(gpu, oracle, tiny_model, vivian, quant, use_graph):
    """one greedy request whose decode crosses slot 64 (40 prompt rows, 40 frames), then four ragged prompts beside each other (one of
    them crossing slot 64 in its prefill): every request's codes equal the oracle's run of it alone"""
    e = gpu.Engine(tiny_model, quant, max_batch=4, max_steps=40, load_codec=False, use_graph=use_graph, kv_type="q8_0")
    try:
        p = _prompt(e, vivian, 70, 40)
        want = _oracle_codes(oracle, tiny_model, quant, p, 40)
        assert want.shape == (40, 16)
        assert np.array_equal(_run(e, [p], 40)[0], want), (quant, use_graph, "single")
        ps = [_prompt(e, vivian, 71 + i, n) for i, n in enumerate((9, 70, 23, 58))]
        for i, (p, got) in enumerate(zip(ps, _run(e, ps, 10))):
            assert np.array_equal(got, _oracle_codes(oracle, tiny_model, quant, p, 10)), (quant, use_graph, "batch", i)
    finally:
        e.close()


def test_engine_q8_slot_and_pages_reused(gpu, oracle, tiny_model, vivian):
    """one slot: a 130-row request (three pages) finishes, then a 9-row request takes the slot and its pages, whose tail holds the first
    request's quants and scales: both equal the oracle"""
    e = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False, kv_type="q8_0")
    try:
        for seed, rows in ((80, 130), (81, 9)):
            p = _prompt(e, vivian, seed, rows)
            assert np.array_equal(_run(e, [p], 6)[0], _oracle_codes(oracle, tiny_model, "q8_0", p, 6)), rows
    finally:
        e.close()
