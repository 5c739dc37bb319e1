"""[EXT] KV cache type Q8_0 through the engine (q3tts_engine_create_kv, Engine(kv_type="q8_0")) on the tiny synthetic model: a request's
codes depend on its prompt, seed and options alone -- not on what runs beside it, on how its prefill wave was shared, or on whether its
pages came from a fork (k_kv_fork), a stem store (k_kv_stem) or its own prefill -- and resume continues the straight run.  The F16 type is
the plain engine.  These are invariances; the values themselves are pinned to the oracle bit for bit in tests/test_gpu_kv_q8_parity.py and,
here, in test_both_types_side_by_side.  No threshold on Q8_0-against-F16 agreement: it is a quantisation effect and is only printed.  (-m gpu)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
WAIT_MS = 60000.0
STEPS = 12


@pytest.fixture(scope="module")
def q8(gpu, tiny_model):
    e = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=40, load_codec=False, kv_type="q8_0")
    yield e
    e.close()


def prompt(e, vivian, seed, n=8):
    rng = np.random.default_rng(seed)
    return e.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


def codes(e, rids):
    out = []
    for r in rids:
        assert e.wait(r, WAIT_MS)
        out.append(e.result(r)["codes"])
    return out


def run(e, p, seed, **kw):
    return codes(e, [e.submit(p, max_steps=STEPS, seed=seed, mask_eos=True, **SAMPLED, **kw)])[0]


def test_alone_and_beside_three(q8, vivian):
    ps = [prompt(q8, vivian, 10 + i, 6 + 3 * i) for i in range(4)]
    alone = run(q8, ps[0], 500)
    assert alone.shape == (STEPS, 16)
    together = codes(q8, [q8.submit(p, max_steps=STEPS, seed=500 + i, mask_eos=True, **SAMPLED) for i, p in enumerate(ps)])
    assert np.array_equal(together[0], alone)


def test_prefill_wave_shared_or_solo(q8, vivian):
    """130 rows: three KV pages, and a prefill chunk beside other prompts' rows or alone"""
    long = prompt(q8, vivian, 20, 140)[:130]
    assert long.shape[0] == 130
    solo = run(q8, long, 600)
    shared = codes(q8, [q8.submit(p, max_steps=STEPS, seed=600 + i, mask_eos=True, **SAMPLED)
                        for i, p in enumerate([long, prompt(q8, vivian, 21, 9), prompt(q8, vivian, 22, 70)])])
    assert np.array_equal(shared[0], solo)


def test_candidates_fork_q8_pages(q8, vivian):
    p = prompt(q8, vivian, 30, 75)                                       # two pages to fork
    seeds = [701, 702, 703]
    got = codes(q8, q8.submit_candidates(p, seeds, max_steps=STEPS, mask_eos=True, **SAMPLED))
    for s, c in zip(seeds, got):
        assert np.array_equal(c, run(q8, p, s)), s
    assert not np.array_equal(got[0], got[1])


def test_stem_restore_q8_pages(q8, vivian):
    p = prompt(q8, vivian, 40, 90)
    want = run(q8, p, 800)
    sid = q8.stem_create(p[:70])                                         # two store pages, the second partly stale
    assert q8.stem_wait(sid, WAIT_MS)
    before = q8.stem_stats()["restores"]
    q8.set_stem(sid)
    got = run(q8, p, 800)
    q8.set_stem(None)
    q8.stem_release(sid)
    assert q8.stem_stats()["restores"] == before + 1 and np.array_equal(got, want)


def test_resume_at_5(q8, vivian):
    p = prompt(q8, vivian, 50, 12)
    want = run(q8, p, 900)
    assert np.array_equal(run(q8, p, 900, prefix_codes=want[:5]), want)


def test_both_types_side_by_side(gpu, oracle, q8, tiny_model, vivian):
    """an F16 engine beside the Q8_0 one: each equals the oracle with its cache type (the decode crosses slot 64); F16 through create_kv
    is the plain engine, bit for bit"""
    f16 = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=40, load_codec=False, kv_type="f16")
    plain = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=40, load_codec=False)
    p = prompt(q8, vivian, 60, 40)
    a, b, c = (codes(e, [e.submit(p, max_steps=32, seed=1, mask_eos=True)])[0] for e in (q8, f16, plain))
    assert a.shape == b.shape == (32, 16) and np.array_equal(b, c)
    for got, kv_type in ((a, "q8_0"), (b, "f16")):
        oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), None, 4, kv_type=kv_type)
        want, _ = oe.generate(p, max_steps=32, mask_eos=True)
        oe.close()
        assert np.array_equal(got, want), kv_type
    print("greedy code_0 equal in %d of 32 frames between the Q8_0 and the F16 cache" % int((a[:, 0] == b[:, 0]).sum()))
    f16.close()
    plain.close()


def test_unknown_type_refused(gpu, tiny_model):
    with pytest.raises(gpu.Q3Error, match="unknown KV cache type"):
        gpu.Engine(tiny_model, "q8_0", load_codec=False, kv_type=2)


def test_tf_open_kv(gpu, tiny_model, monkeypatch):
    """q3tts_tf_open_kv: a Q8_0 context gives the same hidden rows however the 70 tokens are cut into calls and chunks, the F16 type is
    q3tts_tf_open bit for bit, and a Q3_SPEC=ggml model refuses the type by name"""
    path = os.path.join(tiny_model, "gguf_q8_0", "qwen3_tts_talker.gguf")
    q, f, plain = (gpu.TfContext(path, n_ctx=256, max_tok=64, kv_type=t) for t in ("q8_0", "f16", None))
    x = np.random.default_rng(5).standard_normal((70, q.n_embd)).astype(np.float32)
    pos = np.stack([np.arange(70)] * 3 + [np.zeros(70, np.int64)], 1).astype(np.int32)
    whole = q.eval(x, pos)[0]                                            # chunks of 64 + 6 tokens
    q.clear()
    parts = np.concatenate([q.eval(x[:10], pos[:10])[0], q.eval(x[10:], pos[10:])[0]])
    assert np.all(np.isfinite(whole)) and np.array_equal(whole, parts)
    hf = f.eval(x, pos)[0]
    assert np.array_equal(hf, plain.eval(x, pos)[0]) and not np.array_equal(hf, whole)
    for c in (q, f, plain):
        c.close()
    monkeypatch.setenv("Q3_SPEC", "ggml")
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml has no KV cache type Q8_0"):
        gpu.TfContext(path, n_ctx=256, max_tok=64, kv_type="q8_0")
