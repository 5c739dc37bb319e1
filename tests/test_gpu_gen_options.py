"""[EXT] generation controls on the GPU (q3tts_gen_options): the talker repetition penalty and the sampled code predictor.
Op level: the frame graph's sampler launches (q3tts_op_sample_rows) against q3oracle.sample, draw for draw.  Engine level: tokens bit-exact and
PCM within the suite's RMS tolerance of the Python restatement of the oracle loop (tests/gen_loop_ref.py), graph and eager, plus the
invariants the options must not disturb (defaults inert, mixed batches, slot reuse, invalid input)."""
import itertools
import os

import numpy as np
import pytest

import gen_loop_ref
import synth_models

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)


def _rows(rng, B, n=2048):
    lg = (rng.standard_normal((B, n)) * 3).astype(np.float32)
    for b in range(B):                                   # planted ties: equal values at scattered indices, some at the top
        top = lg[b].max()
        lg[b, rng.choice(n, 5, replace=False)] = top
        lg[b, rng.choice(n, 40, replace=False)] = np.float32(0.5)
        lg[b, rng.choice(n, 3, replace=False)] = -np.inf
    return lg


CONFIGS = list(itertools.product((0.0, 0.5, 0.9, 1.3), (0, 1, 2, 50, 64, 2048), (0.5, 0.8, 1.0)))


@pytest.mark.parametrize("B", [1, 7, 64])
def test_op_sample_pred_matches_oracle_and_k_sample(gpu, oracle, B):
    rng = np.random.default_rng(100 + B)
    n_draws = 40
    for start in range(0, len(CONFIGS), B if B > 1 else 6):
        cfg = [CONFIGS[(start + b) % len(CONFIGS)] for b in range(B)]
        lg = _rows(rng, B)
        T = np.array([c[0] for c in cfg], np.float32)
        K = np.array([c[1] for c in cfg], np.int32)
        P = np.array([c[2] for c in cfg], np.float32)
        S = rng.integers(0, 2 ** 63, B).astype(np.uint64)
        pred = gpu.op_sample_rows(lg, T, K, P, S, n_draws=n_draws, kernel=1)
        talk = gpu.op_sample_rows(lg, T, K, P, S, n_draws=n_draws, kernel=0)
        assert np.array_equal(pred, talk), cfg
        for b in range(B):
            st = None
            for d in range(n_draws):
                want, st = oracle.sample(lg[b], 0, 2048, float(T[b]), int(K[b]), float(P[b]), int(S[b]), state=st)
                assert pred[d, b] == want, (cfg[b], d)
        if B == 1 and start >= 18:
            break


def test_op_talker_penalty_matches_numpy_and_oracle(gpu, oracle):
    rng = np.random.default_rng(7)
    B, n = 9, 2160
    lg = (rng.standard_normal((B, n)) * 3).astype(np.float32)
    lg[:, 10:20] = -2.5                                   # negative history logits take the multiply branch
    cfg = [(0.0, 0, 1.0, 1.3), (0.9, 50, 1.0, 1.05), (0.7, 40, 0.9, 1.5), (1.3, 0, 0.8, 0.7), (0.0, 40, 0.9, 1.0),
           (0.5, 2, 0.5, 2.0), (0.9, 0, 1.0, 1.05), (0.0, 0, 1.0, 3.0), (0.8, 64, 0.95, 1.2)]
    hist = [list(rng.integers(0, 2048, rng.integers(0, 60))) + [int(np.argmax(lg[b])), 12, 12] for b in range(B)]
    hist[4] = []
    T = np.array([c[0] for c in cfg], np.float32); K = np.array([c[1] for c in cfg], np.int32)
    P = np.array([c[2] for c in cfg], np.float32); R = np.array([c[3] for c in cfg], np.float32)
    S = np.arange(B, dtype=np.uint64) * 977 + 5
    got = gpu.op_sample_rows(lg, T, K, P, S, n_draws=20, kernel=0, penalty=R, history=hist)
    for b in range(B):
        pl = gen_loop_ref.penalise(lg[b], hist[b], R[b])
        st = None
        for d in range(20):
            want, st = oracle.sample(pl, 0, n, float(T[b]), int(K[b]), float(P[b]), int(S[b]), state=st)
            assert got[d, b] == want, (cfg[b], d)
    base = gpu.op_sample_rows(lg, T, K, P, S, n_draws=1, kernel=0)
    assert (base[0] != got[0]).any()                      # the penalty is live


@pytest.fixture(scope="module")
def tiny(gpu, oracle, tiny_model):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    a = gpu.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    pad = a.tts_pad()
    a.close()
    yield oe, pad
    oe.close()


CASES = [dict(repetition_penalty=1.3),
         dict(repetition_penalty=1.05, temperature=0.9, top_k=50, top_p=1.0),
         dict(repetition_penalty=1.05, temperature=0.9, top_k=50, top_p=1.0, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8),
         dict(predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)]


def _ref(oe, pad, prompt, steps, seed, mask_eos, **kw):
    kw = dict(kw)
    kw.setdefault("temperature", 0.0); kw.setdefault("top_k", 40); kw.setdefault("top_p", 0.9)
    codes = gen_loop_ref.generate(oe, pad, prompt, steps, seed=seed, mask_eos=mask_eos, **kw)
    return codes


def _check(oe, pad, prompt, r, steps, seed, mask_eos, kw, pcm=True):
    want = _ref(oe, pad, prompt, steps, seed, mask_eos, **kw)
    assert np.array_equal(r["codes"], want), kw
    if pcm:
        ref = gen_loop_ref.replay_pcm(oe, prompt, want)
        assert r["pcm"].size == ref.size and (ref.size == 0 or np.sqrt(np.mean((ref - r["pcm"]) ** 2)) < PCM_RMS_TOL)


@pytest.mark.parametrize("use_graph", [True, False])
def test_engine_matches_restatement(gpu, tiny, tiny_model, vivian, use_graph):
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=32, load_codec=True, use_graph=use_graph)
    rng = np.random.default_rng(31)
    prompts = [ge.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian) for n in (8, 3, 21, 12)]
    prompts[0] = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    for i, kw in enumerate(CASES):
        res = ge.generate_batch(prompts, max_steps=24, seed=[11 + i, 12, 13, 14], mask_eos=False, want_pcm=True, **kw)   # natural EOS allowed
        for j, (p, r) in enumerate(zip(prompts, res)):
            _check(oe, pad, p, r, 24, [11 + i, 12, 13, 14][j], False, kw, pcm=(j < 2))
    ge.close()


def test_engine_q5_k_m_matches_restatement(gpu, oracle, tiny_model, vivian):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q5_k_m"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    ge = gpu.Engine(tiny_model, "q5_k_m", max_batch=2, max_steps=32, load_codec=True)
    pad = ge.assets.tts_pad()
    prompt = ge.assets.build_core(np.arange(300, 311, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    kw = dict(temperature=0.9, top_k=50, top_p=1.0, **UPSTREAM)
    r = ge.generate_batch([prompt], max_steps=20, seed=3, mask_eos=False, want_pcm=True, **kw)[0]
    _check(oe, pad, prompt, r, 20, 3, False, kw)
    ge.close(); oe.close()


def test_defaults_are_inert(gpu, tiny_model, vivian):
    q3 = gpu
    ge = q3.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=True)
    prompt = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    outs = []
    for mode in ("plain", "null", "defaults"):
        for temp in (0.0, 0.7):
            r = q3.Request()
            pr = np.ascontiguousarray(prompt, np.float32)
            ge._fill(r, pr, 0, 12, temp, 40, 0.9, 42, True)
            rid = q3.C.c_int64()
            if mode == "plain":
                q3._chk(q3.lib().q3tts_submit(ge.h, q3.C.byref(r), 1, q3.C.byref(rid)))
            elif mode == "null":
                q3._chk(q3.lib().q3tts_submit_ex(ge.h, q3.C.byref(r), 1, None, q3.C.byref(rid)))
            else:
                o = q3.GenOptions()
                q3.lib().q3tts_gen_options_default(q3.C.byref(o))
                q3._chk(q3.lib().q3tts_submit_ex(ge.h, q3.C.byref(r), 1, q3.C.byref(o), q3.C.byref(rid)))
            assert ge.wait(rid.value)
            outs.append(ge.result(rid.value, want_pcm=True))
    for k in range(2, 6):
        assert np.array_equal(outs[k]["codes"], outs[k % 2]["codes"]) and np.array_equal(outs[k]["pcm"], outs[k % 2]["pcm"])
    ge.close()


def test_mixed_batch_equals_solo_runs(gpu, tiny, tiny_model, vivian):
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=8, max_steps=32, load_codec=False)
    rng = np.random.default_rng(77)
    prompts = [ge.assets.build_core(rng.integers(0, 4000, 4 + 3 * i).astype(np.int32), lang_id=2055, spk_emb=vivian) for i in range(8)]
    kws = [{}, dict(repetition_penalty=1.3), dict(predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8), {},
           dict(temperature=0.8, top_k=30, top_p=0.9, **UPSTREAM), dict(temperature=0.8, top_k=30, top_p=0.9), dict(repetition_penalty=0.7), {}]
    keys = ("temperature", "top_k", "top_p") + tuple(UPSTREAM)
    dflt = dict(temperature=0.0, top_k=40, top_p=0.9, repetition_penalty=1.0, predictor_temperature=0.0, predictor_top_k=0, predictor_top_p=1.0)
    per = {k: [kw.get(k, dflt[k]) for kw in kws] for k in keys}
    seeds = list(range(50, 58))
    batch = ge.generate_batch(prompts, max_steps=20, seed=seeds, mask_eos=False, **per)
    solo = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=32, load_codec=False)
    for i, (p, kw) in enumerate(zip(prompts, kws)):
        s = solo.generate_batch([p], max_steps=20, seed=seeds[i], mask_eos=False, **kw)[0]
        assert np.array_equal(batch[i]["codes"], s["codes"]), kw
        if not kw:   # default slots: the parent code's path, i.e. the oracle engine itself
            oc, _ = oe.generate(p, max_steps=20, temperature=0.0, seed=seeds[i], mask_eos=False)
            assert np.array_equal(batch[i]["codes"], oc)
        else:
            assert np.array_equal(batch[i]["codes"], _ref(oe, pad, p, 20, seeds[i], False, **kw)), kw
    solo.close(); ge.close()


def test_slot_reuse_reads_no_stale_history(gpu, tiny, tiny_model, vivian):
    """max_batch = 2, six penalty requests of different lengths through the scheduler: slots are reused after long requests; a stale
    history row or a stale current-frame key read at prefill would change the reused slot's tokens"""
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=True)
    rng = np.random.default_rng(5)
    specs = []
    for i, steps in enumerate((30, 6, 17, 3, 24, 11)):
        p = ge.assets.build_core(rng.integers(0, 4000, 2 + 5 * i).astype(np.int32), lang_id=2055, spk_emb=vivian)
        kw = dict(repetition_penalty=1.3 if i % 2 else 0.7)
        if i in (2, 5):
            kw.update(temperature=0.9, top_k=50, top_p=1.0, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
        specs.append((p, steps, 200 + i, kw))
    ids = [ge.submit(p, max_steps=s, seed=sd, mask_eos=(i % 3 == 0), want_pcm=(i < 3), **kw) for i, (p, s, sd, kw) in enumerate(specs)]
    while ge.sched_step():
        pass
    for i, ((p, s, sd, kw), rid) in enumerate(zip(specs, ids)):
        r = ge.result(rid, want_pcm=(i < 3))
        _check(oe, pad, p, r, s, sd, i % 3 == 0, kw, pcm=(i < 3))
    ge.close()


def test_invalid_options_are_rejected(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    prompt = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    ref = ge.generate_batch([prompt], max_steps=6)[0]["codes"]
    for bad in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
                dict(repetition_penalty=float("inf")), dict(predictor_top_k=-1), dict(predictor_top_p=0.0), dict(predictor_top_p=1.5),
                dict(predictor_temperature=0.9, predictor_top_p=float("nan"))):
        with pytest.raises(gpu.Q3Error):
            ge.submit(prompt, max_steps=6, **bad)
        with pytest.raises(gpu.Q3Error):
            ge.generate_batch([prompt, prompt], max_steps=6, **{k: [1.0 if k == "repetition_penalty" else UPSTREAM[k], v] for k, v in bad.items()})
    assert not ge.sched_step()                           # nothing was queued
    assert np.array_equal(ge.generate_batch([prompt], max_steps=6)[0]["codes"], ref)
    ge.close()


def test_ggml_mode_rejects_options(gpu, tiny_model, vivian):
    old = os.environ.get("Q3_SPEC")
    os.environ["Q3_SPEC"] = "ggml"
    try:
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    finally:
        if old is None:
            os.environ.pop("Q3_SPEC")
        else:
            os.environ["Q3_SPEC"] = old
    prompt = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.submit(prompt, max_steps=4, repetition_penalty=1.05)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.submit(prompt, max_steps=4, predictor_temperature=0.9)
    assert ge.generate_batch([prompt], max_steps=4)[0]["codes"].shape == (4, 16)
    ge.close()


def test_fullsize_upstream_options(gpu, oracle, synth_tool, vivian):
    """full-size model, 64 slots with upstream-style options: every result equals the same request through a 2-slot engine, and three
    requests x three frames equal the restatement over the full-size oracle"""
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=64, max_steps=16, load_codec=False)
    rng = np.random.default_rng(64)
    prompts = [ge.assets.build_core(rng.integers(0, 4000, 8 + (i % 5) * 7).astype(np.int32), lang_id=2055, spk_emb=vivian) for i in range(64)]
    kw = dict(temperature=0.9, top_k=50, top_p=1.0, **UPSTREAM)
    seeds = list(range(1000, 1064))
    wide = ge.generate_batch(prompts, max_steps=12, seed=seeds, mask_eos=True, **kw)
    ge.close()
    two = gpu.Engine(model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    narrow = two.generate_batch(prompts, max_steps=12, seed=seeds, mask_eos=True, **kw)
    pad = two.assets.tts_pad()
    two.close()
    for a, b in zip(wide, narrow):
        assert np.array_equal(a["codes"], b["codes"])
    oe = oracle.Engine(os.path.join(model, "gguf_q8_0"), None, 16)
    for i in (0, 1, 2):
        want = gen_loop_ref.generate(oe, pad, prompts[i], 3, seed=seeds[i], mask_eos=True, **kw)
        assert np.array_equal(wide[i]["codes"][:3], want), i
    oe.close()
