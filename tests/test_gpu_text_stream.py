"""[EXT] streaming-text talker input on the GPU (q3tts_submit_trailing, q3tts_submit_text_streaming, q3tts_generate_batch_trailing,
q3tts_group_submit_text_streaming): tokens bit-exact and PCM within the suite's RMS tolerance of the Python restatement
(tests/text_stream_ref.py), graph and eager, Q8_0 and Q5_K_M, greedy and sampled, with and without the generation options; plus the
invariants the mode must not disturb (n_trail = 0, mixed batches, staggered admission, slot reuse, invalid input, a group)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import synth_models
import text_stream_ref

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
TEXT_EOS = 151673
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLING = [dict(), dict(temperature=0.9, top_k=50, top_p=1.0), dict(temperature=0.9, top_k=50, top_p=1.0, **UPSTREAM)]


@pytest.fixture(scope="module")
def tiny(gpu, oracle, tiny_model):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    a = gpu.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    pad = a.tts_pad()
    a.close()
    yield oe, pad
    oe.close()


def _ref(oe, pad, prompt, steps, trail, seed, mask_eos, **kw):
    kw = dict(kw)
    kw.setdefault("temperature", 0.0); kw.setdefault("top_k", 40); kw.setdefault("top_p", 0.9)
    return text_stream_ref.generate(oe, pad, prompt, steps, trail, seed=seed, mask_eos=mask_eos, **kw)


def _check(oe, pad, prompt, r, steps, trail, seed, mask_eos, kw, pcm=True):
    want = _ref(oe, pad, prompt, steps, trail, seed, mask_eos, **kw)
    assert np.array_equal(r["codes"], want), (len(trail), kw)
    if pcm:
        import gen_loop_ref
        ref = gen_loop_ref.replay_pcm(oe, prompt, want)
        assert r["pcm"].size == ref.size and (ref.size == 0 or np.sqrt(np.mean((ref - r["pcm"]) ** 2)) < PCM_RMS_TOL)


def _cases(assets, vivian):
    """(prompt, trail, steps, mask_eos): trail ending mid 4-frame group, trail longer than the run, an out-of-range id, n_trail = 0"""
    rng = np.random.default_rng(12)
    out = []
    p, t = assets.prompt_build_streaming(rng.integers(0, 4000, 6).astype(np.int32), lang_id=2055, spk_emb=vivian)
    out.append((p, t, 20, True))                                      # 6 ids: frames 0..5, the last one mid group 2
    p, t = assets.prompt_build_streaming(rng.integers(0, 4000, 30).astype(np.int32), lang_id=2055, spk_emb=vivian)
    out.append((p, t, 10, True))                                      # 30 ids, 10 frames
    p, t = assets.prompt_build_streaming(np.array([120, 5000, 77, -3, 9], np.int32), lang_id=2055, spk_emb=vivian)
    out.append((p, t, 14, False))                                     # 5000, -3 and TEXT_EOS: the fallback row, natural EOS allowed
    p = assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    out.append((p, np.zeros(0, np.int32), 12, True))                  # n_trail = 0 beside streaming slots
    return out


@pytest.mark.parametrize("use_graph", [True, False])
def test_engine_matches_restatement(gpu, tiny, tiny_model, vivian, use_graph):
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=32, load_codec=True, use_graph=use_graph)
    cases = _cases(ge.assets, vivian)
    for i, kw in enumerate(SAMPLING):
        seeds = [21 + i, 22, 23, 24]
        res = ge.generate_batch([c[0] for c in cases], max_steps=[c[2] for c in cases], seed=seeds, mask_eos=[c[3] for c in cases],
                                want_pcm=True, trailing_ids=[c[1] for c in cases], **kw)
        for j, (c, r) in enumerate(zip(cases, res)):
            _check(oe, pad, c[0], r, c[2], c[1], seeds[j], c[3], kw, pcm=(j < 2 and i != 1))
    ge.close()


def test_engine_q5_k_m_matches_restatement(gpu, oracle, tiny_model, vivian):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q5_k_m"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    ge = gpu.Engine(tiny_model, "q5_k_m", max_batch=2, max_steps=32, load_codec=True)
    pad = ge.assets.tts_pad()
    prompt, trail = ge.assets.prompt_build_streaming(np.arange(300, 311, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    for kw in (dict(), SAMPLING[2]):
        r = ge.generate_batch([prompt], max_steps=18, seed=3, mask_eos=True, want_pcm=True, trailing_ids=[trail], **kw)[0]
        _check(oe, pad, prompt, r, 18, trail, 3, True, kw)
    ge.close(); oe.close()


def test_zero_trail_is_plain_submit(gpu, tiny_model, vivian):
    q3 = gpu
    ge = q3.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=True)
    prompt = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    for temp in (0.0, 0.7):
        a = ge.submit(prompt, max_steps=12, temperature=temp, seed=5, want_pcm=True)
        assert ge.wait(a)
        ra = ge.result(a, want_pcm=True)
        b = ge.submit(prompt, max_steps=12, temperature=temp, seed=5, want_pcm=True, trailing_ids=[])
        assert ge.wait(b)
        rb = ge.result(b, want_pcm=True)
        assert np.array_equal(ra["codes"], rb["codes"]) and np.array_equal(ra["pcm"], rb["pcm"])
    ge.close()


def test_mixed_batch_and_staggered_admission(gpu, tiny, tiny_model, vivian):
    """plain requests beside streaming ones equal their solo runs; the second half is submitted while the first half runs under the
    scheduler thread, so it is admitted through the asynchronous prefill"""
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=8, max_steps=40, load_codec=False)
    rng = np.random.default_rng(77)
    reqs = []
    for i in range(8):
        text = rng.integers(0, 4000, 3 + 2 * i).astype(np.int32)
        if i % 2:
            p, t = ge.assets.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian)
        else:
            p, t = ge.assets.build_core(text, lang_id=2055, spk_emb=vivian), None
        reqs.append((p, t, dict(temperature=0.8, top_k=30, top_p=0.9) if i % 3 == 0 else {}))
    ge.sched_start()
    try:
        ids = [ge.submit(p, max_steps=30, seed=60 + i, mask_eos=True, trailing_ids=t, **kw) for i, (p, t, kw) in enumerate(reqs[:4])]
        while ge.poll(ids[0])["n_frames"] < 4:
            time.sleep(0.002)
        ids += [ge.submit(p, max_steps=30, seed=64 + i, mask_eos=True, trailing_ids=t, **kw) for i, (p, t, kw) in enumerate(reqs[4:])]
        for rid in ids:
            assert ge.wait(rid)
        res = [ge.result(rid) for rid in ids]
    finally:
        ge.sched_stop()
    ge.close()
    solo = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=40, load_codec=False)
    for i, ((p, t, kw), r) in enumerate(zip(reqs, res)):
        if t is None:
            s = solo.generate_batch([p], max_steps=30, seed=60 + i, mask_eos=True, **kw)[0]
            assert np.array_equal(r["codes"], s["codes"]), i
        else:
            assert np.array_equal(r["codes"], _ref(oe, pad, p, 30, t, 60 + i, True, **kw)), i
    solo.close()


def test_slot_reuse_alternating_modes(gpu, tiny, tiny_model, vivian):
    """max_batch = 2, modes alternate through reused slots: a stale trailing count or id row would change the reused slot's tokens"""
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=True)
    rng = np.random.default_rng(5)
    specs = []
    for i, steps in enumerate((26, 6, 17, 3, 22, 11)):
        text = rng.integers(0, 4000, 4 + 5 * i).astype(np.int32)
        if i % 2 == 0:
            p, t = ge.assets.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian)
        else:
            p, t = ge.assets.build_core(text, lang_id=2055, spk_emb=vivian), np.zeros(0, np.int32)
        specs.append((p, t, steps, 200 + i))
    ids = [ge.submit(p, max_steps=s, seed=sd, mask_eos=True, want_pcm=(i < 2), trailing_ids=t if t.size else None)
           for i, (p, t, s, sd) in enumerate(specs)]
    while ge.sched_step():
        pass
    for i, ((p, t, s, sd), rid) in enumerate(zip(specs, ids)):
        _check(oe, pad, p, ge.result(rid, want_pcm=(i < 2)), s, t, sd, True, {}, pcm=(i < 2))
    ge.close()


def test_submit_text_streaming_equals_submit_trailing(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=False)
    rng = np.random.default_rng(9)
    preset = ge.register_voice(vivian)
    ref_codes = rng.integers(0, 2048, (4, 16)).astype(np.int32)
    ref_text = rng.integers(0, 4000, 3).astype(np.int32)
    clone = ge.register_voice(vivian, ref_codes, ref_text)
    text = rng.integers(0, 4000, 7).astype(np.int32)
    for vid, extra in ((preset, {}), (clone, dict(ref_codes=ref_codes, ref_text_ids=ref_text))):
        a = ge.submit_text(vid, text, max_steps=16, temperature=0.7, seed=8, streaming_text=True)
        assert ge.wait(a)
        ra = ge.result(a)
        p, t = ge.assets.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian, **extra)
        b = ge.submit(p, max_steps=16, temperature=0.7, seed=8, trailing_ids=t)
        assert ge.wait(b)
        rb = ge.result(b)
        c = ge.submit_text(vid, text, max_steps=16, temperature=0.7, seed=8)
        assert ge.wait(c)
        rc = ge.result(c)
        assert np.array_equal(ra["codes"], rb["codes"]) and ra["codes"].shape[0] > 0
        assert not np.array_equal(ra["codes"], rc["codes"])             # the layout is live
    ge.close()


def test_invalid_input_is_rejected(gpu, tiny_model, vivian):
    q3 = gpu
    ge = q3.Engine(tiny_model, "q8_0", max_batch=2, max_prompt=64, max_steps=16, load_codec=False)
    prompt = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    ref = ge.generate_batch([prompt], max_steps=6)[0]["codes"]
    with pytest.raises(q3.Q3Error, match="n_trail"):
        ge.submit(prompt, max_steps=6, trailing_ids=np.arange(65, dtype=np.int32))
    with pytest.raises(q3.Q3Error, match="n_trail"):
        ge.generate_batch([prompt, prompt], max_steps=6, trailing_ids=[[1, 2], np.arange(65, dtype=np.int32)])
    r = q3.Request()
    pr = np.ascontiguousarray(prompt, np.float32)
    ge._fill(r, pr, 0, 6, 0.0, 40, 0.9, 42, True)
    rid = C.c_int64()
    for ids, n in ((None, 3), (None, -1), (np.arange(3, dtype=np.int32), -1)):
        assert q3.lib().q3tts_submit_trailing(ge.h, C.byref(r), 0, None, q3._p(ids), n, C.byref(rid)) != 0
    vid = ge.register_voice(vivian)
    with pytest.raises(q3.Q3Error, match="n_text >= 1"):
        ge.submit_text(vid, np.zeros(0, np.int32), max_steps=6, streaming_text=True)
    assert not ge.sched_step()                                         # nothing was queued
    assert np.array_equal(ge.generate_batch([prompt], max_steps=6)[0]["codes"], ref)
    ge.close()


def test_ggml_mode_rejects_trailing_ids(gpu, tiny_model, vivian):
    old = os.environ.get("Q3_SPEC")
    os.environ["Q3_SPEC"] = "ggml"
    try:
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    finally:
        if old is None:
            os.environ.pop("Q3_SPEC")
        else:
            os.environ["Q3_SPEC"] = old
    prompt, trail = ge.assets.prompt_build_streaming(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.submit(prompt, max_steps=4, trailing_ids=trail)
    vid = ge.register_voice(vivian)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.submit_text(vid, np.arange(100, 108, dtype=np.int32), max_steps=4, streaming_text=True)
    assert not ge.sched_step()
    assert ge.generate_batch([prompt], max_steps=4)[0]["codes"].shape == (4, 16)
    ge.close()


def test_group_of_one_device(gpu, tiny_model, vivian):
    q3 = gpu
    L = q3.lib()
    p = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    md, qn = tiny_model.encode(), b"q8_0"
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = md, qn, 2, 24, 0
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_voice_register.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_poll.argtypes = [C.c_void_p, C.c_int64, C.POINTER(q3.ReqStatus)]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs = np.zeros(1, np.int32)
    g = C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(p), q3._p(devs), 1, C.byref(g)))
    try:
        spk = np.ascontiguousarray(vivian, np.float32)
        vid = C.c_int32()
        q3._chk(L.q3tts_group_voice_register(g, q3._p(spk), None, 0, None, 0, C.byref(vid)))
        text = np.arange(200, 209, dtype=np.int32)
        sc = q3.SamplerConfig(0.7, 40, 0.9, 1, 17)
        rid = C.c_int64()
        q3._chk(L.q3tts_group_submit_text_streaming(g, vid.value, q3._p(text), text.size, 2055, None, 0, C.byref(sc), 14, 1, 0, None, C.byref(rid)))
        assert L.q3tts_group_wait(g, rid.value, -1.0) == 0
        codes = np.zeros(14 * 16, np.int32)
        gf, gp = C.c_int32(), C.c_int64()
        q3._chk(L.q3tts_group_fetch(g, rid.value, q3._p(codes), 0, 14, None, 0, 0, C.byref(gf), C.byref(gp)))
        q3._chk(L.q3tts_group_release(g, rid.value))
    finally:
        L.q3tts_group_destroy(g)
    ge = q3.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=False)
    v = ge.register_voice(vivian)
    e = ge.submit_text(v, text, max_steps=14, temperature=0.7, top_k=40, top_p=0.9, seed=17, streaming_text=True)
    assert ge.wait(e)
    want = ge.result(e)["codes"]
    ge.close()
    assert gf.value == 14 and np.array_equal(codes.reshape(14, 16), want)


def test_fullsize_streaming(gpu, oracle, synth_tool, vivian):
    """full-size model, 64 streaming requests with varied n_trail through 64 slots: every result equals the same request through a 2-slot
    engine, and three requests x three frames equal the restatement over the full-size oracle"""
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=64, max_steps=16, load_codec=False)
    rng = np.random.default_rng(64)
    built = [ge.assets.prompt_build_streaming(rng.integers(0, 4000, 1 + (i % 9) * 3).astype(np.int32), lang_id=2055, spk_emb=vivian)
             for i in range(64)]
    prompts, trails = [b[0] for b in built], [b[1] for b in built]
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    seeds = list(range(2000, 2064))
    wide = ge.generate_batch(prompts, max_steps=12, seed=seeds, mask_eos=True, trailing_ids=trails, **kw)
    ge.close()
    two = gpu.Engine(model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    narrow = two.generate_batch(prompts, max_steps=12, seed=seeds, mask_eos=True, trailing_ids=trails, **kw)
    pad = two.assets.tts_pad()
    two.close()
    for a, b in zip(wide, narrow):
        assert np.array_equal(a["codes"], b["codes"])
    oe = oracle.Engine(os.path.join(model, "gguf_q8_0"), None, 16)
    for i in (0, 1, 5):
        want = _ref(oe, pad, prompts[i], 3, trails[i], seeds[i], True, **kw)
        assert np.array_equal(wide[i]["codes"][:3], want), i
    oe.close()
