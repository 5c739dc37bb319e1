"""[EXT] live text append on the GPU (q3tts_submit_trailing_open, q3tts_trail_append, q3tts_trail_progress, q3tts_submit_text_streaming_open,
q3tts_text_append and the q3tts_group_* forms): a request whose trail is appended in pieces, with any number of waited frames, gives the
codes (bit-exact) and PCM (within the suite's RMS tolerance) of the same request submitted closed, and of tests/text_stream_ref.py.  Waiting
slots cost no frame group when they are alone, and leave what shares the batch with them untouched."""
import ctypes as C
import os
import threading
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


def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((a - b) ** 2)))


def _ref(oe, pad, prompt, steps, trail, seed, **kw):
    kw = dict(kw)
    kw.setdefault("temperature", 0.0); kw.setdefault("top_k", 40); kw.setdefault("top_p", 0.9)
    return text_stream_ref.generate(oe, pad, prompt, steps, trail, seed=seed, mask_eos=True, **kw)


def _closed(ge, prompt, trail, steps, seed, kw, want_pcm=False):
    rid = ge.submit(prompt, max_steps=steps, seed=seed, mask_eos=True, want_pcm=want_pcm, trailing_ids=trail, **kw)
    assert ge.wait(rid)
    return ge.result(rid, want_pcm=want_pcm)


def _stalled_run(ge, prompt, trail, k, steps, seed, kw, want_pcm=False):
    """open with trail[:k], step by hand until the slot waits, check that it stays put, then append the rest and close"""
    rid = ge.submit(prompt, max_steps=steps, seed=seed, mask_eos=True, want_pcm=want_pcm, trailing_ids=trail[:k], open_trail=True, **kw)
    for _ in range(64):
        ge.sched_step()
        if ge.poll(rid)["n_frames"] >= k:
            break
    assert ge.poll(rid)["n_frames"] == k
    g0 = ge.stats()["graph_frames"]
    for _ in range(4):
        assert ge.sched_step()                                          # busy, but no frame group runs
    assert ge.poll(rid)["n_frames"] == k and ge.stats()["graph_frames"] == g0
    assert ge.trail_progress(rid) == (k, k, False)
    mid = (k + len(trail)) // 2                                        # two more pieces, the second one closes
    assert ge.trail_append(rid, trail[k:mid]) == 0
    assert ge.trail_append(rid, trail[mid:], close=True) == 0
    assert ge.trail_progress(rid)[0::2] == (len(trail), True)
    while ge.sched_step():
        pass
    return ge.result(rid, want_pcm=want_pcm)


@pytest.fixture(scope="module")
def tiny(gpu, oracle, tiny_model):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    a = gpu.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    pad = a.tts_pad()
    a.close()
    yield oe, pad
    oe.close()


@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_deterministic_stalls(gpu, tiny, tiny_model, vivian, quant, use_graph):
    """k = 0, 1, 5, 6 ids at submit: 5 and 6 make the slot wait in the middle of a 4-frame group"""
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, quant, max_batch=2, max_steps=24, load_codec=True, use_graph=use_graph)
    prompt, trail = ge.assets.prompt_build_streaming(np.arange(300, 310, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    assert len(trail) == 10
    steps = 14
    for i, kw in enumerate(SAMPLING):
        seed = 40 + i
        pcm = i == 0
        want = _closed(ge, prompt, trail, steps, seed, kw, want_pcm=pcm)
        if quant == "q8_0" and use_graph:
            assert np.array_equal(want["codes"], _ref(oe, pad, prompt, steps, trail, seed, **kw)), kw
        for k in (0, 1, 5, 6):
            got = _stalled_run(ge, prompt, trail, k, steps, seed, kw, want_pcm=pcm)
            assert np.array_equal(got["codes"], want["codes"]), (k, kw)
            if pcm:
                assert got["pcm"].size == want["pcm"].size and _rms(got["pcm"], want["pcm"]) < PCM_RMS_TOL
    ge.close()


def test_stalls_inside_a_mixed_batch(gpu, tiny_model, vivian):
    """open requests wait while plain, closed-trail and option-carrying requests run beside them; the second wave is admitted through
    the asynchronous prefill while the first one runs.  Every request equals its solo / closed result"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=8, max_steps=40, load_codec=False)
    rng = np.random.default_rng(31)
    specs = []   # (prompt, trail or None, open?, kw)
    for i in range(8):
        text = rng.integers(0, 4000, 4 + 2 * i).astype(np.int32)
        kind = i % 4
        if kind == 0:
            p, t = ge.assets.build_core(text, lang_id=2055, spk_emb=vivian), None
        else:
            p, t = ge.assets.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian)
        kw = [dict(), dict(temperature=0.8, top_k=30, top_p=0.9), SAMPLING[2], dict()][(i // 2) % 4] if kind != 1 else dict(**UPSTREAM)
        specs.append((p, t, kind >= 2, kw))
    ge.sched_start()
    ids, feeds = [], []
    try:
        def sub(i):
            p, t, op, kw = specs[i]
            rid = ge.submit(p, max_steps=30, seed=90 + i, mask_eos=True, trailing_ids=(t[:2] if op else t), open_trail=op, **kw)
            ids.append(rid)
            if op:
                feeds.append((rid, t))
        for i in range(4):
            sub(i)
        while ge.poll(ids[0])["n_frames"] < 6:
            time.sleep(0.002)
        for i in range(4, 8):
            sub(i)
        time.sleep(0.05)
        for rid, t in feeds[:2]:                                        # the first wave's open requests wait at frame 2 by now
            assert ge.poll(rid)["n_frames"] == 2 and ge.trail_progress(rid) == (2, 2, False)
        for rid, t in feeds:
            assert ge.trail_append(rid, t[2:5]) == 0
        time.sleep(0.03)
        for rid, t in feeds:
            assert ge.trail_append(rid, t[5:], close=True) == 0
        for rid in ids:
            assert ge.wait(rid, 60000)
        res = [ge.result(rid) for rid in ids]
    finally:
        ge.sched_stop()
    ge.close()
    solo = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=40, load_codec=False)
    for i, ((p, t, op, kw), r) in enumerate(zip(specs, res)):
        s = solo.generate_batch([p], max_steps=30, seed=90 + i, mask_eos=True, trailing_ids=[t], **kw)[0]
        assert r["codes"].shape == (30, 16) and np.array_equal(r["codes"], s["codes"]), i
    solo.close()


def _feeder(append, streams, seed, lock_errors, max_sleep=0.006):
    """appends each stream's remaining ids in pieces of 1-5 at random intervals, streams interleaved; the last piece closes"""
    rng = np.random.default_rng(seed)
    pos = [1] * len(streams)
    try:
        while any(p < len(s[1]) for p, s in zip(pos, streams)):
            i = int(rng.integers(0, len(streams)))
            rid, ids = streams[i]
            if pos[i] >= len(ids):
                continue
            n = int(rng.integers(1, 6))
            piece = ids[pos[i]:pos[i] + n]
            pos[i] += len(piece)
            assert append(rid, piece, pos[i] >= len(ids)) == 0
            time.sleep(float(rng.uniform(0.0, max_sleep)))
    except Exception as ex:   # surfaced by the test thread
        lock_errors.append(ex)


def test_randomised_feeder_text_level(gpu, tiny_model, vivian):
    """8 text-level streams (preset and clone voices) through 4 slots, fed by a seeded thread while the driver runs; some wait in the
    queue while they are fed.  Each equals q3tts_submit_text_streaming of its whole text"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=40, load_codec=True)
    rng = np.random.default_rng(8)
    preset = ge.register_voice(vivian)
    clone = ge.register_voice(vivian, rng.integers(0, 2048, (4, 16)).astype(np.int32), rng.integers(0, 4000, 3).astype(np.int32))
    texts = [rng.integers(0, 4000, int(rng.integers(6, 20))).astype(np.int32) for _ in range(8)]
    kws = [SAMPLING[i % 3] for i in range(8)]
    vids = [preset if i % 2 == 0 else clone for i in range(8)]
    want = []
    for i in range(8):
        rid = ge.submit_text(vids[i], texts[i], max_steps=24, seed=500 + i, want_pcm=(i < 2), streaming_text=True, **kws[i])
        assert ge.wait(rid)
        want.append(ge.result(rid, want_pcm=(i < 2)))
    ge.sched_start()
    errors = []
    try:
        ids = [ge.submit_text(vids[i], texts[i][:1], max_steps=24, seed=500 + i, want_pcm=(i < 2), streaming_text=True, open_text=True,
                              **kws[i]) for i in range(8)]
        th = threading.Thread(target=_feeder, args=(lambda rid, ids_, last: ge.text_append(rid, ids_, is_last=last),
                                                     list(zip(ids, texts)), 1234, errors))
        th.start()
        th.join()
        assert not errors, errors
        for rid in ids:
            assert ge.wait(rid, 60000)
        got = [ge.result(rid, want_pcm=(i < 2)) for i, rid in enumerate(ids)]
    finally:
        ge.sched_stop()
    ge.close()
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["codes"], w["codes"]) and g["codes"].shape == (24, 16), i
        if i < 2:
            assert g["pcm"].size == w["pcm"].size and _rms(g["pcm"], w["pcm"]) < PCM_RMS_TOL


def test_text_level_equivalences(gpu, tiny, tiny_model, vivian):
    oe, pad = tiny
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=False)
    vid = ge.register_voice(vivian)
    text = np.arange(700, 709, dtype=np.int32)
    for k in (1, 4, 9):
        kw = SAMPLING[k % 3]
        a = ge.submit_text(vid, text, max_steps=16, seed=8, streaming_text=True, **kw)
        assert ge.wait(a)
        ra = ge.result(a)
        b = ge.submit_text(vid, text[:k], max_steps=16, seed=8, streaming_text=True, open_text=True, **kw)
        assert ge.trail_progress(b) == (k - 1, 0, False)
        assert ge.text_append(b, text[k:], is_last=True) == 0
        assert ge.trail_progress(b) == (len(text), 0, True)
        assert ge.wait(b)
        assert np.array_equal(ge.result(b)["codes"], ra["codes"]), k
    # closing through trail_append without TEXT_EOS equals the closed raw trail without it
    prompt, trail = ge.assets.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian)
    raw = trail[:-1]
    c = _closed(ge, prompt, raw, 16, 3, {})
    assert np.array_equal(c["codes"], _ref(oe, pad, prompt, 16, raw, 3))
    d = ge.submit(prompt, max_steps=16, seed=3, trailing_ids=raw[:3], open_trail=True)
    assert ge.trail_append(d, raw[3:], close=True) == 0
    assert ge.wait(d)
    assert np.array_equal(ge.result(d)["codes"], c["codes"])
    ge.close()


def test_edges(gpu, tiny_model, vivian):
    q3 = gpu
    ge = q3.Engine(tiny_model, "q8_0", max_batch=2, max_prompt=64, max_steps=16, load_codec=False)
    prompt, trail = ge.assets.prompt_build_streaming(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    # finished by max_steps while open: 1, nothing appended
    a = ge.submit(prompt, max_steps=3, seed=1, trailing_ids=trail[:5], open_trail=True)
    assert ge.wait(a)
    assert ge.trail_progress(a) == (5, 3, False)
    assert ge.trail_append(a, trail[5:]) == 1 and ge.trail_append(a, None, close=True) == 1
    assert ge.trail_progress(a) == (5, 3, False)
    assert ge.result(a)["codes"].shape == (3, 16)
    # errors: unknown id, a closed trail, a request not submitted open, the max_prompt cap, bad pieces
    L = q3.lib()
    ids = np.arange(3, dtype=np.int32)
    assert L.q3tts_trail_append(ge.h, 987654, q3._p(ids), 3, 0) < 0
    with pytest.raises(q3.Q3Error, match="unknown request id"):
        ge.trail_progress(987654)
    b = ge.submit(prompt, max_steps=6, seed=1, trailing_ids=trail[:2], open_trail=True)
    assert ge.trail_append(b, trail[2:4], close=True) == 0
    with pytest.raises(q3.Q3Error, match="closed"):
        ge.trail_append(b, trail[4:])
    with pytest.raises(q3.Q3Error, match="closed"):
        ge.trail_append(b, None, close=True)
    c = ge.submit(prompt, max_steps=6, seed=1, trailing_ids=trail)
    with pytest.raises(q3.Q3Error, match="open trail"):
        ge.trail_append(c, trail[:1])
    with pytest.raises(q3.Q3Error, match="open trail"):
        ge.text_append(c, trail[:1], is_last=True)
    assert ge.trail_progress(c) == (len(trail), 0, True)
    d = ge.submit(prompt, max_steps=6, seed=1, trailing_ids=np.arange(60, dtype=np.int32), open_trail=True)
    with pytest.raises(q3.Q3Error, match="max_prompt"):
        ge.trail_append(d, np.arange(5, dtype=np.int32))
    assert L.q3tts_trail_append(ge.h, d, None, 2, 0) < 0
    assert L.q3tts_trail_append(ge.h, d, q3._p(ids), -1, 0) < 0
    assert ge.trail_progress(d) == (60, 0, False)
    assert ge.trail_append(d, np.arange(4, dtype=np.int32), close=True) == 0
    with pytest.raises(q3.Q3Error, match="n_trail"):
        ge.submit(prompt, max_steps=6, trailing_ids=np.arange(65, dtype=np.int32), open_trail=True)
    for rid in (b, c, d):
        assert ge.wait(rid)
        ge.release(rid)
    ge.close()


def test_ggml_mode_rejects_open_requests(gpu, tiny_model, vivian):
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
        ge.submit(prompt, max_steps=4, open_trail=True)
    vid = ge.register_voice(vivian)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.submit_text(vid, np.arange(100, 104, dtype=np.int32), max_steps=4, streaming_text=True, open_text=True)
    assert not ge.sched_step()
    ge.close()


def test_slot_reuse_after_open_requests(gpu, tiny_model, vivian):
    """a slot freed by an open request -- one that finished while still open and waiting, one closed late -- serves plain and
    closed-trail requests that equal a fresh engine's"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=32, load_codec=True)
    prompt, trail = ge.assets.prompt_build_streaming(np.arange(400, 412, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    plain = ge.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    kw = dict(temperature=0.9, top_k=50, top_p=1.0, **UPSTREAM)
    a = ge.submit(prompt, max_steps=4, seed=2, trailing_ids=trail[:4], open_trail=True, want_pcm=True, **kw)   # ends open, at its cap
    b = ge.submit(plain, max_steps=12, seed=3, want_pcm=True, **kw)
    c = ge.submit(prompt, max_steps=10, seed=4, trailing_ids=trail[:3], open_trail=True, **kw)
    for _ in range(400):
        ge.sched_step()
        if ge.poll(a)["state"] == gpu.REQ_DONE and ge.poll(b)["state"] == gpu.REQ_DONE and ge.poll(c)["n_frames"] == 3:
            break
    assert ge.poll(a)["state"] == gpu.REQ_DONE and ge.poll(b)["state"] == gpu.REQ_DONE
    g0 = ge.stats()["graph_frames"]
    for _ in range(3):
        ge.sched_step()
    assert ge.poll(c)["n_frames"] == 3 and ge.stats()["graph_frames"] == g0
    assert ge.trail_append(c, trail[3:], close=True) == 0
    d = ge.submit(prompt, max_steps=12, seed=5, trailing_ids=trail, **kw)
    while ge.sched_step():
        pass
    res = {k: ge.result(r, want_pcm=(k in "ab")) for k, r in zip("abcd", (a, b, c, d))}
    ge.close()
    fresh = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=32, load_codec=True)
    for key, p, steps, seed, t, pcm in (("a", prompt, 4, 2, trail[:4], True), ("b", plain, 12, 3, None, True), ("c", prompt, 10, 4, trail, False),
                                        ("d", prompt, 12, 5, trail, False)):
        w = _closed(fresh, p, t, steps, seed, kw, want_pcm=pcm)
        assert np.array_equal(res[key]["codes"], w["codes"]), key
        if pcm:
            assert res[key]["pcm"].size == w["pcm"].size and _rms(res[key]["pcm"], w["pcm"]) < PCM_RMS_TOL, key
    fresh.close()


def test_group_of_one_device(gpu, tiny_model, vivian):
    q3 = gpu
    L = q3.lib()
    p = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 24, 0
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_voice_register.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs = np.zeros(1, np.int32)
    g = C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(p), q3._p(devs), 1, C.byref(g)))
    text = np.arange(200, 211, dtype=np.int32)
    try:
        spk = np.ascontiguousarray(vivian, np.float32)
        vid = C.c_int32()
        q3._chk(L.q3tts_group_voice_register(g, q3._p(spk), None, 0, None, 0, C.byref(vid)))
        sc = q3.SamplerConfig(0.7, 40, 0.9, 1, 17)
        rid = C.c_int64()
        head = np.ascontiguousarray(text[:3])
        q3._chk(L.q3tts_group_submit_text_streaming_open(g, vid.value, q3._p(head), 3, 2055, None, 0, C.byref(sc), 14, 1, 0, None,
                                                         C.byref(rid)))
        na, nc, cl = C.c_int32(), C.c_int32(), C.c_int32()
        q3._chk(L.q3tts_group_trail_progress(g, rid.value, C.byref(na), C.byref(nc), C.byref(cl)))
        assert (na.value, cl.value) == (2, 0)
        mid = np.ascontiguousarray(text[3:6])
        assert L.q3tts_group_trail_append(g, rid.value, q3._p(mid), 3, 0) == 0
        rest = np.ascontiguousarray(text[6:])
        assert L.q3tts_group_text_append(g, rid.value, q3._p(rest), rest.size, 1) == 0
        q3._chk(L.q3tts_group_trail_progress(g, rid.value, C.byref(na), C.byref(nc), C.byref(cl)))
        assert (na.value, cl.value) == (text.size, 1)
        assert L.q3tts_group_text_append(g, rid.value, None, 0, 1) < 0          # closed
        assert L.q3tts_group_trail_append(g, (rid.value | 5), None, 0, 1) < 0   # an engine index the group does not have
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


def test_fullsize_open_streams(gpu, vivian):
    """full-size model, 64 slots, every request open and fed by a thread while the driver runs: each equals its closed submission, and
    the 64-wide gated graph carries the run"""
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=64, max_steps=16, load_codec=False)
    rng = np.random.default_rng(65)
    built = [ge.assets.prompt_build_streaming(rng.integers(0, 4000, 4 + (i % 5) * 2).astype(np.int32), lang_id=2055, spk_emb=vivian)
             for i in range(64)]
    prompts, trails = [b[0] for b in built], [b[1] for b in built]
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    seeds = list(range(3000, 3064))
    want = ge.generate_batch(prompts, max_steps=12, seed=seeds, mask_eos=True, trailing_ids=trails, **kw)
    ge.reset_stats()
    # trails of at most 12 ids for 12 frames: no request can finish before its trail is closed.  All 64 are queued before the driver
    # starts, so they are admitted as one wave into the 64-wide graph
    ids = [ge.submit(prompts[i], max_steps=12, seed=seeds[i], trailing_ids=trails[i][:1], open_trail=True, **kw) for i in range(64)]
    ge.sched_start()
    errors = []
    try:
        th = threading.Thread(target=_feeder, args=(lambda rid, ids_, last: ge.trail_append(rid, ids_, close=last),
                                                     list(zip(ids, trails)), 99, errors, 0.002))
        th.start()
        th.join()
        assert not errors, errors
        for rid in ids:
            assert ge.wait(rid, 120000)
        got = [ge.result(rid) for rid in ids]
    finally:
        ge.sched_stop()
    st = ge.stats()
    ge.close()
    for i, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(g["codes"], w["codes"]), i
    assert st["graph_frames"] > 0 and st["slot_frames"] / st["graph_frames"] >= 48, st
