"""[EXT] resume on the GPU (q3tts_submit_resume, q3tts_group_submit_resume, q3tts_op_feedback_rows; include/q3tts_spec.h "resume"): a request
handed the first k frames of its own uninterrupted run goes on with exactly the frames that run emits -- at every split point, graph and
eager, Q8_0 and Q5_K_M, greedy, sampled, with the generation options and with trailing text, across KV pages and prefill chunks, after a
cancel, on another engine, beside other requests -- and its PCM is that of the whole utterance.  The scheduler is stepped by hand where the
order matters; every wait is bounded."""
import ctypes as C

import numpy as np
import pytest

import resume_ref
import synth_models

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
WAIT_MS = 60000.0


def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((a - b) ** 2)))


def _steps(ge, n):
    for _ in range(n):
        assert ge.sched_step()


def _drain(ge, limit=4000):
    for _ in range(limit):
        if not ge.sched_step():
            return
    raise AssertionError("the scheduler did not go idle")


def _until(ge, cond, limit=4000):
    for _ in range(limit):
        if cond():
            return
        ge.sched_step()
    raise AssertionError("condition not reached")


def _plain(ge, vivian, seed, n=8):
    rng = np.random.default_rng(seed)
    return ge.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


def _streaming(ge, vivian, seed, n=10):
    rng = np.random.default_rng(seed)
    return ge.assets.prompt_build_streaming(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


def _run(ge, prompt, steps, seed, kw, trail=None, pcm=False, prefix=None):
    rid = ge.submit(prompt, max_steps=steps, seed=seed, mask_eos=True, want_pcm=pcm, trailing_ids=trail, prefix_codes=prefix, **kw)
    assert ge.wait(rid, WAIT_MS)
    return ge.result(rid, want_pcm=pcm)


# ---- 1. the feedback rows ----
@pytest.mark.parametrize("n", [1, 3, 17])
def test_feedback_rows_bit_exact(gpu, tiny_model, n):
    import os
    a = gpu.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    pad = a.tts_pad()
    rng = np.random.default_rng(100 + n)
    codes = rng.integers(0, 2048, (n, 16)).astype(np.int32)
    codes[0, 15] = 2047                                                  # the table's last row
    codes[n - 1, 0] = 2159                                               # code_0's table is longer: the talker's last sampled id
    codes[n // 2, 7] = 2048                                              # one past a residual table: the zero row
    codes[n // 2, 9] = -3                                                # negative: row 0
    want_pad = resume_ref.feedback_rows(a, pad, codes)
    got = gpu.op_feedback_rows(a, codes)
    assert got.dtype == np.float32 and got.shape == (n, 2048) and np.array_equal(got, want_pad)
    for trail in ([5], [7, 151673, 4095, 4096, 12][: max(1, min(n, 5))], list(range(30, 30 + n)), list(range(30, 30 + n + 4))):
        # fewer ids than rows (the rest adds tts_pad), an id outside the 4096-row table (fallback row), its edges, more ids than rows
        want = resume_ref.feedback_rows(a, pad, codes, trail[:n])
        # sentinel rows around the host buffer; the entry point itself guards the device rows on either side
        buf = np.full((n + 2, 2048), -777.0, np.float32)
        t = np.asarray(trail, np.int32)
        gpu._chk(gpu.lib().q3tts_op_feedback_rows(a.h, gpu._p(codes), n, gpu._p(t), t.size, C.c_void_p(buf.ctypes.data + 2048 * 4)))
        assert np.array_equal(buf[1:n + 1], want), trail
        assert np.all(buf[0] == -777.0) and np.all(buf[n + 1] == -777.0)
        assert not np.array_equal(want[0], want_pad[0])
    a.close()


# ---- 2. every split point ----
MODES = [("greedy", {}, False), ("sampled", SAMPLED, False), ("upstream", dict(SAMPLED, **UPSTREAM), False),
         ("greedy_penalty", dict(repetition_penalty=1.3), False), ("trail_long", dict(SAMPLED, **UPSTREAM), 16), ("trail_short", SAMPLED, 5)]


@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_every_split_point(gpu, tiny_model, vivian, quant, use_graph):
    """12 frames uninterrupted, then resumed at every k in 1..11: the 11 resumed requests queue through 4 slots, so the first wave is
    prefilled in line and the later ones asynchronously beside running slots"""
    ge = gpu.Engine(tiny_model, quant, max_batch=4, max_steps=40, load_codec=False, use_graph=use_graph)
    one = gpu.Engine(tiny_model, quant, max_batch=1, max_steps=40, load_codec=False, use_graph=use_graph)   # always the in-line prefill
    for i, (name, kw, n_text) in enumerate(MODES):
        if n_text:
            prompt, trail = _streaming(ge, vivian, 40 + i, n_text)       # n_text trailing ids: longer (16) or shorter (5) than the split points
            assert len(trail) == n_text
        else:
            prompt, trail = _plain(ge, vivian, 40 + i, 6 + i), None
        want = _run(ge, prompt, 12, 900 + i, kw, trail)["codes"]
        assert want.shape == (12, 16)
        ids = [ge.submit(prompt, max_steps=12, seed=900 + i, mask_eos=True, trailing_ids=trail, prefix_codes=want[:k], **kw) for k in range(1, 12)]
        assert [ge.poll(r)["n_frames"] for r in ids] == list(range(1, 12))          # the prefix counts from the start
        _drain(ge)
        for k, rid in zip(range(1, 12), ids):
            g = ge.result(rid)
            assert g["state"] == gpu.REQ_DONE and g["codes"].shape == (12, 16), (name, k)
            assert np.array_equal(g["codes"], want), (name, k, np.argwhere(g["codes"] != want)[:3])
        for k in (1, 6, 11):
            assert np.array_equal(_run(one, prompt, 12, 900 + i, kw, trail, prefix=want[:k])["codes"], want), (name, k, "one slot")
    assert not ge.sched_step()
    ge.close()
    one.close()


def test_another_seed_keeps_the_prefix_and_redraws_the_rest(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=40, load_codec=False)
    prompt = _plain(ge, vivian, 77)
    want = _run(ge, prompt, 16, 5, SAMPLED)["codes"]
    got = _run(ge, prompt, 16, 6, SAMPLED, prefix=want[:8])["codes"]
    ge.close()
    assert np.array_equal(got[:8], want[:8]) and not np.array_equal(got[8:], want[8:])


# ---- 3. page and chunk boundaries ----
def test_prefix_crosses_the_kv_page(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=False)
    prompt = _plain(ge, vivian, 50, 44)
    n = prompt.shape[0]
    assert 64 - 30 < n < 64, n
    kw = dict(SAMPLED, **UPSTREAM)
    want = _run(ge, prompt, 40, 31, kw)["codes"]
    for k in (63 - n, 64 - n, 65 - n, 70 - n):                          # the last prefix row is the page's last row, the next page's first, further on
        assert n < 64 <= n + k + 1 and k < 40
        assert np.array_equal(_run(ge, prompt, 40, 31, kw, prefix=want[:k])["codes"], want), k
    ge.close()


@pytest.mark.parametrize("beside_running", [False, True])
def test_prefix_spans_two_prefill_chunks(gpu, tiny_model, vivian, beside_running):
    """n_prompt + k exceeds the talker's prefill launch width (read from the engine; the tiny model's 256 is within max_prompt + max_steps):
    the prefix starts in the first chunk and ends in the second -- in line, and asynchronously beside a running request"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=False)
    width = ge.prefill_width()
    prompt = _plain(ge, vivian, 51, width - 26)
    n = prompt.shape[0]
    assert width - 30 < n < width - 2, (n, width)
    k = width - n + 6
    assert 2 < k < 36 and n + k > width
    want = _run(ge, prompt, k + 4, 32, SAMPLED)["codes"]
    other_p = _plain(ge, vivian, 52, 9)
    other_want = _run(ge, other_p, 24, 33, SAMPLED)["codes"]
    if beside_running:
        other = ge.submit(other_p, max_steps=24, seed=33, mask_eos=True, **SAMPLED)
        _steps(ge, 1)
        assert ge.poll(other)["n_frames"] == 4
    rid = ge.submit(prompt, max_steps=k + 4, seed=32, mask_eos=True, prefix_codes=want[:k], **SAMPLED)
    if beside_running:
        _steps(ge, 1)                                                    # the wave is prefilled on the second stream
        assert (ge.poll(other)["n_frames"], ge.poll(rid)["n_frames"]) == (8, k)
    _drain(ge)
    assert np.array_equal(ge.result(rid)["codes"], want)
    if beside_running:
        assert np.array_equal(ge.result(other)["codes"], other_want)
    ge.close()


# ---- 4. cancel, then resume ----
def test_cancel_then_resume_same_and_fresh_engine(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=40, load_codec=False)
    prompt = _plain(ge, vivian, 60, 9)
    kw = dict(SAMPLED, **UPSTREAM)
    want = _run(ge, prompt, 20, 44, kw)["codes"]
    rid = ge.submit(prompt, max_steps=20, seed=44, mask_eos=True, **kw)
    _steps(ge, 2)
    assert ge.cancel(rid) is True
    _drain(ge)
    part = ge.result(rid)
    assert part["state"] == gpu.REQ_CANCELLED and part["codes"].shape == (8, 16) and np.array_equal(part["codes"], want[:8])
    same = _run(ge, prompt, 20, 44, kw, prefix=part["codes"])           # the one slot the cancel freed
    ge.close()
    ge2 = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=False)
    fresh = _run(ge2, prompt, 20, 44, kw, prefix=part["codes"])
    ge2.close()
    for g in (same, fresh):
        assert g["state"] == gpu.REQ_DONE and np.array_equal(g["codes"], want)


# ---- 5. PCM ----
@pytest.mark.parametrize("k", [8, 6])
def test_pcm_of_the_whole_utterance(gpu, tiny_model, vivian, k):
    """k a multiple of the 4-frame chunk, and k = 6: the prefix ends inside a chunk the new frames complete"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=True)
    prompt = _plain(ge, vivian, 61, 7)
    want = _run(ge, prompt, 14, 45, SAMPLED, pcm=True)
    spf = want["pcm"].size // 14
    assert spf > 0 and want["pcm"].size == 14 * spf
    rid = ge.submit(prompt, max_steps=14, seed=45, mask_eos=True, want_pcm=True, prefix_codes=want["codes"][:k], **SAMPLED)
    codes, _ = ge.fetch(rid, 0, 40)
    assert np.array_equal(codes, want["codes"][:k])                      # fetchable at once
    assert ge.wait(rid, WAIT_MS)
    got = ge.result(rid, want_pcm=True)
    ge.close()
    assert np.array_equal(got["codes"], want["codes"])
    rms = _rms(got["pcm"], want["pcm"]) if got["pcm"].size == want["pcm"].size else float("nan")
    print("k = %d: n_pcm %d / %d, rms %.3g" % (k, got["pcm"].size, want["pcm"].size, rms))
    assert got["n_pcm"] == want["n_pcm"] == got["pcm"].size == want["pcm"].size
    assert rms < PCM_RMS_TOL


# ---- 6. mixed batch ----
def test_mixed_batch(gpu, tiny_model, vivian):
    """a resumed request joins running plain, streaming-text and open-trail requests through an asynchronous prefill wave; a second one
    takes the slot the first plain request frees"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=40, load_codec=False)
    sp, st = _streaming(ge, vivian, 71, 9)
    op, ot = _streaming(ge, vivian, 72, 12)
    kw_r = dict(SAMPLED, **UPSTREAM)
    rp, rp2 = _plain(ge, vivian, 73, 10), _plain(ge, vivian, 74, 5)
    solo = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=40, load_codec=False)
    w_plain = _run(solo, _plain(ge, vivian, 70), 12, 50, SAMPLED)["codes"]
    w_stream = _run(solo, sp, 28, 51, kw_r, st)["codes"]
    w_open = _run(solo, op, 24, 52, SAMPLED, ot)["codes"]
    w_res = _run(solo, rp, 30, 53, kw_r)["codes"]
    w_res2 = _run(solo, rp2, 22, 54, dict(repetition_penalty=1.3))["codes"]
    solo.close()
    a = ge.submit(_plain(ge, vivian, 70), max_steps=12, seed=50, mask_eos=True, **SAMPLED)
    b = ge.submit(sp, max_steps=28, seed=51, mask_eos=True, trailing_ids=st, **kw_r)
    _steps(ge, 1)
    c = ge.submit(op, max_steps=24, seed=52, mask_eos=True, trailing_ids=ot[:6], open_trail=True, **SAMPLED)
    d = ge.submit(rp, max_steps=30, seed=53, mask_eos=True, prefix_codes=w_res[:13], **kw_r)
    _steps(ge, 1)                                                        # a and b run on; c and d are one asynchronous wave
    assert [ge.poll(r)["n_frames"] for r in (a, b, c, d)] == [8, 8, 0, 13]
    e = ge.submit(rp2, max_steps=22, seed=54, mask_eos=True, prefix_codes=w_res2[:7], repetition_penalty=1.3)
    _steps(ge, 2)
    assert ge.trail_append(c, ot[6:], close=True) == 0
    _drain(ge)
    for rid, w, name in ((a, w_plain, "plain"), (b, w_stream, "streaming"), (c, w_open, "open"), (d, w_res, "resumed"), (e, w_res2, "resumed 2")):
        g = ge.result(rid)
        assert g["state"] == gpu.REQ_DONE and np.array_equal(g["codes"], w), name
    assert not ge.sched_step()
    ge.close()


# ---- 7. edges ----
def test_k0_is_the_plain_submission_and_refusals_queue_nothing(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=False)
    L = gpu.lib()
    sp, st = _streaming(ge, vivian, 80, 7)
    want = _run(ge, sp, 10, 60, SAMPLED, st)["codes"]
    got = _run(ge, sp, 10, 60, SAMPLED, st, prefix=np.zeros((0, 16), np.int32))["codes"]
    assert np.array_equal(got, want)
    r = gpu.Request()
    pr = np.ascontiguousarray(sp, np.float32)
    ge._fill(r, pr, 0, 10, 0.9, 50, 1.0, 60, True)
    tr = np.ascontiguousarray(st, np.int32)
    good = np.ascontiguousarray(want[:4])

    def sub(codes, n_prefix, open_=0, n_trail=tr.size, steps=10):
        r.max_steps = steps
        rid = C.c_int64(-1)
        rc = L.q3tts_submit_resume(ge.h, C.byref(r), 0, None, gpu._p(tr), n_trail, open_, gpu._p(codes) if codes is not None else None, n_prefix,
                                   C.byref(rid))
        return rc, L.q3tts_last_error() if rc < 0 else b"", rid.value

    def bad(q, v):
        c = good.copy()
        c[1, q] = v
        return c
    for args, why in (((good, -1), b">= 0"), ((good, 4, 0, tr.size, 4), b"max_steps"), ((good, 4, 0, tr.size, 3), b"max_steps"), ((None, 4), b"missing"),
                      ((bad(0, 2160), 4), b"code_0"), ((bad(0, -1), 4), b"code_0"), ((bad(0, 2150), 4), b"EOS"), ((bad(3, 2048), 4), b"residual"),
                      ((bad(15, -2), 4), b"residual"), ((good, 4, 1, 3), b"open trail")):
        rc, err, rid = sub(*args)
        assert rc < 0 and why in err and rid == -1, (args[1:], err)
    assert not ge.sched_step()                                           # nothing was queued
    rc, err, rid = sub(good, 4)
    assert rc == 0 and rid > 0
    assert ge.wait(rid, WAIT_MS) and np.array_equal(ge.result(rid)["codes"], want)
    ge.close()


def test_cancel_during_the_prefix_prefill(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=True)
    p1, p2 = _plain(ge, vivian, 81), _plain(ge, vivian, 82, 11)
    want = _run(ge, p2, 16, 62, SAMPLED, pcm=True)
    w1 = _run(ge, p1, 24, 61, {})["codes"]
    a = ge.submit(p1, max_steps=24, seed=61, mask_eos=True)
    _steps(ge, 1)
    rid = ge.submit(p2, max_steps=16, seed=62, mask_eos=True, want_pcm=True, prefix_codes=want["codes"][:9], **SAMPLED)
    _steps(ge, 1)                                                        # admitted into an asynchronous wave
    assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"], ge.poll(a)["n_frames"]) == (gpu.REQ_RUNNING, 9, 8)
    assert ge.cancel(rid) is True
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_CANCELLED)
    st = ge.poll(rid)
    assert st["n_frames"] == 9
    g = ge.result(rid, want_pcm=True)
    assert np.array_equal(g["codes"], want["codes"][:9])                 # what it had at that moment includes the prefix
    assert g["pcm"].size == st["n_pcm"] and g["pcm"].size <= want["pcm"].size and _rms(g["pcm"], want["pcm"][:g["pcm"].size]) < PCM_RMS_TOL
    # the slot, its pages and the codec stream serve the same resume again
    again = ge.submit(p2, max_steps=16, seed=62, mask_eos=True, want_pcm=True, prefix_codes=want["codes"][:9], **SAMPLED)
    _drain(ge)
    g2 = ge.result(again, want_pcm=True)
    assert np.array_equal(g2["codes"], want["codes"]) and g2["pcm"].size == want["pcm"].size and _rms(g2["pcm"], want["pcm"]) < PCM_RMS_TOL
    assert np.array_equal(ge.result(a)["codes"], w1)
    # cancelled while still queued: CANCELLED at once, the prefix stays
    b = ge.submit(p1, max_steps=24, seed=61, mask_eos=True)
    c = ge.submit(p1, max_steps=24, seed=61, mask_eos=True)
    q = ge.submit(p2, max_steps=16, seed=62, mask_eos=True, prefix_codes=want["codes"][:5], **SAMPLED)
    _steps(ge, 1)
    assert ge.poll(q)["state"] == gpu.REQ_QUEUED and ge.cancel(q) is True
    assert (ge.poll(q)["state"], ge.poll(q)["n_frames"]) == (gpu.REQ_CANCELLED, 5)
    assert np.array_equal(ge.result(q)["codes"], want["codes"][:5])
    _drain(ge)
    ge.release(b)
    ge.release(c)
    ge.close()


def test_open_trail_resumed_then_appended_and_closed(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=40, load_codec=False)
    sp, st = _streaming(ge, vivian, 83, 12)
    kw = dict(SAMPLED, **UPSTREAM)
    want = _run(ge, sp, 20, 63, kw, st)["codes"]
    for k, have in ((5, 5), (5, 8)):                                     # exactly the prefix's ids (the slot waits at once), and a few more
        rid = ge.submit(sp, max_steps=20, seed=63, mask_eos=True, trailing_ids=st[:have], open_trail=True, prefix_codes=want[:k], **kw)
        _steps(ge, 4)
        assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"]) == (gpu.REQ_RUNNING, have)   # it waits for text at frame `have`
        assert ge.trail_append(rid, st[have:have + 2]) == 0
        _steps(ge, 2)
        assert ge.poll(rid)["n_frames"] == have + 2
        assert ge.trail_append(rid, st[have + 2:], close=True) == 0
        _drain(ge)
        g = ge.result(rid)
        assert g["state"] == gpu.REQ_DONE and np.array_equal(g["codes"], want), (k, have)
    ge.close()


def test_group_failover_to_the_other_engine(gpu, tiny_model, vivian):
    """a group with the device listed twice: k frames on engine 0, cancel, q3tts_group_submit_resume on engine 1"""
    q3 = gpu
    L = q3.lib()
    p = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 40, 0
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_engine.restype = C.c_void_p
    L.q3tts_group_engine.argtypes = [C.c_void_p, C.c_int32]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_poll.argtypes = [C.c_void_p, C.c_int64, C.POINTER(q3.ReqStatus)]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    L.q3tts_group_device_of.argtypes = [C.c_void_p, C.c_int64]
    devs = np.zeros(2, np.int32)
    g = C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(p), q3._p(devs), 2, C.byref(g)))
    try:
        assets = q3.Assets(handle=L.q3tts_engine_assets(L.q3tts_group_engine(g, 0)))
        rng = np.random.default_rng(90)
        prompt = np.ascontiguousarray(assets.build_core(rng.integers(0, 4000, 9).astype(np.int32), lang_id=2055, spk_emb=vivian), np.float32)
        r = q3.Request()
        r.prompt, r.n_prompt, r.max_steps, r.mask_eos = prompt.ctypes.data, prompt.shape[0], 20, 1
        r.sampler = q3.SamplerConfig(0.9, 50, 1.0, 1, 64)
        o = q3.GenOptions(**UPSTREAM)
        st = q3.ReqStatus()
        gf, gp = C.c_int32(), C.c_int64()

        def fetch(rid):
            out = np.zeros(40 * 16, np.int32)
            q3._chk(L.q3tts_group_fetch(g, rid, q3._p(out), 0, 40, None, 0, 0, C.byref(gf), C.byref(gp)))
            return out[: gf.value * 16].reshape(-1, 16).copy()
        whole = C.c_int64()
        q3._chk(L.q3tts_group_submit_resume(g, 0, C.byref(r), 0, C.byref(o), None, 0, 0, None, 0, C.byref(whole)))   # n_prefix = 0: plain
        assert whole.value & 255 == 0 and L.q3tts_group_wait(g, whole.value, WAIT_MS) == 0
        want = fetch(whole.value)
        assert want.shape == (20, 16)
        q3._chk(L.q3tts_group_release(g, whole.value))
        first = C.c_int64()
        q3._chk(L.q3tts_group_submit_resume(g, 0, C.byref(r), 0, C.byref(o), None, 0, 0, None, 0, C.byref(first)))
        e0 = L.q3tts_group_engine(g, 0)
        busy = C.c_int32()
        for _ in range(2):
            q3._chk(L.q3tts_sched_step(e0, C.byref(busy)))
        assert L.q3tts_group_cancel(g, first.value) == 0
        assert L.q3tts_group_wait(g, first.value, WAIT_MS) == 0
        q3._chk(L.q3tts_group_poll(g, first.value, C.byref(st)))
        assert (st.state, st.n_frames) == (q3.REQ_CANCELLED, 8)
        part = fetch(first.value)
        q3._chk(L.q3tts_group_release(g, first.value))
        assert np.array_equal(part, want[:8])
        bad = C.c_int64(-1)
        assert L.q3tts_group_submit_resume(g, 2, C.byref(r), 0, C.byref(o), None, 0, 0, q3._p(part), 8, C.byref(bad)) < 0 and bad.value == -1
        second = C.c_int64()
        q3._chk(L.q3tts_group_submit_resume(g, 1, C.byref(r), 0, C.byref(o), None, 0, 0, q3._p(part), 8, C.byref(second)))
        assert second.value & 255 == 1
        assert L.q3tts_group_wait(g, second.value, WAIT_MS) == 0
        q3._chk(L.q3tts_group_poll(g, second.value, C.byref(st)))
        got = fetch(second.value)
        q3._chk(L.q3tts_group_release(g, second.value))
        assert st.state == q3.REQ_DONE and np.array_equal(got, want)
    finally:
        L.q3tts_group_destroy(g)


# ---- 8. full size ----
def test_fullsize_16_slots_4_resumed(gpu, synth_tool, vivian):
    """Q3TTS-1.7B-synth, 16 slots, 24 frames: 4 requests are resumed at different k -- one with n_prompt + k past the prefill launch width
    and past a 128-position boundary -- beside 12 plain ones; all 16 equal the uninterrupted 16-slot run"""
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=16, max_steps=24, load_codec=False)
    width = ge.prefill_width()
    rng = np.random.default_rng(88)
    n_text = [4 + (i % 5) * 2 for i in range(16)]
    n_text[5] = width - 22
    prompts = [ge.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian) for n in n_text]
    n5 = prompts[5].shape[0]
    assert width - 24 < n5 < width - 4
    ks = {2: 3, 5: width - n5 + 7, 9: 12, 14: 23}
    assert n5 + ks[5] > width and (n5 // 128) != ((n5 + ks[5]) // 128) and ks[5] < 24
    seeds = list(range(7000, 7016))
    kws = [dict(SAMPLED, **UPSTREAM) if i % 2 else SAMPLED for i in range(16)]
    want = []
    ids = [ge.submit(prompts[i], max_steps=24, seed=seeds[i], mask_eos=True, **kws[i]) for i in range(16)]
    _drain(ge)
    want = [ge.result(r)["codes"] for r in ids]
    ids = [ge.submit(prompts[i], max_steps=24, seed=seeds[i], mask_eos=True, prefix_codes=(want[i][:ks[i]] if i in ks else None), **kws[i])
           for i in range(16)]
    _drain(ge)
    for i, rid in enumerate(ids):
        g = ge.result(rid)
        assert g["state"] == gpu.REQ_DONE and g["codes"].shape == (24, 16) and np.array_equal(g["codes"], want[i]), (i, ks.get(i))
    assert not ge.sched_step()
    ge.close()
