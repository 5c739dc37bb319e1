"""[EXT] request cancellation on the GPU (q3tts_cancel, q3tts_group_cancel, Q3TTS_REQ_CANCELLED): a request is stopped in every state it can be
in -- queued, inside an asynchronous prefill wave, running, running but waiting for text, draining -- and ends CANCELLED with the frames it
had (bit-identical to the same prefix of its uncancelled run) and the PCM of the chunks already handed to the codec; its slot, KV pages and
codec stream serve later requests as a fresh engine would; what shares the batch with it is untouched.  The scheduler is stepped by hand
wherever the point of cancellation has to be exact; every wait is bounded."""
import ctypes as C
import os
import threading
import time

import numpy as np
import pytest

import synth_models

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
WAIT_MS = 5000.0


def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((a - b) ** 2)))


def _steps(ge, n):
    for _ in range(n):
        assert ge.sched_step()


def _drain(ge, limit=2000):
    """steps until the engine reports idle; a scheduler that never gets there fails the test instead of hanging it"""
    for _ in range(limit):
        if not ge.sched_step():
            return
    raise AssertionError("the scheduler did not go idle")


def _until(ge, cond, limit=2000):
    for _ in range(limit):
        if cond():
            return
        ge.sched_step()
    raise AssertionError("condition not reached")


def _solo(gpu, model, quant, specs, use_graph=True, load_codec=False):
    """each (prompt, trail, steps, seed, kw, want_pcm) alone on a fresh one-slot engine"""
    ge = gpu.Engine(model, quant, max_batch=1, max_steps=40, load_codec=load_codec, use_graph=use_graph)
    out = []
    for p, t, steps, seed, kw, pcm in specs:
        rid = ge.submit(p, max_steps=steps, seed=seed, mask_eos=True, want_pcm=pcm and load_codec, trailing_ids=t, **kw)
        assert ge.wait(rid, 60000)
        out.append(ge.result(rid, want_pcm=pcm and load_codec))
    ge.close()
    return out


def _plain(ge, vivian, seed, n=8):
    rng = np.random.default_rng(seed)
    return ge.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


def _streaming(ge, vivian, seed, n=10):
    rng = np.random.default_rng(seed)
    return ge.assets.prompt_build_streaming(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_each_state(gpu, tiny_model, vivian, quant, use_graph):
    """queued, running (after exactly 2 groups), draining and done, on 5 requests over 4 slots"""
    ge = gpu.Engine(tiny_model, quant, max_batch=4, max_steps=24, load_codec=True, use_graph=use_graph)
    spf = ge.generate_batch([_plain(ge, vivian, 1)], max_steps=4, want_pcm=True)[0]["pcm"].size // 4
    # (prompt, trail, steps, seed, kw, want_pcm): run = cancelled while running, drain = cancelled while draining, two bystanders, one queued
    specs = [(_plain(ge, vivian, 10), None, 24, 70, SAMPLED, False), (_plain(ge, vivian, 11), None, 12, 71, {}, True),
             (_plain(ge, vivian, 12), None, 16, 72, dict(SAMPLED, **UPSTREAM), False), (_plain(ge, vivian, 13), None, 20, 73, {}, False),
             (_plain(ge, vivian, 14), None, 8, 74, {}, False)]
    ids = [ge.submit(p, max_steps=s, seed=seed, mask_eos=True, want_pcm=pcm, **kw) for p, t, s, seed, kw, pcm in specs]
    run, drain, by1, by2, queued = ids
    _steps(ge, 1)
    assert [ge.poll(r)["state"] for r in ids] == [gpu.REQ_RUNNING] * 4 + [gpu.REQ_QUEUED]
    # queued: CANCELLED at once, in this thread, with nothing
    assert ge.cancel(queued) is True
    st = ge.poll(queued)
    assert (st["state"], st["n_frames"], st["n_pcm"]) == (gpu.REQ_CANCELLED, 0, 0)
    assert ge.cancel(queued) is False and ge.wait(queued, WAIT_MS)
    ge.release(queued)
    # running: honoured between two frame groups
    _steps(ge, 1)
    assert ge.poll(run)["n_frames"] == 8
    assert ge.cancel(run) is True
    assert (ge.poll(run)["state"], ge.poll(run)["n_frames"]) == (gpu.REQ_RUNNING, 8)
    assert ge.cancel(run) is True                                         # the first one is still pending
    _steps(ge, 1)
    assert (ge.poll(run)["state"], ge.poll(run)["n_frames"]) == (gpu.REQ_CANCELLED, 8)
    assert ge.cancel(run) is False and ge.wait(run, WAIT_MS)
    # draining: that third group took `drain` to its 12 frames; its fence has not been harvested yet
    assert (ge.poll(drain)["state"], ge.poll(drain)["n_frames"]) == (gpu.REQ_DRAINING, 12)
    assert ge.cancel(drain) is True
    _until(ge, lambda: ge.poll(drain)["state"] != gpu.REQ_DRAINING)
    st = ge.poll(drain)
    assert (st["state"], st["n_frames"]) == (gpu.REQ_CANCELLED, 12)
    assert st["n_pcm"] % (4 * spf) == 0 and st["n_pcm"] <= 12 * spf
    _drain(ge)
    # done: nothing changes
    assert ge.poll(by1)["state"] == gpu.REQ_DONE and ge.cancel(by1) is False and ge.poll(by1)["state"] == gpu.REQ_DONE
    # an unknown id is an error with a message, not an abort
    assert gpu.lib().q3tts_cancel(ge.h, 987654) < 0 and b"unknown request id" in gpu.lib().q3tts_last_error()
    got = [ge.result(r, want_pcm=(r == drain)) for r in (run, drain, by1, by2)]
    assert not ge.sched_step()
    ge.close()
    want = _solo(gpu, tiny_model, quant, specs[:4], use_graph=use_graph, load_codec=True)
    assert got[0]["codes"].shape == (8, 16) and np.array_equal(got[0]["codes"], want[0]["codes"][:8])
    assert np.array_equal(got[1]["codes"], want[1]["codes"])
    n = got[1]["pcm"].size
    assert n == st["n_pcm"] and _rms(got[1]["pcm"], want[1]["pcm"][:n]) < PCM_RMS_TOL
    for g, w, s in zip(got[2:], want[2:], (16, 20)):                      # the others are unaffected
        assert g["state"] == gpu.REQ_DONE and g["codes"].shape == (s, 16) and np.array_equal(g["codes"], w["codes"])


def test_survivors_are_bit_exact(gpu, tiny_model, vivian):
    """greedy, sampled, sampled with generation options and streaming-text in one batch; the third is cancelled after 2 groups"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=False)
    sp, st = _streaming(ge, vivian, 23)
    specs = [(_plain(ge, vivian, 20), None, 20, 80, {}, False), (_plain(ge, vivian, 21, 11), None, 20, 81, SAMPLED, False),
             (_plain(ge, vivian, 22, 5), None, 20, 82, dict(SAMPLED, **UPSTREAM), False), (sp, st, 20, 83, SAMPLED, False)]
    ids = [ge.submit(p, max_steps=s, seed=seed, mask_eos=True, trailing_ids=t, **kw) for p, t, s, seed, kw, pcm in specs]
    _steps(ge, 2)
    assert ge.cancel(ids[2]) is True
    _drain(ge)
    assert [ge.poll(r)["state"] for r in ids] == [gpu.REQ_DONE, gpu.REQ_DONE, gpu.REQ_CANCELLED, gpu.REQ_DONE]
    got = [ge.result(r) for r in ids]
    ge.close()
    want = _solo(gpu, tiny_model, "q8_0", specs)
    for i, (g, w) in enumerate(zip(got, want)):
        n = 8 if i == 2 else 20
        assert g["codes"].shape == (n, 16) and np.array_equal(g["codes"], w["codes"][:n]), i


def test_pcm_prefix_and_stream_reuse(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=True)
    a, b = _plain(ge, vivian, 30), _plain(ge, vivian, 31, 12)
    rid = ge.submit(a, max_steps=24, seed=90, want_pcm=True, **SAMPLED)
    assert ge.wait(rid, 60000)
    want = ge.result(rid, want_pcm=True)
    spf = want["pcm"].size // 24
    assert want["pcm"].size == 24 * spf and spf > 0
    rid = ge.submit(a, max_steps=24, seed=90, want_pcm=True, **SAMPLED)
    _steps(ge, 3)
    assert ge.cancel(rid) is True
    _drain(ge)
    st = ge.poll(rid)
    assert (st["state"], st["n_frames"]) == (gpu.REQ_CANCELLED, 12)
    print("n_pcm of the cancelled request: %d (%d chunks of 3)" % (st["n_pcm"], st["n_pcm"] // (4 * spf)))
    assert st["n_pcm"] % (4 * spf) == 0
    assert st["n_pcm"] <= (st["n_frames"] // 4) * 4 * spf
    got = ge.result(rid, want_pcm=True)                                   # partial results stay fetchable until release
    assert np.array_equal(got["codes"], want["codes"][:12])
    assert got["pcm"].size == st["n_pcm"] and _rms(got["pcm"], want["pcm"][:got["pcm"].size]) < PCM_RMS_TOL
    # the codec stream it gave back (the free list is last-in first-out) decodes the next request as a fresh engine does
    nxt = ge.submit(b, max_steps=16, seed=91, want_pcm=True)
    assert ge.wait(nxt, 60000)
    got2 = ge.result(nxt, want_pcm=True)
    ge.close()
    w2 = _solo(gpu, tiny_model, "q8_0", [(b, None, 16, 91, {}, True)], load_codec=True)[0]
    assert np.array_equal(got2["codes"], w2["codes"])
    assert got2["pcm"].size == w2["pcm"].size == 16 * spf and _rms(got2["pcm"], w2["pcm"]) < PCM_RMS_TOL


def test_slot_kv_and_stream_reuse(gpu, tiny_model, vivian):
    """3 cycles of: fill the 4 slots with PCM requests, cancel all 4 mid-run, run 4 other requests.  The engine has 8 codec streams and KV pages
    for 4 sequences, so a cancel that leaked either would starve the second or third cycle"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=True)
    sp, st = _streaming(ge, vivian, 44)
    fresh = [(_plain(ge, vivian, 40), None, 12, 100, {}, True), (_plain(ge, vivian, 41, 13), None, 16, 101, dict(SAMPLED, **UPSTREAM), False),
             (sp, st, 14, 102, SAMPLED, True), (_plain(ge, vivian, 43, 4), None, 10, 103, SAMPLED, False)]
    got = []
    for cycle in range(3):
        doomed = [ge.submit(_plain(ge, vivian, 50 + 4 * cycle + i, 6 + i), max_steps=24, seed=200 + i, want_pcm=True, **(SAMPLED if i % 2 else {}))
                  for i in range(4)]
        _steps(ge, 2)
        assert [ge.poll(r)["n_frames"] for r in doomed] == [8] * 4
        for r in doomed:
            assert ge.cancel(r) is True
        ids = [ge.submit(p, max_steps=s, seed=seed, mask_eos=True, want_pcm=pcm, trailing_ids=t, **kw) for p, t, s, seed, kw, pcm in fresh]
        _drain(ge)
        for r in doomed:
            assert (ge.poll(r)["state"], ge.poll(r)["n_frames"]) == (gpu.REQ_CANCELLED, 8)
            ge.release(r)
        got.append([ge.result(r, want_pcm=spec[5]) for r, spec in zip(ids, fresh)])
    assert not ge.sched_step()
    ge.close()
    want = _solo(gpu, tiny_model, "q8_0", fresh, load_codec=True)
    for cycle in range(3):
        for i, (g, w) in enumerate(zip(got[cycle], want)):
            assert g["state"] == gpu.REQ_DONE and np.array_equal(g["codes"], w["codes"]), (cycle, i)
            if fresh[i][5]:
                assert g["pcm"].size == w["pcm"].size and _rms(g["pcm"], w["pcm"]) < PCM_RMS_TOL, (cycle, i)


def test_stalled_open_trail(gpu, tiny_model, vivian):
    """an open request without text, alone: every live slot waits, no frame group runs -- by hand, then under the driver thread, which sleeps"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=False)
    vid = ge.register_voice(vivian)
    text = np.arange(500, 509, dtype=np.int32)
    rid = ge.submit_text(vid, text[:1], max_steps=16, seed=5, streaming_text=True, open_text=True)
    _steps(ge, 3)                                                         # busy, but nothing to run
    g0 = ge.stats()["graph_frames"]
    assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"], g0) == (gpu.REQ_RUNNING, 0, 0)
    assert ge.cancel(rid) is True
    assert ge.text_append(rid, text[1:4]) == 1                            # from the moment cancel returned 0
    assert not ge.sched_step()                                            # the slot is retired and the engine is idle
    assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"]) == (gpu.REQ_CANCELLED, 0)
    assert ge.stats()["graph_frames"] == g0 and not ge.sched_step()
    assert ge.text_append(rid, text[1:], is_last=True) == 1 and ge.trail_progress(rid) == (0, 0, False)
    ge.release(rid)
    # the freed slot is a normal slot again
    chk = ge.submit_text(vid, text, max_steps=12, seed=6, streaming_text=True)
    assert ge.wait(chk, 60000)
    want = ge.result(chk)["codes"]
    ge.sched_start()
    try:
        rid = ge.submit_text(vid, text[:1], max_steps=16, seed=5, streaming_text=True, open_text=True)
        for _ in range(5000):                                             # prefilled: the driver finds nothing to run and goes to sleep
            if ge.poll(rid)["prefill_ms"] > 0:
                break
            assert not ge.wait(rid, 1.0)
        assert ge.poll(rid)["prefill_ms"] > 0 and ge.poll(rid)["state"] == gpu.REQ_RUNNING
        assert ge.cancel(rid) is True
        assert ge.wait(rid, WAIT_MS)                                      # the sleeping driver woke up
        assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"]) == (gpu.REQ_CANCELLED, 0)
        assert ge.text_append(rid, text[1:4]) == 1
        ge.release(rid)
        again = ge.submit_text(vid, text, max_steps=12, seed=6, streaming_text=True)
        assert ge.wait(again, 60000)
        assert np.array_equal(ge.result(again)["codes"], want)
    finally:
        ge.sched_stop()
    assert ge.stats()["graph_frames"] == g0 + 2 * 12
    ge.close()


def test_during_asynchronous_prefill(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=True)
    specs = [(_plain(ge, vivian, 60), None, 20, 300, SAMPLED, False), (_plain(ge, vivian, 61, 10), None, 16, 301, {}, True),
             (_plain(ge, vivian, 62, 14), None, 12, 302, SAMPLED, True),       # cancelled inside the wave; it holds a codec stream
             (_plain(ge, vivian, 63, 6), None, 12, 303, dict(SAMPLED, **UPSTREAM), False),
             (_plain(ge, vivian, 64, 9), None, 10, 304, SAMPLED, True)]        # takes the freed slot later

    def sub(i):
        p, t, s, seed, kw, pcm = specs[i]
        return ge.submit(p, max_steps=s, seed=seed, mask_eos=True, want_pcm=pcm, **kw)
    a, b = sub(0), sub(1)
    _steps(ge, 1)
    c, d = sub(2), sub(3)
    _steps(ge, 1)                                                         # slots are running: the wave of c and d is prefilled on the second stream
    assert [(ge.poll(r)["state"], ge.poll(r)["n_frames"]) for r in (a, b, c, d)] == [(gpu.REQ_RUNNING, 8)] * 2 + [(gpu.REQ_RUNNING, 0)] * 2
    assert ge.cancel(c) is True
    _until(ge, lambda: ge.poll(c)["state"] == gpu.REQ_CANCELLED)
    st = ge.poll(c)
    assert (st["n_frames"], st["n_pcm"]) == (0, 0) and st["first_chunk_ms"] == 0.0
    e = sub(4)
    _drain(ge)
    ge.release(c)
    got = {i: ge.result(r, want_pcm=specs[i][5]) for i, r in ((0, a), (1, b), (3, d), (4, e))}
    assert not ge.sched_step()
    ge.close()
    want = _solo(gpu, tiny_model, "q8_0", specs, load_codec=True)
    for i, g in got.items():
        assert g["state"] == gpu.REQ_DONE and g["codes"].shape == (specs[i][2], 16) and np.array_equal(g["codes"], want[i]["codes"]), i
        if specs[i][5]:
            assert g["pcm"].size == want[i]["pcm"].size and _rms(g["pcm"], want[i]["pcm"]) < PCM_RMS_TOL, i


def _canceller(ge, ended, targets, errors, answers):
    """cancels each request of targets = {rid: frames} the moment it has that many frames -- all of them watched at once, without
    sleeping: the tiny model runs its 24 frames in a few ms, so a clock alone would find every request either queued or done;
    answers[rid] = what cancel returned"""
    left = dict(targets)
    try:
        t0 = time.perf_counter()
        while left and time.perf_counter() - t0 < 20.0:
            for rid, n in list(left.items()):
                st = ge.poll(rid)
                if st["n_frames"] >= n or st["state"] in ended:
                    answers[rid] = ge.cancel(rid)
                    del left[rid]
    except Exception as ex:   # surfaced by the test thread
        errors.append(ex)


def test_canceller_thread(gpu, tiny_model, vivian):
    """the driver runs 8 requests through 4 slots while a seeded thread cancels half of them; two of those are open requests whose feeder
    never comes back.  DONE ones equal their solo runs, CANCELLED ones are prefixes of theirs"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=True)
    kws = [{}, SAMPLED, dict(SAMPLED, **UPSTREAM)]
    specs = []
    for i in range(8):
        if i % 4 == 3:
            p, t = _streaming(ge, vivian, 700 + i, 8 + i)
        else:
            p, t = _plain(ge, vivian, 700 + i, 5 + i), None
        specs.append((p, t, 24, 600 + i, kws[i % 3], i in (0, 3, 5)))
    want = []
    for p, t, s, seed, kw, pcm in specs:
        rid = ge.submit(p, max_steps=s, seed=seed, mask_eos=True, want_pcm=pcm, trailing_ids=t, **kw)
        assert ge.wait(rid, 60000)
        want.append(ge.result(rid, want_pcm=pcm))
    rng = np.random.default_rng(77)
    doomed = sorted({3, 7} | set(int(x) for x in rng.permutation([0, 1, 2, 4, 5, 6])[:2]))   # the open ones (3, 7) and two others
    ge.sched_start()
    errors, answers = [], {}
    try:
        ids = []
        for i, (p, t, s, seed, kw, pcm) in enumerate(specs):
            op = i in (3, 7)
            ids.append(ge.submit(p, max_steps=s, seed=seed, mask_eos=True, want_pcm=pcm, trailing_ids=(t[:3] if op else t), open_trail=op, **kw))
        # an open one gets as far as its 3 ids at the most; the others are caught anywhere in their run (0 frames: possibly still queued)
        targets = {ids[i]: int(rng.integers(0, 4 if i in (3, 7) else 20)) for i in doomed}
        th = threading.Thread(target=_canceller, args=(ge, (gpu.REQ_DONE, gpu.REQ_CANCELLED, gpu.REQ_FAILED), targets, errors, answers))
        th.start()
        th.join(30.0)
        assert not th.is_alive() and not errors, errors
        for rid in ids:
            assert ge.wait(rid, 60000)
        sts = [ge.poll(rid) for rid in ids]
        got = [ge.result(rid, want_pcm=specs[i][5]) for i, rid in enumerate(ids)]   # every one releases cleanly
    finally:
        ge.sched_stop()
    assert not ge.sched_step()
    ge.close()
    print("frames at the end:", [(i, s["state"], s["n_frames"]) for i, s in enumerate(sts)], "cancelled:", doomed)
    assert len(answers) == len(doomed)
    for i, (g, w, s) in enumerate(zip(got, want, sts)):
        assert s["state"] in (gpu.REQ_DONE, gpu.REQ_CANCELLED), i
        # a request whose cancel was accepted never reads DONE; one that had ended first, or was never cancelled, is DONE and whole
        assert (s["state"] == gpu.REQ_CANCELLED) == bool(answers.get(ids[i], False)), (i, answers)
        assert i not in (3, 7) or s["state"] == gpu.REQ_CANCELLED, i     # nothing but the cancel could end the open ones
        n = g["codes"].shape[0]
        assert n == s["n_frames"] and np.array_equal(g["codes"], w["codes"][:n]), i
        if s["state"] == gpu.REQ_DONE:
            assert n == 24
        if specs[i][5]:
            m = g["pcm"].size
            assert m == s["n_pcm"] and m <= w["pcm"].size and _rms(g["pcm"], w["pcm"][:m]) < PCM_RMS_TOL, i


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
    L.q3tts_group_poll.argtypes = [C.c_void_p, C.c_int64, C.POINTER(q3.ReqStatus)]
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
        stuck, full = C.c_int64(), C.c_int64()
        head = np.ascontiguousarray(text[:3])
        q3._chk(L.q3tts_group_submit_text_streaming_open(g, vid.value, q3._p(head), 3, 2055, None, 0, C.byref(sc), 14, 1, 0, None, C.byref(stuck)))
        q3._chk(L.q3tts_group_submit_text_streaming(g, vid.value, q3._p(text), text.size, 2055, None, 0, C.byref(sc), 14, 1, 0, None, C.byref(full)))
        assert L.q3tts_group_wait(g, full.value, 60000.0) == 0            # drives the scheduler; `stuck` waits at frame 2 beside it
        st = q3.ReqStatus()
        q3._chk(L.q3tts_group_poll(g, stuck.value, C.byref(st)))
        assert (st.state, st.n_frames) == (q3.REQ_RUNNING, 2)
        assert L.q3tts_group_cancel(g, (stuck.value | 5)) < 0             # an engine index the group does not have
        assert L.q3tts_group_cancel(g, stuck.value + (1 << 20)) < 0 and L.q3tts_last_error()   # an id the engine does not have
        assert L.q3tts_group_cancel(g, stuck.value) == 0
        rest = np.ascontiguousarray(text[3:])
        assert L.q3tts_group_text_append(g, stuck.value, q3._p(rest), rest.size, 1) == 1
        assert L.q3tts_group_wait(g, stuck.value, WAIT_MS) == 0
        q3._chk(L.q3tts_group_poll(g, stuck.value, C.byref(st)))
        assert (st.state, st.n_frames) == (q3.REQ_CANCELLED, 2)
        assert L.q3tts_group_cancel(g, stuck.value) == 1 and L.q3tts_group_cancel(g, full.value) == 1
        part, codes = np.zeros(14 * 16, np.int32), np.zeros(14 * 16, np.int32)
        gf, gp = C.c_int32(), C.c_int64()
        q3._chk(L.q3tts_group_fetch(g, stuck.value, q3._p(part), 0, 14, None, 0, 0, C.byref(gf), C.byref(gp)))
        assert gf.value == 2
        q3._chk(L.q3tts_group_fetch(g, full.value, q3._p(codes), 0, 14, None, 0, 0, C.byref(gf), C.byref(gp)))
        assert gf.value == 14
        q3._chk(L.q3tts_group_release(g, stuck.value))
        q3._chk(L.q3tts_group_release(g, full.value))
    finally:
        L.q3tts_group_destroy(g)
    assert np.array_equal(part[:32], codes[:32])                          # same voice, text prefix, sampler and seed: the same first frames


def test_ggml_mode_engine_cancels(gpu, tiny_model, vivian):
    old = os.environ.get("Q3_SPEC")
    os.environ["Q3_SPEC"] = "ggml"
    try:
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    finally:
        if old is None:
            os.environ.pop("Q3_SPEC")
        else:
            os.environ["Q3_SPEC"] = old
    prompt = _plain(ge, vivian, 3)
    whole = ge.generate_batch([prompt], max_steps=12, mask_eos=True)[0]["codes"]
    rid = ge.submit(prompt, max_steps=12, mask_eos=True)
    _steps(ge, 1)
    assert ge.cancel(rid) is True
    assert not ge.sched_step()
    assert ge.poll(rid)["state"] == gpu.REQ_CANCELLED
    assert np.array_equal(ge.result(rid)["codes"], whole[:4])
    ge.close()


def test_fullsize_cancel_16_of_64(gpu, vivian):
    """full-size model, 64 slots in the 64-wide graph: 16 are cancelled after 2 groups, the 48 others equal the uncancelled 64-slot run"""
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=64, max_steps=16, load_codec=False)
    rng = np.random.default_rng(66)
    prompts = [ge.assets.build_core(rng.integers(0, 4000, 4 + (i % 5) * 2).astype(np.int32), lang_id=2055, spk_emb=vivian) for i in range(64)]
    seeds = list(range(4000, 4064))
    want = ge.generate_batch(prompts, max_steps=16, seed=seeds, mask_eos=True, **SAMPLED)
    ids = [ge.submit(prompts[i], max_steps=16, seed=seeds[i], **SAMPLED) for i in range(64)]
    _steps(ge, 2)
    doomed = set(range(1, 64, 4))
    for i in sorted(doomed):
        assert ge.cancel(ids[i]) is True
    _drain(ge)
    for i, rid in enumerate(ids):
        g = ge.result(rid)
        n = 8 if i in doomed else 16
        assert g["state"] == (gpu.REQ_CANCELLED if i in doomed else gpu.REQ_DONE), i
        assert g["codes"].shape == (n, 16) and np.array_equal(g["codes"], want[i]["codes"][:n]), i
    assert not ge.sched_step()
    ge.close()
