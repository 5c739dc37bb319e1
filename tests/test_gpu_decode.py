"""[EXT] decoding given frames on the GPU (q3tts_submit_decode, q3tts_group_submit_decode; include/q3tts_spec.h "decoding given frames").
D1: the PCM of a decode-only request is the PCM of the request that emitted the frames -- at every chunk shape, on a fresh engine, on the
engine that generated them, and against the standalone decoder fed the same chunks.  D2: requests that share the engine with decode-only
requests keep their codes bit for bit and their PCM within the standing tolerance.  D3: no slot, no prefill, no frame.  Then the scheduling:
no slot is needed, at most decode_width requests hold a stream, cancels at every point, every refusal, the candidate-set workflow the call
exists for, and the driver thread and a group.  Tiny model, Q8_0 (the codec does not depend on the talker's quantisation), max_steps <= 24.
The scheduler is stepped by hand except where a test says otherwise; every wait is bounded."""
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
WAIT_MS = 60000.0
SAMPLE_END, CODEC_EOS = 2160, 2150   # Q3_SAMPLE_END, Q3_CODEC_EOS


def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((a - b) ** 2)))


def _steps(ge, n):
    for _ in range(n):
        assert ge.sched_step()


def _drain(ge, limit=4000):
    """steps until the engine reports idle; a scheduler that never gets there fails the test instead of hanging it"""
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


class Takes:
    """generated once, shared, read-only: take(p, n, sampled, seed) is the request of prompt p run alone with PCM on a one-slot engine for
    exactly n frames (mask_eos), greedy or sampled with `seed` (p when not given).  Every comparison in this file is against one of these."""

    def __init__(self, gpu, model, vivian):
        self.ge = gpu.Engine(model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
        self.vivian, self.memo = vivian, {}
        self.spf = None

    def prompt(self, seed):
        return _plain(self.ge, self.vivian, seed)

    def __call__(self, p, n, sampled=False, seed=None):
        seed = p if seed is None else seed
        key = (p, n, sampled, seed)
        if key not in self.memo:
            rid = self.ge.submit(self.prompt(p), max_steps=n, seed=seed, mask_eos=True, want_pcm=True, **(SAMPLED if sampled else {}))
            assert self.ge.wait(rid, WAIT_MS)
            r = self.ge.result(rid, want_pcm=True)
            assert r["state"] == 3 and r["codes"].shape == (n, 16) and r["pcm"].size > 0 and r["pcm"].size % n == 0
            r["codes"].setflags(write=False), r["pcm"].setflags(write=False)
            self.spf = r["pcm"].size // n
            self.memo[key] = r
        return self.memo[key]


@pytest.fixture(scope="module")
def takes(gpu, tiny_model, vivian):
    t = Takes(gpu, tiny_model, vivian)
    yield t
    t.ge.close()


def _decode(ge, codes, gpu):
    rid = ge.submit_decode(codes)
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    return ge.result(rid, want_pcm=True)


def _same_pcm(got, want, what):
    """equal count, RMS below the standing tolerance; returns the RMS"""
    assert got.size == want.size, (what, got.size, want.size)
    rms = _rms(got, want)
    assert rms < PCM_RMS_TOL, "%s: PCM rms %.3e" % (what, rms)
    return rms


# ---------------------------------------------------------------- 1: D1 ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 8, 9])
def test_decode_equals_generate(gpu, tiny_model, takes, n):
    """tail only (1, 3), exact chunks (4, 8), chunks plus a tail of 1 (5, 9)"""
    ref = takes(40 + n, n)
    fresh = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    rid = fresh.submit_decode(ref["codes"])
    st = fresh.poll(rid)
    assert (st["state"], st["n_frames"], st["n_pcm"], st["prefill_ms"]) == (gpu.REQ_QUEUED, n, 0, 0.0)   # the frames are there from submission on
    codes, _ = fresh.fetch(rid, 0, n)
    assert np.array_equal(codes, ref["codes"])
    seen = [0]
    for _ in range(4000):                                                 # n_pcm grows chunk by chunk and never shrinks: the PCM can be streamed
        st = fresh.poll(rid)
        assert st["n_pcm"] >= seen[-1] and st["n_frames"] == n and st["state"] in (gpu.REQ_QUEUED, gpu.REQ_DRAINING, gpu.REQ_DONE)
        seen.append(st["n_pcm"])
        if st["state"] == gpu.REQ_DONE:
            break
        fresh.sched_step()
    a = fresh.result(rid, want_pcm=True)
    assert not fresh.sched_step()
    fresh.close()
    assert a["state"] == gpu.REQ_DONE and np.array_equal(a["codes"], ref["codes"]) and a["prefill_ms"] == 0.0 and "logprobs" not in a
    b = _decode(takes.ge, ref["codes"], gpu)                              # the engine that generated them
    dec = gpu.Decoder(os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"))
    dec.reset()
    alone = np.concatenate([dec.decode(ref["codes"][f:f + 4], is_last=f + 4 >= n) for f in range(0, n, 4)])
    dec.close()
    worst = max(_same_pcm(a["pcm"], ref["pcm"], "fresh engine"), _same_pcm(b["pcm"], ref["pcm"], "same engine"),
                _same_pcm(a["pcm"], alone, "standalone decoder"))
    assert worst < PCM_RMS_TOL, "largest PCM rms over the three comparisons: %.3e" % worst
    print("n = %d: largest PCM rms %.3e" % (n, worst))


# ---------------------------------------------------------------- 2: D3 ----------------------------------------------------------------
@pytest.mark.parametrize("n", [7, 16])
def test_no_talker_work(gpu, tiny_model, takes, n):
    ref = takes(60, 16)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=True)
    s0 = ge.stats()
    out = _decode(ge, ref["codes"][:n], gpu)
    assert out["pcm"].size == n * takes.spf and out["first_chunk_ms"] > 0.0
    s1 = ge.stats()
    assert (s1["graph_frames"], s1["frames"], s1["prefill_ms"], s1["sched_steps"]) == (0, 0, 0.0, 0)
    assert s1["codec_calls"] - s0["codec_calls"] == -(-n // 4)
    assert ge.decode_stats() == dict(requests=1, chunks=-(-n // 4), chunks_shared=0)
    assert not ge.sched_step()
    ge.close()
    if n == 16:
        _same_pcm(out["pcm"], ref["pcm"], "idle engine")


# ---------------------------------------------------------------- 3 and 9: beside live requests ----------------------------------------------------------------
LIVE = [(71, 16), (72, 16), (73, 16)]          # (seed, frames) of the sampled requests with PCM
GIVEN = [(81, 4), (82, 7), (83, 8), (84, 12), (85, 16)]   # (seed, length) of the decode-only requests


def _mixture(gpu, tiny_model, takes, driver):
    want_live = [takes(s, n, sampled=True) for s, n in LIVE]
    given, want_given = [takes(s, n)["codes"] for s, n in GIVEN], [takes(s, n)["pcm"] for s, n in GIVEN]
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=16, load_codec=True)
    assert ge.decode_width() == 2
    if driver:
        ge.sched_start()
    live = [ge.submit(takes.prompt(s), max_steps=n, seed=s, mask_eos=True, want_pcm=True, **SAMPLED) for s, n in LIVE]
    if driver:
        for _ in range(10 ** 7):                                          # bounded: the first frame group has run
            if ge.poll(live[0])["n_frames"] >= 4:
                break
        else:
            raise AssertionError("no frame group ran")
    else:
        _steps(ge, 1)
        assert [ge.poll(r)["n_frames"] for r in live] == [4, 4, 4]
    dec = [ge.submit_decode(c) for c in given]
    if driver:
        for r in live + dec:
            assert ge.wait(r, WAIT_MS)
        ge.sched_stop()
    else:
        _drain(ge)
    got_live = [ge.result(r, want_pcm=True) for r in live]
    got_dec = [ge.result(r, want_pcm=True) for r in dec]
    stats = ge.decode_stats()
    ge.close()
    for g, w, (s, n) in zip(got_live, want_live, LIVE):                   # D2
        assert g["state"] == gpu.REQ_DONE and np.array_equal(g["codes"], w["codes"]), s
        _same_pcm(g["pcm"], w["pcm"], "live request %d" % s)
    for g, c, w, (s, n) in zip(got_dec, given, want_given, GIVEN):        # D1, beside them
        assert g["state"] == gpu.REQ_DONE and np.array_equal(g["codes"], c) and g["pcm"].size == n * takes.spf, s
        _same_pcm(g["pcm"], w, "decode-only request %d" % s)
    assert stats["requests"] == len(GIVEN) and stats["chunks"] == sum(-(-n // 4) for _, n in GIVEN)
    return stats


def test_beside_live_requests(gpu, tiny_model, takes):
    """3 sampled requests with PCM over 4 slots; 5 decode-only requests (frames of greedy takes of 4, 7, 8, 12 and 16 frames) arrive after the
    first frame group"""
    stats = _mixture(gpu, tiny_model, takes, driver=False)
    assert stats["chunks_shared"] > 0, stats


# ---------------------------------------------------------------- 4: no slot needed ----------------------------------------------------------------
def test_no_slot_needed(gpu, tiny_model, takes):
    ref = takes(60, 16)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=True)
    hold = [ge.submit(takes.prompt(90 + i), max_steps=24, seed=90 + i, mask_eos=True, want_pcm=False) for i in range(2)]
    waiting = ge.submit(takes.prompt(95), max_steps=4, seed=95, mask_eos=True, want_pcm=True)
    _steps(ge, 1)
    assert [ge.poll(r)["state"] for r in hold + [waiting]] == [gpu.REQ_RUNNING, gpu.REQ_RUNNING, gpu.REQ_QUEUED]
    rid = ge.submit_decode(ref["codes"][:4])
    for _ in range(4):                                                    # the holders need five more groups; the decode is one chunk and a fence
        _steps(ge, 1)
        if ge.poll(rid)["state"] == gpu.REQ_DONE:
            break
    assert ge.poll(rid)["state"] == gpu.REQ_DONE
    assert [ge.poll(r)["state"] for r in hold + [waiting]] == [gpu.REQ_RUNNING, gpu.REQ_RUNNING, gpu.REQ_QUEUED]
    out = ge.result(rid, want_pcm=True)
    _same_pcm(out["pcm"], ref["pcm"][:4 * takes.spf], "decode-only request beside a full engine")
    _drain(ge)
    w = ge.result(waiting, want_pcm=True)                                 # the one that waited for a slot is served as ever
    _same_pcm(w["pcm"], takes(95, 4)["pcm"], "the waiting request")
    assert np.array_equal(w["codes"], takes(95, 4)["codes"])
    for r in hold:
        assert ge.result(r)["codes"].shape == (24, 16)
    ge.close()


# ---------------------------------------------------------------- 5: more than decode_width ----------------------------------------------------------------
def test_more_requests_than_decode_width(gpu, tiny_model, takes):
    ref = takes(60, 16)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=16, load_codec=True)
    w = ge.decode_width()
    assert w == 2
    lens = [16, 12, 8, 16, 4][: 2 * w + 1]
    ids = [ge.submit_decode(ref["codes"][:n]) for n in lens]
    assert [ge.poll(r)["state"] for r in ids] == [gpu.REQ_QUEUED] * len(ids)
    most, order = 0, []
    for _ in range(4000):
        states = [ge.poll(r)["state"] for r in ids]
        most = max(most, states.count(gpu.REQ_DRAINING))
        assert states.count(gpu.REQ_DRAINING) <= w, states
        for i, s in enumerate(states):
            if s != gpu.REQ_QUEUED and i not in order:
                order.append(i)
        if all(s == gpu.REQ_DONE for s in states):
            break
        ge.sched_step()
    assert order == list(range(len(ids))) and most >= 1                   # admitted in submission order
    for r, n in zip(ids, lens):
        _same_pcm(ge.result(r, want_pcm=True)["pcm"], ref["pcm"][:n * takes.spf], "request of %d frames" % n)
    assert ge.decode_stats()["requests"] == len(ids) and not ge.sched_step()
    ge.close()


# ---------------------------------------------------------------- 6: cancel ----------------------------------------------------------------
def test_cancel_at_every_point(gpu, tiny_model, takes):
    ref = takes(60, 16)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=True)
    assert ge.decode_width() == 1
    holding, queued = ge.submit_decode(ref["codes"]), ge.submit_decode(ref["codes"][:8])
    _steps(ge, 1)
    assert [ge.poll(r)["state"] for r in (holding, queued)] == [gpu.REQ_DRAINING, gpu.REQ_QUEUED]
    # queued: CANCELLED at once, in this thread, with no PCM
    assert ge.cancel(queued) is True
    st = ge.poll(queued)
    assert (st["state"], st["n_frames"], st["n_pcm"]) == (gpu.REQ_CANCELLED, 8, 0)
    assert ge.cancel(queued) is False and ge.wait(queued, WAIT_MS)
    # holding a stream: the chunks already enqueued stay, the rest is purged, CANCELLED behind the fence
    assert ge.cancel(holding) is True
    _until(ge, lambda: ge.poll(holding)["state"] != gpu.REQ_DRAINING)
    st = ge.poll(holding)
    assert st["state"] == gpu.REQ_CANCELLED and st["n_pcm"] % (4 * takes.spf) == 0 and st["n_pcm"] <= 16 * takes.spf
    kept = ge.result(holding, want_pcm=True)
    assert kept["pcm"].size == st["n_pcm"] and _rms(kept["pcm"], ref["pcm"][:kept["pcm"].size]) < PCM_RMS_TOL
    assert ge.result(queued, want_pcm=True)["pcm"].size == 0
    # done: nothing changes
    done = ge.submit_decode(ref["codes"][:5])
    _until(ge, lambda: ge.poll(done)["state"] == gpu.REQ_DONE)
    assert ge.cancel(done) is False and ge.poll(done)["state"] == gpu.REQ_DONE
    assert ge.result(done, want_pcm=True)["pcm"].size == 5 * takes.spf
    assert not ge.sched_step()
    # the streams were reset and serve a generating request as a fresh engine would
    for seed in (61, 62):                                                 # both streams of the one-slot engine
        rid = ge.submit(takes.prompt(seed), max_steps=8, seed=seed, mask_eos=True, want_pcm=True)
        assert ge.wait(rid, WAIT_MS)
        g, w = ge.result(rid, want_pcm=True), takes(seed, 8)
        assert np.array_equal(g["codes"], w["codes"])
        _same_pcm(g["pcm"], w["pcm"], "generating request %d after the cancels" % seed)
    ge.close()


# ---------------------------------------------------------------- 7: refusals ----------------------------------------------------------------
def test_refusals(gpu, tiny_model, takes):
    ref = takes(60, 16)
    L = gpu.lib()
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=True)
    ok = np.ascontiguousarray(ref["codes"][:8], np.int32)

    def refused(codes, n, why, rid_null=False):
        rid = C.c_int64(-5)
        rc = L.q3tts_submit_decode(ge.h, gpu._p(codes) if codes is not None else None, n, None if rid_null else C.byref(rid))
        assert rc < 0 and why in L.q3tts_last_error() and rid.value == -5, (why, L.q3tts_last_error())

    def with_code(f, q, v):
        c = ok.copy()
        c[f, q] = v
        return c
    refused(None, 8, b"null argument")
    refused(ok, 8, b"null argument", rid_null=True)
    refused(ok, 0, b"n must be >= 1")
    refused(ok, -1, b"n must be >= 1")
    refused(np.ascontiguousarray(ref["codes"][:9], np.int32), 9, b"max_steps")
    refused(with_code(7, 0, CODEC_EOS), 8, b"EOS")
    refused(with_code(0, 0, SAMPLE_END), 8, b"code_0")
    refused(with_code(3, 0, -1), 8, b"code_0")
    refused(with_code(7, 15, 2048), 8, b"residual")
    refused(with_code(0, 1, -1), 8, b"residual")
    with pytest.raises(gpu.Q3Error, match="max_steps"):
        ge.submit_decode(ref["codes"][:9])
    assert ge.decode_stats() == dict(requests=0, chunks=0, chunks_shared=0) and not ge.sched_step()   # nothing was queued
    # the other calls on a decode-only request: nothing is recorded, there is no trail
    rid = ge.submit_decode(ok)                                            # n = max_steps is accepted
    assert L.q3tts_fetch_logprobs(ge.h, rid, None, 0, 0, None) < 0
    assert L.q3tts_trail_append(ge.h, rid, None, 0, 1) < 0
    na, nc, cl = C.c_int32(), C.c_int32(), C.c_int32()
    assert L.q3tts_trail_progress(ge.h, rid, C.byref(na), C.byref(nc), C.byref(cl)) < 0 and b"no trail" in L.q3tts_last_error()
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    _same_pcm(ge.result(rid, want_pcm=True)["pcm"], ref["pcm"][:8 * takes.spf], "n = max_steps")
    # after the refusals the engine serves a normal request
    r2 = ge.submit(takes.prompt(61), max_steps=8, seed=61, mask_eos=True, want_pcm=True)
    assert ge.wait(r2, WAIT_MS)
    g, w = ge.result(r2, want_pcm=True), takes(61, 8)
    assert np.array_equal(g["codes"], w["codes"])
    _same_pcm(g["pcm"], w["pcm"], "the request after the refusals")
    ge.close()
    # an engine without a codec refuses, and goes on generating codes
    nc_ = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    rid = C.c_int64(-5)
    assert L.q3tts_submit_decode(nc_.h, gpu._p(ok), 8, C.byref(rid)) < 0 and b"load_codec" in L.q3tts_last_error() and rid.value == -5
    assert nc_.decode_width() == 0 and not nc_.sched_step()
    r3 = nc_.submit(takes.prompt(61), max_steps=8, seed=61, mask_eos=True)
    assert nc_.wait(r3, WAIT_MS) and np.array_equal(nc_.result(r3)["codes"], w["codes"])
    nc_.close()


# ---------------------------------------------------------------- 8: the workflow ----------------------------------------------------------------
def test_codes_only_best_of_n_then_decode_the_winner(gpu, tiny_model, takes):
    seeds = [71, 72, 73]
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=16, load_codec=True)
    ge.set_logprobs(True)
    ids = ge.submit_candidates(takes.prompt(71), seeds, max_steps=16, mask_eos=True, want_pcm=False, **SAMPLED)
    _drain(ge)
    cands = [ge.result(r) for r in ids]
    calls = ge.stats()["codec_calls"]
    assert calls == 0 and all(c["pcm"] is None and c["codes"].shape == (16, 16) for c in cands)   # codes only: the codec did not run
    score = [float(np.sum(c["logprobs"][:, :16], dtype=np.float64)) for c in cands]
    best = int(np.argmax(score))
    out = _decode(ge, cands[best]["codes"], gpu)
    assert ge.stats()["codec_calls"] == 4                                 # one stream's worth of codec work, not three
    ge.close()
    w = takes(71, 16, sampled=True, seed=seeds[best])                     # the plain seeded submission with want_pcm = 1
    assert np.array_equal(w["codes"], cands[best]["codes"])
    _same_pcm(out["pcm"], w["pcm"], "the winner (seed %d)" % seeds[best])


# ---------------------------------------------------------------- 9: driver thread, group ----------------------------------------------------------------
def test_under_the_driver_thread(gpu, tiny_model, takes):
    _mixture(gpu, tiny_model, takes, driver=True)


def test_through_a_group_of_one_engine(gpu, tiny_model, takes):
    ref = takes(60, 16)
    L, q3 = gpu.lib(), gpu
    p = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 16, 1
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_poll.argtypes = [C.c_void_p, C.c_int64, C.POINTER(q3.ReqStatus)]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs, g = np.zeros(1, np.int32), C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(p), q3._p(devs), 1, C.byref(g)))
    try:
        for n, idx in ((16, -1), (6, 0)):
            rid = q3.group_submit_decode(g, idx, ref["codes"][:n])
            assert rid & 255 == 0 and L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            st = q3.ReqStatus()
            q3._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
            assert (st.state, st.n_frames, st.n_pcm) == (q3.REQ_DONE, n, n * takes.spf)
            codes, pcm, gf, gp = np.zeros(16 * 16, np.int32), np.zeros(st.n_pcm, np.float32), C.c_int32(), C.c_int64()
            q3._chk(L.q3tts_group_fetch(g, rid, q3._p(codes), 0, 16, q3._p(pcm), 0, pcm.size, C.byref(gf), C.byref(gp)))
            assert gf.value == n and gp.value == pcm.size and np.array_equal(codes[:n * 16].reshape(n, 16), ref["codes"][:n])
            if n == 16:
                _same_pcm(pcm, ref["pcm"], "through the group")
            else:                                                         # a chunk and a 2-frame tail: the first chunk is the take's
                _same_pcm(pcm[:4 * takes.spf], ref["pcm"][:4 * takes.spf], "through the group, first chunk")
            q3._chk(L.q3tts_group_release(g, rid))
        with pytest.raises(q3.Q3Error, match="engine_index"):
            q3.group_submit_decode(g, 1, ref["codes"])
        rid = C.c_int64(-5)
        assert L.q3tts_group_submit_decode(g, -1, None, 4, C.byref(rid)) < 0 and rid.value == -5
    finally:
        L.q3tts_group_destroy(g)
