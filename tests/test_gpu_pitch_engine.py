"""[EXT] pitch through the engine (q3tts_engine_set_pitch, q3tts_request_pitch, q3tts_engine_pitch_stats and the group forms;
include/q3tts_spec.h "pitch").  The codes of a request never depend on its pitch; its sample counts are the closed forms while it streams
and at its end; and its PCM is q3tts_op_pitch of the PCM the same request delivers with the pitch off, judged under the kernel test's
derived bound with that run's trace: sum |h32| bz + gamma(K + 1) sum |h32 z64| + 2^-149 (plus half a step for int16).  Tiny model, Q8_0,
max_steps <= 24.  The scheduler is stepped by hand and every wait is bounded.  A request's native take is a second run on the same engine with
the pitch off -- alone where the request ran alone, side by side where it ran side by side -- so that both runs decode the same chunks at
the same width."""
import ctypes as C

import numpy as np
import pytest

import pitch_ref as R

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
WAIT_MS = 60000.0
SPF = 1920
NO_PITCH = dict(chunks=0, samples_out=0, flushes=0, table_bytes=0)


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


def _prompt(ge, vivian, seed, n=8):
    rng = np.random.default_rng(seed)
    return ge.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


class Takes:
    """take(p, n, **kw): the request of prompt p run natively (no rate, no pitch) with PCM on the given engine for exactly n frames
    (mask_eos); together([...]) runs several side by side"""

    def __init__(self, gpu, ge, vivian):
        self.gpu, self.ge, self.vivian, self.memo = gpu, ge, vivian, {}

    def prompt(self, p):
        return _prompt(self.ge, self.vivian, p)

    def together(self, jobs):
        rids = []
        for p, n, kw in jobs:
            kw = dict(kw)
            kw.setdefault("seed", p)
            rids.append(self.ge.submit(self.prompt(p), max_steps=n, mask_eos=True, want_pcm=True, **kw))
        assert all(self.ge.request_pitch(r) == 100 and self.ge.request_speech_rate(r) == 100 for r in rids)
        _until(self.ge, lambda: all(self.ge.poll(r)["state"] == self.gpu.REQ_DONE for r in rids))
        out = [self.ge.result(r, want_pcm=True) for r in rids]
        for r, (p, n, kw) in zip(out, jobs):
            assert r["codes"].shape == (n, 16) and r["pcm"].size == n * SPF and r["pcm"].dtype == np.float32
            r["codes"].setflags(write=False), r["pcm"].setflags(write=False)
        return out

    def __call__(self, p, n, **kw):
        key = (p, n, tuple(sorted((k, tuple(v) if hasattr(v, "__len__") else v) for k, v in kw.items())))
        if key not in self.memo:
            self.memo[key] = self.together([(p, n, kw)])[0]
        return self.memo[key]


@pytest.fixture(scope="module")
def eng3(gpu, tiny_model):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=3, max_steps=24, load_codec=True)
    yield ge
    ge.close()


@pytest.fixture(scope="module")
def takes(gpu, eng3, vivian):
    return Takes(gpu, eng3, vivian)


def _check(gpu, got, native, Rt, P, enc, what, final=True):
    """count, dtype and the bound of one delivered stream against q3tts_op_pitch of the native take"""
    native = np.asarray(native, np.float32)
    assert got.dtype == (np.int16 if enc else np.float32), what
    assert got.size == gpu.pitch_samples(Rt, P, native.size, final) == R.n_samples(Rt, P, native.size, final), (what, got.size)
    rms_native = float(np.sqrt(np.mean(native.astype(np.float64) ** 2)))
    assert rms_native >= 1e-3, "%s: the native take is silent (rms %.3e): the check would be vacuous" % (what, rms_native)
    outs, traces, _, _, _, _, _ = gpu.op_pitch(native[None, :], [native.size], [[0]], 1, [Rt], [P], [enc], flush=final)
    y, bound, _, _ = R.pitch(native, Rt, P, final=final, deltas=traces[0])
    scale = 32767.0 if enc else 1.0
    err = np.abs(got.astype(np.float64) - y * scale)
    lim = bound * scale + (0.5 if enc else 0.0)
    print("%s: rate %d pitch %d %s, %d samples, native rms %.3e, max err / bound %.3g, equal to the kernel's own run: %s"
          % (what, Rt, P, "s16" if enc else "f32", got.size, rms_native, (err / lim).max(), np.array_equal(got, outs[0])))
    assert np.all(err <= lim), "%s: %.3g of the bound" % (what, (err / lim).max())


def _run(ge, gpu, prompt, n, Rt, P, enc, **kw):
    ge.set_output_format(24000, enc)
    ge.set_speech_rate(Rt)
    ge.set_pitch(P)
    rid = ge.submit(prompt, max_steps=n, mask_eos=True, want_pcm=True, **kw)
    ge.set_pitch(100)
    ge.set_speech_rate(100)
    ge.set_output_format(None)
    assert ge.request_pitch(rid) == P and ge.request_speech_rate(rid) == Rt and ge.request_format(rid) == (24000, enc)
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    return ge.result(rid, want_pcm=True)


# -------------------------------------------------------- 1: per request, streamed --------------------------------------------------------
@pytest.mark.parametrize("Rt,P,enc,n", [(100, 107, 0, 10), (125, 80, 1, 11)])
def test_generated_request_with_a_pitch(gpu, eng3, takes, Rt, P, enc, n):
    ref = takes(60 + P, n)
    s0 = eng3.pitch_stats()
    eng3.set_output_format(24000, enc)
    eng3.set_speech_rate(Rt)
    eng3.set_pitch(P)
    rid = eng3.submit(takes.prompt(60 + P), max_steps=n, seed=60 + P, mask_eos=True, want_pcm=True)
    eng3.set_pitch(100)
    eng3.set_speech_rate(100)
    eng3.set_output_format(None)
    fetch = (lambda off, cap: eng3.fetch_pcm16(rid, off, cap)) if enc else (lambda off, cap: eng3.fetch(rid, 0, 0, off, cap)[1])
    total = gpu.pitch_samples(Rt, P, n * SPF, True)
    allowed = {gpu.pitch_samples(Rt, P, f * SPF, False) for f in range(n + 1)} | {total}
    seen, part = [0], None
    for _ in range(4000):
        st = eng3.poll(rid)
        assert st["n_pcm"] >= seen[-1] and st["n_pcm"] in allowed          # delivered samples: what N native samples have made
        if st["n_pcm"] != seen[-1]:
            seen.append(st["n_pcm"])
            part = fetch(0, st["n_pcm"])                                   # what is there can be fetched while the request runs
            assert part.size == st["n_pcm"]
        if st["state"] == gpu.REQ_DONE:
            break
        eng3.sched_step()
    L, M, _, _ = R.plan(P)
    assert seen[-1] == total == -(-480 * -(-P * n * SPF // (480 * Rt)) * L // M)
    whole = fetch(0, total)
    assert np.array_equal(whole[: part.size], part)
    for off, cap in ((1, 7), (479, 3), (480, 481), (total - 1, 50), (total, 5), (0, total + 1000)):
        assert np.array_equal(fetch(off, cap), whole[off: off + cap]), (off, cap)
    r = eng3.result(rid, want_pcm=True)
    assert r["sample_rate"] == 24000 and r["n_pcm"] == total and np.array_equal(r["pcm"], whole)
    assert np.array_equal(r["codes"], ref["codes"])                        # the pitch never reaches the talker
    _check(gpu, whole, ref["pcm"], Rt, P, enc, "generated")
    s1 = eng3.pitch_stats()
    assert s1["chunks"] - s0["chunks"] == -(-n // 4) and s1["samples_out"] - s0["samples_out"] == total and s1["flushes"] - s0["flushes"] == 1
    assert s1["table_bytes"] == 366999 * 4                                 # all 151 tables, uploaded once


# -------------------------------------------------------- 2: the other submit forms --------------------------------------------------------
def test_streaming_text_request(gpu, eng3, takes):
    ids = [11, 22, 33, 44, 55, 66]
    ref = takes(70, 9, trailing_ids=ids)
    r = _run(eng3, gpu, takes.prompt(70), 9, 100, 89, 0, seed=70, trailing_ids=ids)
    assert np.array_equal(r["codes"], ref["codes"])
    _check(gpu, r["pcm"], ref["pcm"], 100, 89, 0, "streaming text")


def test_decode_only_and_resumed_requests(gpu, eng3, takes):
    ref = takes(71, 10)
    eng3.set_pitch(120)
    eng3.set_speech_rate(90)
    rid = eng3.submit_decode(ref["codes"])
    eng3.set_speech_rate(100)
    eng3.set_pitch(100)
    assert eng3.request_pitch(rid) == 120 and eng3.request_speech_rate(rid) == 90
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_DONE)
    dec = eng3.result(rid, want_pcm=True)
    _check(gpu, dec["pcm"], ref["pcm"], 90, 120, 0, "decode-only")
    res = _run(eng3, gpu, takes.prompt(71), 10, 100, 107, 1, seed=71, prefix_codes=ref["codes"][:5])
    assert np.array_equal(res["codes"], ref["codes"])
    _check(gpu, res["pcm"], ref["pcm"], 100, 107, 1, "resumed")            # count and check as the uninterrupted request


def test_candidate_set(gpu, eng3, takes):
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    rids = eng3.submit_candidates(takes.prompt(72), [1, 2, 3], max_steps=5, want_pcm=True, **kw)   # the same set, natively
    _until(eng3, lambda: all(eng3.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    refs = [eng3.result(x, want_pcm=True) for x in rids]
    assert all(r["pcm"].size == 5 * SPF for r in refs)
    eng3.set_pitch(80)
    rids = eng3.submit_candidates(takes.prompt(72), [1, 2, 3], max_steps=5, want_pcm=True, **kw)
    eng3.set_pitch(100)
    _until(eng3, lambda: all(eng3.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    for seed, x, ref in zip((1, 2, 3), rids, refs):
        assert eng3.request_pitch(x) == 80 and eng3.request_speech_rate(x) == 100   # read once per set
        o = eng3.result(x, want_pcm=True)
        assert np.array_equal(o["codes"], ref["codes"])
        _check(gpu, o["pcm"], ref["pcm"], 100, 80, 0, "candidate %d" % seed)
    _drain(eng3)


def test_group_of_two_engines_on_one_device(gpu, tiny_model, takes):
    codes = takes(71, 10)["codes"]
    L = gpu.lib()
    p = gpu.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 16, 1
    L.q3tts_group_create.argtypes = [C.POINTER(gpu.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_poll.argtypes = [C.c_void_p, C.c_int64, C.POINTER(gpu.ReqStatus)]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs, g = np.zeros(2, np.int32), C.c_void_p()
    gpu._chk(L.q3tts_group_create(C.byref(p), gpu._p(devs), 2, C.byref(g)))
    try:
        for bad in (49, 201):
            with pytest.raises(gpu.Q3Error, match="range"):
                gpu.group_set_pitch(g, bad)
        def decode(idx, n=10):
            rid = gpu.group_submit_decode(g, idx, codes[:n])
            assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            return rid

        def fetch(rid, total):
            buf, gp = np.zeros(total, np.float32), C.c_int64()
            gpu._chk(L.q3tts_group_fetch(g, rid, None, 0, 0, gpu._p(buf), 0, total, None, C.byref(gp)))
            assert gp.value == total
            gpu._chk(L.q3tts_group_release(g, rid))
            return buf

        native = [fetch(decode(idx), 10 * SPF) for idx in (0, 1)]           # each engine's own native take
        gpu.group_set_pitch(g, 107)
        total = gpu.pitch_samples(100, 107, 10 * SPF, True)
        for idx in (0, 1):                                                  # both engines took the pitch
            rid = decode(idx)
            st = gpu.ReqStatus()
            gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
            assert (st.state, st.n_frames, st.n_pcm) == (gpu.REQ_DONE, 10, total)
            assert gpu.group_request_pitch(g, rid) == 107 and gpu.group_request_speech_rate(g, rid) == 100
            _check(gpu, fetch(rid, total), native[idx], 100, 107, 0, "group engine %d" % idx)
        gpu.group_set_pitch(g, 100)
        rid = decode(0, 4)
        assert gpu.group_request_pitch(g, rid) == 100
        st = gpu.ReqStatus()
        gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
        assert st.n_pcm == 4 * SPF
        gpu._chk(L.q3tts_group_release(g, rid))
    finally:
        L.q3tts_group_destroy(g)


# -------------------------------------------------------- 3: cancel, preamble --------------------------------------------------------
def test_a_cancelled_request_keeps_what_was_delivered_and_is_not_flushed(gpu, eng3, takes):
    ref = takes(73, 23)
    s0 = eng3.pitch_stats()
    eng3.set_output_format(24000, gpu.PCM_S16)
    eng3.set_pitch(107)
    rid = eng3.submit(takes.prompt(73), max_steps=23, seed=73, mask_eos=True, want_pcm=True)
    eng3.set_pitch(100)
    eng3.set_output_format(None)
    _until(eng3, lambda: eng3.poll(rid)["n_frames"] >= 9 and eng3.poll(rid)["n_pcm"] >= gpu.pitch_samples(100, 107, 4 * SPF, False))
    assert eng3.cancel(rid)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_CANCELLED)
    r = eng3.result(rid, want_pcm=True)
    streamed = {gpu.pitch_samples(100, 107, f * SPF, False): f for f in list(range(4, 24, 4)) + [23]}
    assert r["n_pcm"] in streamed and r["pcm"].size == r["n_pcm"]           # whole chunks' samples, no flush
    f = streamed[r["n_pcm"]]
    assert r["n_pcm"] < gpu.pitch_samples(100, 107, f * SPF, True)
    assert np.array_equal(r["codes"], ref["codes"][: r["codes"].shape[0]])
    _check(gpu, r["pcm"], ref["pcm"][: f * SPF], 100, 107, 1, "cancelled", final=False)
    assert eng3.pitch_stats()["flushes"] == s0["flushes"]
    _drain(eng3)


def test_a_primed_request_starts_both_stages_from_a_reset(gpu, tiny_model, vivian, takes):
    pre = np.ascontiguousarray(takes(74, 9)["codes"])
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        ge.set_pitch(120)                                                 # a preamble build is never shifted
        pid = ge.preamble_create(pre)
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, 9)
        assert ge.pitch_stats() == NO_PITCH
        ge.set_pitch(100)
        prompt = _prompt(ge, vivian, 75)
        ge.set_preamble(pid)
        rid = ge.submit(prompt, max_steps=10, seed=75, mask_eos=True, want_pcm=True)
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        native = ge.result(rid, want_pcm=True)                            # the primed request, natively
        ge.set_pitch(120)
        ge.set_speech_rate(90)
        rid = ge.submit(prompt, max_steps=10, seed=75, mask_eos=True, want_pcm=True)
        ge.set_speech_rate(100)
        ge.set_pitch(100)
        ge.set_preamble(None)
        assert ge.request_preamble(rid) == pid and ge.request_pitch(rid) == 120
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        assert np.array_equal(r["codes"], native["codes"])
        _check(gpu, r["pcm"], native["pcm"], 90, 120, 0, "primed")         # the reference starts from zeros: so did both stages
    finally:
        ge.close()


# -------------------------------------------------------- 4: 100 is off; side by side --------------------------------------------------------
def test_pitch_100_is_an_ordinary_request_and_a_rate_alone_is_the_speaking_rate(gpu, tiny_model, vivian):
    plain = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)   # an engine that never hears of pitch
    takes = Takes(gpu, plain, vivian)
    ref = takes(76, 6)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        ge.set_pitch(100)
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=True)
        assert ge.request_pitch(rid) == 100
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        assert np.array_equal(r["codes"], ref["codes"])
        assert np.array_equal(r["pcm"].view(np.uint32), ref["pcm"].view(np.uint32))   # the bits of an engine that never heard of pitch
        ge.set_speech_rate(125)                                            # a rate alone: the stretcher's request, bit for bit
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=True)
        ge.set_speech_rate(100)
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        outs, _, _, _, _, _ = gpu.op_tsm(np.asarray(ref["pcm"])[None, :], [4 * SPF, 2 * SPF], [[0], [0]], 1, [125], [0], flush=True)
        assert np.array_equal(r["pcm"].view(np.uint32), outs[0].view(np.uint32)) and ge.tsm_stats()["flushes"] == 1
        ge.set_pitch(107)                                                  # not shifted: no PCM wanted, scoring
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=False)
        sid = ge.submit_score(takes.prompt(76), ref["codes"])
        assert ge.request_pitch(rid) == 100 and ge.request_pitch(sid) == 100
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE and ge.poll(sid)["state"] == gpu.REQ_DONE)
        assert np.array_equal(ge.result(rid)["codes"], ref["codes"]) and ge.poll(sid)["n_pcm"] == 0
        ge.release(sid)
        assert ge.pitch_stats() == NO_PITCH
        with pytest.raises(gpu.Q3Error, match="unknown request id"):
            ge.request_pitch(rid)
        assert plain.pitch_stats() == NO_PITCH
    finally:
        ge.close()
        plain.close()


def test_three_pitches_side_by_side(gpu, eng3, takes):
    refs = takes.together([(77 + i, 8, {}) for i in range(3)])             # the same three side by side, natively
    rates, pitches, encs = [100, 100, 150], [89, 137, 75], [0, 1, 0]
    rids = []
    for i, (Rt, P, enc) in enumerate(zip(rates, pitches, encs)):
        eng3.set_output_format(24000, enc)
        eng3.set_speech_rate(Rt)
        eng3.set_pitch(P)
        rids.append(eng3.submit(takes.prompt(77 + i), max_steps=8, seed=77 + i, mask_eos=True, want_pcm=True))
    eng3.set_pitch(100)
    eng3.set_speech_rate(100)
    eng3.set_output_format(None)
    assert [eng3.request_pitch(r) for r in rids] == pitches and [eng3.request_speech_rate(r) for r in rids] == rates
    _until(eng3, lambda: all(eng3.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [eng3.result(r, want_pcm=True) for r in rids]
    for o, ref in zip(out, refs):
        assert np.array_equal(o["codes"], ref["codes"])
    assert [o["n_pcm"] for o in out] == [gpu.pitch_samples(a, b, 8 * SPF, True) for a, b in zip(rates, pitches)]
    for o, ref, Rt, P, enc in zip(out, refs, rates, pitches, encs):
        _check(gpu, o["pcm"], ref["pcm"], Rt, P, enc, "side by side, %d / %d" % (Rt, P))


# -------------------------------------------------------- 5: refusals --------------------------------------------------------
def test_refusals(gpu, tiny_model, eng3, takes):
    for P in (49, 201):
        with pytest.raises(gpu.Q3Error, match="range"):
            eng3.set_pitch(P)
    rid = eng3.submit(takes.prompt(80), max_steps=1, seed=80, mask_eos=True, want_pcm=True)   # a refused call changed nothing
    assert eng3.request_pitch(rid) == 100
    forms = (lambda: eng3.submit(takes.prompt(80), max_steps=4, seed=80, mask_eos=True, want_pcm=True),
             lambda: eng3.submit_decode(takes(71, 10)["codes"]),
             lambda: eng3.submit_candidates(takes.prompt(80), [1, 2], max_steps=4, want_pcm=True))
    eng3.set_speech_rate(50)                                               # each value is in range, the pair is not: judged at submit
    eng3.set_pitch(101)
    for submit in forms:
        with pytest.raises(gpu.Q3Error, match="1/2, 2"):
            submit()
    eng3.set_speech_rate(100)
    eng3.set_pitch(107)
    eng3.set_output_format(16000, gpu.PCM_S16)                             # a resampled format and a pitch do not combine
    for submit in forms:
        with pytest.raises(gpu.Q3Error, match="24000"):
            submit()
    eng3.set_output_format(None)
    eng3.set_speech_rate(50)                                               # f32 at (50, 50): twice the native bytes and a hop
    eng3.set_pitch(50)
    with pytest.raises(gpu.Q3Error, match="staging"):
        eng3.submit(takes.prompt(80), max_steps=24, seed=80, mask_eos=True, want_pcm=True)
    ok = eng3.submit(takes.prompt(80), max_steps=11, seed=80, mask_eos=True, want_pcm=True)
    eng3.set_pitch(100)
    eng3.set_speech_rate(100)
    _until(eng3, lambda: all(eng3.poll(r)["state"] == gpu.REQ_DONE for r in (rid, ok)))   # nothing else was queued
    assert eng3.poll(ok)["n_pcm"] == gpu.pitch_samples(50, 50, 11 * SPF, True)
    assert ok == rid + 1                                                   # request ids are handed out at the queue: no refused submit took one
    for r in (rid, ok):
        eng3.release(r)
    _drain(eng3)
    bare = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    for P in (107, 100):
        with pytest.raises(gpu.Q3Error, match="codec"):
            bare.set_pitch(P)
    assert bare.pitch_stats() == NO_PITCH
    bare.close()
