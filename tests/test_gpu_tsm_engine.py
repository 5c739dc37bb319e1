"""[EXT] speaking rate through the engine (q3tts_engine_set_speech_rate, q3tts_request_speech_rate, q3tts_engine_tsm_stats and the group
forms; include/q3tts_spec.h "speaking rate").  The codes of a request never depend on its rate; its sample count is the closed form; and
its PCM is explained, hop by hop, by the PCM the same request delivers natively: tests/tsm_ref.py explain() finds a candidate for every
hop whose overlap-add reproduces the delivered hop within the standing PCM tolerance of 1e-4 RMS (1.1e-4 for int16), and whose float64
cost is within 2e of the least cost, e = 8 tau sqrt(480), tau = 1e-4 -- the kernel minimised the cost over PCM that may differ from the
native take by the standing tolerance, and the factor 4 over 2 tau sqrt(480) covers local versus global RMS.  Tiny model, Q8_0,
max_steps <= 24.  The scheduler is stepped by hand and every wait is bounded.  Native takes come from a one-slot engine."""
import ctypes as C

import numpy as np
import pytest

import tsm_ref as R

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
S16_RMS_TOL = 1.1e-4          # 1e-4 and 1 / (32767 sqrt(12)) = 8.8e-6 of quantisation noise, summed
TAU = 1e-4
E = 8 * TAU * np.sqrt(480.0)
WAIT_MS = 60000.0
SPF = 1920


def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


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
    """take(p, n, **kw): the request of prompt p run alone, natively, with PCM on a one-slot engine for exactly n frames (mask_eos)"""

    def __init__(self, gpu, model, vivian):
        self.ge = gpu.Engine(model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
        self.vivian, self.memo = vivian, {}

    def prompt(self, p):
        return _prompt(self.ge, self.vivian, p)

    def __call__(self, p, n, **kw):
        key = (p, n, tuple(sorted((k, tuple(v) if hasattr(v, "__len__") else v) for k, v in kw.items())))
        if key not in self.memo:
            kw.setdefault("seed", p)
            rid = self.ge.submit(self.prompt(p), max_steps=n, mask_eos=True, want_pcm=True, **kw)
            assert self.ge.wait(rid, WAIT_MS)
            assert self.ge.request_speech_rate(rid) == 100
            r = self.ge.result(rid, want_pcm=True)
            assert r["state"] == 3 and r["codes"].shape == (n, 16) and r["pcm"].size == n * SPF and r["pcm"].dtype == np.float32
            r["codes"].setflags(write=False), r["pcm"].setflags(write=False)
            self.memo[key] = r
        return self.memo[key]


@pytest.fixture(scope="module")
def takes(gpu, tiny_model, vivian):
    t = Takes(gpu, tiny_model, vivian)
    yield t
    assert t.ge.tsm_stats() == dict(chunks=0, frames_out=0, flushes=0)   # an engine that never had a rate never ran the stretcher
    t.ge.close()


@pytest.fixture(scope="module")
def eng3(gpu, tiny_model):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=3, max_steps=24, load_codec=True)
    yield ge
    ge.close()


def _check(gpu, got, native, pct, enc, what, final=True):
    """count, dtype and the explain check of one delivered stream against the native take"""
    native = np.asarray(native)
    assert got.dtype == (np.int16 if enc else np.float32), what
    if final:
        assert got.size == gpu.tsm_samples(pct, native.size, True) == R.n_samples(pct, native.size, True), (what, got.size)
    rms_native = float(np.sqrt(np.mean(native.astype(np.float64) ** 2)))
    assert rms_native >= 1e-3, "%s: the native take is silent (rms %.3e): the check would be vacuous" % (what, rms_native)
    y = got.astype(np.float64) / 32767.0 if enc else got.astype(np.float64)
    ex = R.explain(native, y, pct, final=final)
    resid = _rms(ex["recon"], y)
    slack = np.sqrt(ex["ssd_p"]) - np.sqrt(ex["ssd_min"])
    print("%s: pct %d %s, %d hops, native rms %.3e, residual rms %.3e, worst cost slack %.3e (2e = %.3e)"
          % (what, pct, "s16" if enc else "f32", ex["p"].size, rms_native, resid, slack.max() if slack.size else 0.0, 2 * E))
    assert np.all(ex["p"] >= 0) and np.all(np.abs(ex["p"] - np.array([R.a_of(pct, k) for k in range(ex["p"].size)])) <= R.SEARCH)
    assert resid <= (S16_RMS_TOL if enc else PCM_RMS_TOL), "%s: residual rms %.3e" % (what, resid)
    assert np.all(slack <= 2 * E), "%s: a hop's cost is %.3e above the least" % (what, slack.max())
    return ex


def _run(ge, gpu, prompt, n, pct, enc, **kw):
    ge.set_output_format(24000, enc)
    ge.set_speech_rate(pct)
    rid = ge.submit(prompt, max_steps=n, mask_eos=True, want_pcm=True, **kw)
    ge.set_speech_rate(100)
    ge.set_output_format(None)
    assert ge.request_speech_rate(rid) == pct and ge.request_format(rid) == (24000, enc)
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    return ge.result(rid, want_pcm=True)


# -------------------------------------------------------- 1: per request, streamed --------------------------------------------------------
@pytest.mark.parametrize("pct,enc,n", [(50, 0, 10), (80, 1, 11), (125, 0, 10), (200, 1, 9)])
def test_generated_request_at_a_rate(gpu, eng3, takes, pct, enc, n):
    ref = takes(60 + pct, n)
    s0 = eng3.tsm_stats()
    eng3.set_output_format(24000, enc)
    eng3.set_speech_rate(pct)
    rid = eng3.submit(takes.prompt(60 + pct), max_steps=n, seed=60 + pct, mask_eos=True, want_pcm=True)
    eng3.set_speech_rate(100)
    eng3.set_output_format(None)
    fetch = (lambda off, cap: eng3.fetch_pcm16(rid, off, cap)) if enc else (lambda off, cap: eng3.fetch(rid, 0, 0, off, cap)[1])
    allowed = {gpu.tsm_samples(pct, f * SPF, False) for f in range(n + 1)} | {gpu.tsm_samples(pct, n * SPF, True)}
    seen, part = [0], None
    for _ in range(4000):
        st = eng3.poll(rid)
        assert st["n_pcm"] >= seen[-1] and st["n_pcm"] % 480 == 0 and st["n_pcm"] in allowed   # delivered samples: whole hops
        if st["n_pcm"] != seen[-1]:
            seen.append(st["n_pcm"])
            part = fetch(0, st["n_pcm"])                                  # what is there can be fetched while the request runs
            assert part.size == st["n_pcm"]
        if st["state"] == gpu.REQ_DONE:
            break
        eng3.sched_step()
    total = gpu.tsm_samples(pct, n * SPF, True)
    assert seen[-1] == total == 480 * -(-100 * n * SPF // (480 * pct))
    whole = fetch(0, total)
    assert np.array_equal(whole[: part.size], part)
    for off, cap in ((1, 7), (479, 3), (480, 481), (total - 1, 50), (total, 5), (0, total + 1000)):
        assert np.array_equal(fetch(off, cap), whole[off: off + cap]), (off, cap)
    with pytest.raises(gpu.Q3Error, match="int16" if enc else "f32"):
        (eng3.fetch(rid, 0, 0, 0, 16) if enc else eng3.fetch_pcm16(rid, 0, 16))
    r = eng3.result(rid, want_pcm=True)
    assert r["sample_rate"] == 24000 and r["n_pcm"] == total and np.array_equal(r["pcm"], whole)
    assert np.array_equal(r["codes"], ref["codes"])                       # the rate never reaches the talker
    _check(gpu, whole, ref["pcm"], pct, enc, "generated")
    s1 = eng3.tsm_stats()
    assert s1["chunks"] - s0["chunks"] == -(-n // 4) and s1["frames_out"] - s0["frames_out"] == total // 480 and s1["flushes"] - s0["flushes"] == 1


# -------------------------------------------------------- 2: the other submit forms --------------------------------------------------------
def test_streaming_text_request(gpu, eng3, takes):
    ids = [11, 22, 33, 44, 55, 66]
    ref = takes(70, 9, trailing_ids=ids)
    r = _run(eng3, gpu, takes.prompt(70), 9, 125, 0, seed=70, trailing_ids=ids)
    assert np.array_equal(r["codes"], ref["codes"])
    _check(gpu, r["pcm"], ref["pcm"], 125, 0, "streaming text")


def test_decode_only_and_resumed_requests(gpu, eng3, takes):
    ref = takes(71, 10)
    eng3.set_speech_rate(80)
    rid = eng3.submit_decode(ref["codes"])
    eng3.set_speech_rate(100)
    assert eng3.request_speech_rate(rid) == 80
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_DONE)
    dec = eng3.result(rid, want_pcm=True)
    _check(gpu, dec["pcm"], ref["pcm"], 80, 0, "decode-only")
    res = _run(eng3, gpu, takes.prompt(71), 10, 125, 1, seed=71, prefix_codes=ref["codes"][:5])
    assert np.array_equal(res["codes"], ref["codes"])
    _check(gpu, res["pcm"], ref["pcm"], 125, 1, "resumed")               # count and check as the uninterrupted request


def test_candidate_set(gpu, eng3, takes):
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    eng3.set_speech_rate(80)
    rids = eng3.submit_candidates(takes.prompt(72), [1, 2, 3], max_steps=5, want_pcm=True, **kw)
    eng3.set_speech_rate(100)
    _until(eng3, lambda: all(eng3.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    for seed, x in zip((1, 2, 3), rids):
        assert eng3.request_speech_rate(x) == 80
        o = eng3.result(x, want_pcm=True)
        ref = takes(72, 5, seed=seed, **kw)
        assert np.array_equal(o["codes"], ref["codes"])
        _check(gpu, o["pcm"], ref["pcm"], 80, 0, "candidate %d" % seed)
    _drain(eng3)


def test_group_of_two_engines_on_one_device(gpu, tiny_model, takes):
    ref = takes(71, 10)
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
                gpu.group_set_speech_rate(g, bad)
        gpu.group_set_speech_rate(g, 125)
        total = gpu.tsm_samples(125, 10 * SPF, True)
        for idx in (0, 1):                                                  # both engines took the rate
            rid = gpu.group_submit_decode(g, idx, ref["codes"])
            assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            st = gpu.ReqStatus()
            gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
            assert (st.state, st.n_frames, st.n_pcm) == (gpu.REQ_DONE, 10, total)
            assert gpu.group_request_speech_rate(g, rid) == 125
            buf, gp = np.zeros(total, np.float32), C.c_int64()
            gpu._chk(L.q3tts_group_fetch(g, rid, None, 0, 0, gpu._p(buf), 0, total, None, C.byref(gp)))
            assert gp.value == total
            _check(gpu, buf, ref["pcm"], 125, 0, "group engine %d" % idx)
            gpu._chk(L.q3tts_group_release(g, rid))
        gpu.group_set_speech_rate(g, 100)
        rid = gpu.group_submit_decode(g, 0, ref["codes"][:4])
        assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0 and gpu.group_request_speech_rate(g, rid) == 100
        st = gpu.ReqStatus()
        gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
        assert st.n_pcm == 4 * SPF
        gpu._chk(L.q3tts_group_release(g, rid))
    finally:
        L.q3tts_group_destroy(g)


# -------------------------------------------------------- 3: cancel, preamble --------------------------------------------------------
def test_a_cancelled_request_keeps_whole_hops_and_is_not_flushed(gpu, eng3, takes):
    ref = takes(73, 24)
    s0 = eng3.tsm_stats()
    eng3.set_output_format(24000, gpu.PCM_S16)
    eng3.set_speech_rate(80)
    rid = eng3.submit(takes.prompt(73), max_steps=24, seed=73, mask_eos=True, want_pcm=True)
    eng3.set_speech_rate(100)
    eng3.set_output_format(None)
    _until(eng3, lambda: eng3.poll(rid)["n_frames"] >= 9 and eng3.poll(rid)["n_pcm"] >= gpu.tsm_samples(80, 4 * SPF, False))
    assert eng3.cancel(rid)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_CANCELLED)
    r = eng3.result(rid, want_pcm=True)
    streamed = {gpu.tsm_samples(80, f * SPF, False): f for f in range(4, 25, 4)}
    assert r["n_pcm"] in streamed and r["n_pcm"] % 480 == 0 and r["pcm"].size == r["n_pcm"]      # whole chunks' whole hops, no flush
    assert r["n_pcm"] < gpu.tsm_samples(80, streamed[r["n_pcm"]] * SPF, True)
    assert np.array_equal(r["codes"], ref["codes"][: r["codes"].shape[0]])
    _check(gpu, r["pcm"], ref["pcm"], 80, 1, "cancelled", final=False)
    assert eng3.tsm_stats()["flushes"] == s0["flushes"]
    _drain(eng3)


def test_a_primed_request_starts_its_stretcher_from_a_reset(gpu, tiny_model, vivian, takes):
    pre = np.ascontiguousarray(takes(74, 9)["codes"])
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        pid = ge.preamble_create(pre)
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, 9)
        assert ge.tsm_stats() == dict(chunks=0, frames_out=0, flushes=0)  # a preamble build is never stretched
        prompt = _prompt(ge, vivian, 75)
        ge.set_preamble(pid)
        rid = ge.submit(prompt, max_steps=10, seed=75, mask_eos=True, want_pcm=True)
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        native = ge.result(rid, want_pcm=True)                            # the primed request, natively
        ge.set_speech_rate(50)
        with pytest.raises(gpu.Q3Error, match="staging"):                 # a preamble build ignores the rate, a request does not
            ge.submit(prompt, max_steps=13, seed=75, mask_eos=True, want_pcm=True)
        ge.set_speech_rate(125)
        rid = ge.submit(prompt, max_steps=10, seed=75, mask_eos=True, want_pcm=True)
        ge.set_speech_rate(100)
        ge.set_preamble(None)
        assert ge.request_preamble(rid) == pid and ge.request_speech_rate(rid) == 125
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        assert np.array_equal(r["codes"], native["codes"])
        _check(gpu, r["pcm"], native["pcm"], 125, 0, "primed")
    finally:
        ge.close()


# -------------------------------------------------------- 4: 100 is off; side by side --------------------------------------------------------
def test_rate_100_is_an_ordinary_request(gpu, tiny_model, takes):
    ref = takes(76, 6)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=True)
    try:
        ge.set_speech_rate(100)
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=True)
        assert ge.request_speech_rate(rid) == 100
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        assert np.array_equal(r["codes"], ref["codes"]) and r["pcm"].dtype == np.float32
        assert r["pcm"].size == ref["pcm"].size and _rms(r["pcm"], ref["pcm"]) < PCM_RMS_TOL
        ge.set_speech_rate(125)                                           # not stretched: no PCM wanted, scoring
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=False)
        sid = ge.submit_score(takes.prompt(76), ref["codes"])
        assert ge.request_speech_rate(rid) == 100 and ge.request_speech_rate(sid) == 100
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE and ge.poll(sid)["state"] == gpu.REQ_DONE)
        assert np.array_equal(ge.result(rid)["codes"], ref["codes"]) and ge.poll(sid)["n_pcm"] == 0
        ge.release(sid)
        assert ge.tsm_stats() == dict(chunks=0, frames_out=0, flushes=0)
        assert ge.pcm_out_stats() == dict(chunks_converted=0, samples_out=0)
        with pytest.raises(gpu.Q3Error, match="unknown request id"):
            ge.request_speech_rate(rid)
    finally:
        ge.close()


def test_three_rates_side_by_side(gpu, eng3, takes):
    refs = [takes(77 + i, 8) for i in range(3)]
    rates, encs = [100, 50, 200], [0, 1, 0]
    rids = []
    for i, (pct, enc) in enumerate(zip(rates, encs)):
        eng3.set_output_format(24000, enc)
        eng3.set_speech_rate(pct)
        rids.append(eng3.submit(takes.prompt(77 + i), max_steps=8, seed=77 + i, mask_eos=True, want_pcm=True))
    eng3.set_speech_rate(100)
    eng3.set_output_format(None)
    assert [eng3.request_speech_rate(r) for r in rids] == rates
    _until(eng3, lambda: all(eng3.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [eng3.result(r, want_pcm=True) for r in rids]
    for o, ref in zip(out, refs):
        assert np.array_equal(o["codes"], ref["codes"])
    assert [o["n_pcm"] for o in out] == [8 * SPF, gpu.tsm_samples(50, 8 * SPF, True), gpu.tsm_samples(200, 8 * SPF, True)]
    assert out[0]["pcm"].dtype == np.float32 and _rms(out[0]["pcm"], refs[0]["pcm"]) < PCM_RMS_TOL
    _check(gpu, out[1]["pcm"], refs[1]["pcm"], 50, 1, "side by side, 50")
    _check(gpu, out[2]["pcm"], refs[2]["pcm"], 200, 0, "side by side, 200")


# -------------------------------------------------------- 5: refusals --------------------------------------------------------
def test_refusals(gpu, tiny_model, eng3, takes):
    for pct in (49, 201):
        with pytest.raises(gpu.Q3Error, match="range"):
            eng3.set_speech_rate(pct)
    rid = eng3.submit(takes.prompt(80), max_steps=1, seed=80, mask_eos=True, want_pcm=True)   # a refused call changed nothing
    assert eng3.request_speech_rate(rid) == 100
    eng3.set_output_format(16000, gpu.PCM_S16)                             # a resampled format and a rate do not combine
    eng3.set_speech_rate(125)
    for submit in (lambda: eng3.submit(takes.prompt(80), max_steps=4, seed=80, mask_eos=True, want_pcm=True),
                   lambda: eng3.submit_decode(takes(71, 10)["codes"]),
                   lambda: eng3.submit_candidates(takes.prompt(80), [1, 2], max_steps=4, want_pcm=True)):
        with pytest.raises(gpu.Q3Error, match="24000"):
            submit()
    eng3.set_output_format(None)
    eng3.set_speech_rate(50)                                               # f32 at 50: twice the native bytes
    with pytest.raises(gpu.Q3Error, match="staging"):
        eng3.submit(takes.prompt(80), max_steps=13, seed=80, mask_eos=True, want_pcm=True)
    ok = eng3.submit(takes.prompt(80), max_steps=12, seed=80, mask_eos=True, want_pcm=True)
    eng3.set_output_format(24000, gpu.PCM_S16)                             # s16 at 50: as many bytes as native
    ok16 = eng3.submit(takes.prompt(80), max_steps=24, seed=80, mask_eos=True, want_pcm=True)
    eng3.set_speech_rate(100)
    eng3.set_output_format(None)
    _until(eng3, lambda: all(eng3.poll(r)["state"] == gpu.REQ_DONE for r in (rid, ok, ok16)))
    assert eng3.poll(ok)["n_pcm"] == gpu.tsm_samples(50, 12 * SPF, True) == 12 * SPF * 2
    assert eng3.poll(ok16)["n_pcm"] == gpu.tsm_samples(50, 24 * SPF, True) == 24 * SPF * 2
    for r in (rid, ok, ok16):
        eng3.release(r)
    _drain(eng3)
    bare = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    for pct in (125, 100):
        with pytest.raises(gpu.Q3Error, match="codec"):
            bare.set_speech_rate(pct)
    assert bare.tsm_stats() == dict(chunks=0, frames_out=0, flushes=0)
    bare.close()
