"""[EXT] volume through the engine (q3tts_engine_set_volume, q3tts_request_volume, q3tts_engine_volume_stats and the group forms;
include/q3tts_spec.h "volume").  The codes and log-probability rows of a request never depend on its volume and its sample counts are the
native ones; its f32 PCM lies within 10 u |y64| + 2^-149 of the float64 evaluation on the PCM the same request delivers with the volume off,
and is q3tts_op_volume of that PCM bit for bit.  With a format, a rate or a pitch it is, bit for bit, that stage's test entry point run on
q3tts_op_volume of the native take.  Tiny model, Q8_0, max_steps <= 24.  The scheduler is stepped by hand and every wait is bounded.  A
request's native take is a second run on the same engine with the volume off -- alone where the request ran alone, side by side where it ran
side by side -- so that both runs decode the same chunks at the same width."""
import ctypes as C
import os

import numpy as np
import pytest

import volume_ref as R

pytestmark = pytest.mark.gpu
WAIT_MS = 60000.0
SPF = 1920
NO_VOLUME = dict(chunks=0, samples=0)


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
    """take(p, n, **kw): the request of prompt p run natively (no volume, no format, rate or pitch) with PCM on the given engine for exactly n
    frames (mask_eos); together([...]) runs several side by side"""

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
        assert all(self.ge.request_volume(r) == 0 for r in rids)
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
def eng4(gpu, tiny_model):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=True)
    yield ge
    ge.close()


@pytest.fixture(scope="module")
def takes(gpu, eng4, vivian):
    return Takes(gpu, eng4, vivian)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def volumed(gpu, native, db10):
    """q3tts_op_volume of a native take, in one chunk (the stage does not depend on the chunking)"""
    native = np.asarray(native, np.float32)
    outs, _, _, _, _, _ = gpu.op_volume(native[None, :], [native.size], [[0]], 1, [db10], trace=False)
    return outs[0]


def _check(gpu, got, native, db10, what):
    """count, dtype, the bound against float64 and the kernel's own bits, of one f32 stream against its native take"""
    native = np.asarray(native, np.float32)
    assert got.dtype == np.float32 and got.size == native.size, what
    rms_native = float(np.sqrt(np.mean(native.astype(np.float64) ** 2)))
    assert rms_native >= 1e-3, "%s: the native take is silent (rms %.3e): the check would be vacuous" % (what, rms_native)
    v = R.scaled(native, db10)
    y64, g64, _ = R.volume64(v)
    err = np.abs(got.astype(np.float64) - y64) / R.y_bound(y64)
    same = np.array_equal(bits(got), bits(volumed(gpu, native, db10)))
    print("%s: %+d tenths of a dB, %d samples, native rms %.3e peak %.3f, %.1f %% limited, max err / bound %.3g, equal to the kernel's own run: %s"
          % (what, db10, got.size, rms_native, np.abs(native).max(), 100 * np.mean(g64 < 1), err.max(), same))
    assert np.all(err <= 1.0), "%s: %.3g of the bound" % (what, err.max())
    assert np.abs(got).max() <= 1.0 and same, what
    if np.abs(v).max() <= 1.0:                                             # nothing to limit: the delayed product, bit for bit
        assert np.array_equal(bits(got), bits(np.concatenate([np.zeros(R.DELAY, np.float32), v[:-R.DELAY]]))), what


def _run(ge, gpu, prompt, n, db10, fmt=None, rate=100, pitch=100, **kw):
    if fmt:
        ge.set_output_format(*fmt)
    ge.set_speech_rate(rate)
    ge.set_pitch(pitch)
    ge.set_volume(db10)
    rid = ge.submit(prompt, max_steps=n, mask_eos=True, want_pcm=True, **kw)
    ge.set_volume(0)
    ge.set_pitch(100)
    ge.set_speech_rate(100)
    ge.set_output_format(None)
    assert ge.request_volume(rid) == db10 and ge.request_pitch(rid) == pitch and ge.request_speech_rate(rid) == rate
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    return ge.result(rid, want_pcm=True)


# -------------------------------------------------------- 1: per request --------------------------------------------------------
def test_codes_log_probabilities_counts_and_pcm_at_three_volumes(gpu, eng4, takes):
    n, got = 9, {}
    eng4.set_logprobs(True)
    for db10 in (0, -60, 120):
        s0 = eng4.volume_stats()
        eng4.set_volume(db10)
        rid = eng4.submit(takes.prompt(60), max_steps=n, seed=60, mask_eos=True, want_pcm=True, temperature=0.8, top_k=50, top_p=1.0)
        eng4.set_volume(0)
        assert eng4.request_volume(rid) == db10 and eng4.records(rid)
        seen = [0]
        for _ in range(4000):
            st = eng4.poll(rid)
            assert st["n_pcm"] >= seen[-1] and st["n_pcm"] % SPF == 0       # whole native chunks: the stage changes no count
            seen.append(st["n_pcm"])
            if st["state"] == gpu.REQ_DONE:
                break
            eng4.sched_step()
        assert seen[-1] == n * SPF
        lp = eng4.fetch_logprobs(rid)
        r = eng4.result(rid, want_pcm=True)
        got[db10] = (r, lp)
        s1 = eng4.volume_stats()
        want = (-(-n // 4), n * SPF) if db10 else (0, 0)
        assert (s1["chunks"] - s0["chunks"], s1["samples"] - s0["samples"]) == want
    eng4.set_logprobs(False)
    ref, lp0 = got[0]
    assert lp0.shape == (n, 17)
    for db10 in (-60, 120):
        r, lp = got[db10]
        assert np.array_equal(r["codes"], ref["codes"]) and np.array_equal(bits(lp), bits(lp0))   # the volume never reaches the talker
        assert r["sample_rate"] == 24000 and r["n_pcm"] == ref["n_pcm"] == n * SPF
        _check(gpu, r["pcm"], ref["pcm"], db10, "generated")
    assert np.abs(R.scaled(ref["pcm"], -60)).max() <= 1.0                   # so -60 was judged by bits


# -------------------------------------------------------- 2: composition, by bits --------------------------------------------------------
@pytest.mark.parametrize("what", ["16 kHz s16", "24 kHz s16", "rate 125", "pitch 80", "rate 125 pitch 80"])
def test_volume_in_front_of_every_other_stage(gpu, eng4, takes, what):
    n, db10, S16 = 10, 120, gpu.PCM_S16
    ref = takes(61, n)
    v = volumed(gpu, ref["pcm"], db10)
    if what == "16 kHz s16":
        r = _run(eng4, gpu, takes.prompt(61), n, db10, fmt=(16000, S16), seed=61)
        want = gpu.op_pcm_convert(v[None, :], [v.size], [[0]], 1, [(16000, S16)])[0][0]
    elif what == "24 kHz s16":
        r = _run(eng4, gpu, takes.prompt(61), n, db10, fmt=(24000, S16), seed=61)
        want = gpu.op_pcm_convert(v[None, :], [v.size], [[0]], 1, [(24000, S16)])[0][0]
    elif what == "rate 125":
        r = _run(eng4, gpu, takes.prompt(61), n, db10, rate=125, seed=61)
        want = gpu.op_tsm(v[None, :], [v.size], [[0]], 1, [125], [0], flush=True)[0][0]
    elif what == "pitch 80":
        r = _run(eng4, gpu, takes.prompt(61), n, db10, pitch=80, seed=61)
        want = gpu.op_pitch(v[None, :], [v.size], [[0]], 1, [100], [80], [0], flush=True)[0][0]
    else:
        r = _run(eng4, gpu, takes.prompt(61), n, db10, fmt=(24000, S16), rate=125, pitch=80, seed=61)
        want = gpu.op_pitch(v[None, :], [v.size], [[0]], 1, [125], [80], [S16], flush=True)[0][0]
    assert np.array_equal(r["codes"], ref["codes"])
    assert r["pcm"].dtype == want.dtype and r["pcm"].size == want.size > 0 and want.any()
    assert np.array_equal(r["pcm"].view(np.uint8), want.view(np.uint8)), what
    if r["pcm"].dtype == np.int16:                                         # a boost in front of the quantiser: full scale is reached, not passed
        assert np.abs(r["pcm"].astype(np.int32)).max() <= 32767


# -------------------------------------------------------- 3: the other submit forms --------------------------------------------------------
def test_streaming_text_request(gpu, eng4, takes):
    ids = [11, 22, 33, 44, 55, 66]
    ref = takes(70, 9, trailing_ids=ids)
    r = _run(eng4, gpu, takes.prompt(70), 9, 120, seed=70, trailing_ids=ids)
    assert np.array_equal(r["codes"], ref["codes"])
    _check(gpu, r["pcm"], ref["pcm"], 120, "streaming text")


def test_decode_only_and_resumed_requests(gpu, eng4, takes):
    ref = takes(71, 10)
    eng4.set_volume(200)
    rid = eng4.submit_decode(ref["codes"])
    eng4.set_volume(0)
    assert eng4.request_volume(rid) == 200
    _until(eng4, lambda: eng4.poll(rid)["state"] == gpu.REQ_DONE)
    dec = eng4.result(rid, want_pcm=True)
    _check(gpu, dec["pcm"], ref["pcm"], 200, "decode-only")
    res = _run(eng4, gpu, takes.prompt(71), 10, 90, seed=71, prefix_codes=ref["codes"][:5])
    assert np.array_equal(res["codes"], ref["codes"])
    _check(gpu, res["pcm"], ref["pcm"], 90, "resumed")                     # as the uninterrupted request


def test_candidate_set(gpu, eng4, takes):
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    rids = eng4.submit_candidates(takes.prompt(72), [1, 2, 3], max_steps=5, want_pcm=True, **kw)   # the same set, natively
    _until(eng4, lambda: all(eng4.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    refs = [eng4.result(x, want_pcm=True) for x in rids]
    assert all(r["pcm"].size == 5 * SPF for r in refs)
    eng4.set_volume(120)
    rids = eng4.submit_candidates(takes.prompt(72), [1, 2, 3], max_steps=5, want_pcm=True, **kw)
    eng4.set_volume(0)
    _until(eng4, lambda: all(eng4.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    for seed, x, ref in zip((1, 2, 3), rids, refs):
        assert eng4.request_volume(x) == 120                               # read once per set
        o = eng4.result(x, want_pcm=True)
        assert np.array_equal(o["codes"], ref["codes"])
        _check(gpu, o["pcm"], ref["pcm"], 120, "candidate %d" % seed)
    _drain(eng4)


def test_group_of_one(gpu, tiny_model, takes):
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
    devs, g = np.zeros(1, np.int32), C.c_void_p()
    gpu._chk(L.q3tts_group_create(C.byref(p), gpu._p(devs), 1, C.byref(g)))
    try:
        for bad in (-401, 201):
            with pytest.raises(gpu.Q3Error, match="range"):
                gpu.group_set_volume(g, bad)

        def decode():
            rid = gpu.group_submit_decode(g, 0, codes)
            assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            return rid

        def fetch(rid, total):
            buf, gp = np.zeros(total, np.float32), C.c_int64()
            gpu._chk(L.q3tts_group_fetch(g, rid, None, 0, 0, gpu._p(buf), 0, total, None, C.byref(gp)))
            assert gp.value == total
            gpu._chk(L.q3tts_group_release(g, rid))
            return buf

        rid = decode()
        assert gpu.group_request_volume(g, rid) == 0
        native = fetch(rid, 10 * SPF)                                       # the engine's own native take
        gpu.group_set_volume(g, 120)
        rid = decode()
        st = gpu.ReqStatus()
        gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
        assert (st.state, st.n_frames, st.n_pcm) == (gpu.REQ_DONE, 10, 10 * SPF) and gpu.group_request_volume(g, rid) == 120
        _check(gpu, fetch(rid, 10 * SPF), native, 120, "group of one")
        gpu.group_set_volume(g, 0)
        rid = decode()
        assert gpu.group_request_volume(g, rid) == 0
        assert np.array_equal(bits(fetch(rid, 10 * SPF)), bits(native))
    finally:
        L.q3tts_group_destroy(g)


# -------------------------------------------------------- 4: cancel, preamble --------------------------------------------------------
def test_a_cancelled_request_keeps_what_was_delivered(gpu, eng4, takes):
    ref = takes(73, 23)
    eng4.set_volume(120)
    rid = eng4.submit(takes.prompt(73), max_steps=23, seed=73, mask_eos=True, want_pcm=True)
    eng4.set_volume(0)
    _until(eng4, lambda: eng4.poll(rid)["n_frames"] >= 9 and eng4.poll(rid)["n_pcm"] >= 4 * SPF)
    assert eng4.cancel(rid)
    _until(eng4, lambda: eng4.poll(rid)["state"] == gpu.REQ_CANCELLED)
    r = eng4.result(rid, want_pcm=True)
    assert r["n_pcm"] % SPF == 0 and 4 * SPF <= r["n_pcm"] < 23 * SPF and r["pcm"].size == r["n_pcm"]   # whole chunks' samples
    assert np.array_equal(r["codes"], ref["codes"][: r["codes"].shape[0]])
    _check(gpu, r["pcm"], ref["pcm"][: r["n_pcm"]], 120, "cancelled")
    _drain(eng4)


def test_a_primed_request_starts_the_stage_from_a_reset(gpu, tiny_model, vivian, takes):
    pre = np.ascontiguousarray(takes(74, 9)["codes"])
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        ge.set_volume(120)                                                # a preamble build is never volumed
        pid = ge.preamble_create(pre)
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, 9)
        assert ge.volume_stats() == NO_VOLUME
        ge.set_volume(0)
        prompt = _prompt(ge, vivian, 75)
        ge.set_preamble(pid)
        rid = ge.submit(prompt, max_steps=10, seed=75, mask_eos=True, want_pcm=True)
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        native = ge.result(rid, want_pcm=True)                            # the primed request, natively, at 24000 Hz
        ge.set_volume(120)
        rid = ge.submit(prompt, max_steps=10, seed=75, mask_eos=True, want_pcm=True)
        ge.set_volume(0)
        ge.set_preamble(None)
        assert ge.request_preamble(rid) == pid and ge.request_volume(rid) == 120
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        assert np.array_equal(r["codes"], native["codes"])
        _check(gpu, r["pcm"], native["pcm"], 120, "primed")                # the reference starts from zeros: so did the stage
    finally:
        ge.close()


# -------------------------------------------------------- 5: 0 is off; side by side --------------------------------------------------------
def test_volume_0_is_an_ordinary_request(gpu, tiny_model, vivian):
    plain = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)   # an engine that never hears of volume
    takes = Takes(gpu, plain, vivian)
    ref = takes(76, 6)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        ge.set_volume(0)
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=True)
        assert ge.request_volume(rid) == 0
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        r = ge.result(rid, want_pcm=True)
        assert np.array_equal(r["codes"], ref["codes"])
        assert np.array_equal(bits(r["pcm"]), bits(ref["pcm"]))            # the bits of an engine that never heard of volume
        ge.set_volume(120)                                                 # not volumed: no PCM wanted, scoring
        rid = ge.submit(takes.prompt(76), max_steps=6, seed=76, mask_eos=True, want_pcm=False)
        sid = ge.submit_score(takes.prompt(76), ref["codes"])
        assert ge.request_volume(rid) == 0 and ge.request_volume(sid) == 0
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE and ge.poll(sid)["state"] == gpu.REQ_DONE)
        assert np.array_equal(ge.result(rid)["codes"], ref["codes"]) and ge.poll(sid)["n_pcm"] == 0
        ge.release(sid)
        assert ge.volume_stats() == NO_VOLUME
        with pytest.raises(gpu.Q3Error, match="unknown request id"):
            ge.request_volume(rid)
        assert plain.volume_stats() == NO_VOLUME
    finally:
        ge.close()
        plain.close()


def test_three_volumes_side_by_side_with_a_native_request(gpu, eng4, takes):
    refs = takes.together([(77 + i, 8, {}) for i in range(4)])             # the same four side by side, without the feature
    vols, rids = [60, -60, 200, 0], []
    for i, db10 in enumerate(vols):
        eng4.set_volume(db10)
        rids.append(eng4.submit(takes.prompt(77 + i), max_steps=8, seed=77 + i, mask_eos=True, want_pcm=True))
    eng4.set_volume(0)
    assert [eng4.request_volume(r) for r in rids] == vols
    _until(eng4, lambda: all(eng4.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [eng4.result(r, want_pcm=True) for r in rids]
    for o, ref in zip(out, refs):
        assert np.array_equal(o["codes"], ref["codes"]) and o["n_pcm"] == 8 * SPF
    assert np.array_equal(bits(out[3]["pcm"]), bits(refs[3]["pcm"]))       # the native request beside them: the bytes of a run without volumes
    for o, ref, db10 in zip(out[:3], refs[:3], vols[:3]):
        _check(gpu, o["pcm"], ref["pcm"], db10, "side by side")


def test_all_four_kinds_of_stream_in_the_same_passes(gpu, eng4, takes):
    """native, converted, stretched and shifted side by side: every stage of the pass tail runs in every pass, each on its own stream"""
    n, S16, F32 = 8, gpu.PCM_S16, gpu.PCM_F32
    refs = takes.together([(90 + i, n, {}) for i in range(4)])             # the same four side by side, without any setting
    #          format          rate pitch volume
    specs = [(None,            100, 100, 0),
             ((16000, S16),    100, 100, 60),
             ((24000, F32),    125, 100, -60),
             ((24000, S16),    100, 80,  200)]
    stats = lambda: (eng4.pcm_out_stats(), eng4.tsm_stats(), eng4.pitch_stats(), eng4.volume_stats())
    c0, t0, p0, v0 = stats()
    rids = []
    for i, (fmt, rate, pitch, db10) in enumerate(specs):
        eng4.set_output_format(*(fmt or (None,)))
        eng4.set_speech_rate(rate)
        eng4.set_pitch(pitch)
        eng4.set_volume(db10)
        rids.append(eng4.submit(takes.prompt(90 + i), max_steps=n, seed=90 + i, mask_eos=True, want_pcm=True))
    eng4.set_volume(0)
    eng4.set_pitch(100)
    eng4.set_speech_rate(100)
    eng4.set_output_format(None)
    for r, (fmt, rate, pitch, db10) in zip(rids, specs):
        assert eng4.request_format(r) == (fmt or (24000, F32))
        assert (eng4.request_speech_rate(r), eng4.request_pitch(r), eng4.request_volume(r)) == (rate, pitch, db10)
    _until(eng4, lambda: all(eng4.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [eng4.result(r, want_pcm=True) for r in rids]
    c1, t1, p1, v1 = stats()
    for o, ref in zip(out, refs):
        assert np.array_equal(o["codes"], ref["codes"])
    v = [volumed(gpu, ref["pcm"], s[3]) for ref, s in zip(refs, specs)]
    want = [refs[0]["pcm"],                                                # the native request: the bytes of the run without any setting
            gpu.op_pcm_convert(v[1][None, :], [v[1].size], [[0]], 1, [(16000, S16)])[0][0],
            gpu.op_tsm(v[2][None, :], [v[2].size], [[0]], 1, [125], [F32], flush=True)[0][0],
            gpu.op_pitch(v[3][None, :], [v[3].size], [[0]], 1, [100], [80], [S16], flush=True)[0][0]]
    counts = [n * SPF, gpu.pcm_out_samples(16000, n * SPF), gpu.tsm_samples(125, n * SPF, True), gpu.pitch_samples(100, 80, n * SPF, True)]
    assert counts[1] == n * 1280 and counts[2] % gpu.TSM_HOP == 0 and min(counts) > 0
    for o, w, cnt, what in zip(out, want, counts, ("native", "converted", "stretched", "shifted")):
        assert o["n_pcm"] == cnt == w.size and o["pcm"].dtype == w.dtype and o["pcm"].size == cnt, what
        assert np.array_equal(o["pcm"].view(np.uint8), w.view(np.uint8)), what
    chunks = -(-n // 4)
    assert (c1["chunks_converted"] - c0["chunks_converted"], c1["samples_out"] - c0["samples_out"]) == (chunks, counts[1])
    assert (t1["chunks"] - t0["chunks"], t1["frames_out"] - t0["frames_out"], t1["flushes"] - t0["flushes"]) == (chunks, counts[2] // gpu.TSM_HOP, 1)
    assert (p1["chunks"] - p0["chunks"], p1["samples_out"] - p0["samples_out"], p1["flushes"] - p0["flushes"]) == (chunks, counts[3], 1)
    assert p1["table_bytes"] == 366999 * 4                                 # all 151 tables, uploaded once
    assert (v1["chunks"] - v0["chunks"], v1["samples"] - v0["samples"]) == (3 * chunks, 3 * n * SPF)
    _drain(eng4)


KNOWN_REFUSALS = ("a speech rate needs the 24000 Hz output format", "max_steps at this speech rate makes more PCM than a request's staging holds")


def test_a_request_takes_settings_that_stood_together(gpu, eng4, takes):
    """One lock over the whole record.  With the scheduler stopped, a thread flips (format, rate) between (16000 s16, 100) and (24000 f32, 125)
    through the two setters, in an order such that every state on the way -- (24000 f32, 100) -- is itself acceptable, while this thread
    submits.  Every accepted request carries a pair that stood at some instant; a refusal carries a known text.  (16000 s16, 125), the old
    format with the new rate or the reverse, never stood: a submit that read it would have been refused with the first of the texts, and a
    request that carries it is a torn record."""
    import threading
    S16, F32 = gpu.PCM_S16, gpu.PCM_F32
    stood = {((16000, S16), 100), ((24000, F32), 100), ((24000, F32), 125)}
    prompt, stop, failed = takes.prompt(95), threading.Event(), []

    def flip():
        try:
            for _ in range(3000):
                if stop.is_set():
                    break
                eng4.set_output_format(24000, F32)                         # (16000 s16, 100) -> (24000 f32, 100) -> (24000 f32, 125)
                eng4.set_speech_rate(125)
                eng4.set_speech_rate(100)                                  # and back: the rate first, then the format
                eng4.set_output_format(16000, S16)
        except Exception as ex:                                            # noqa: BLE001 -- reported by the main thread
            failed.append(ex)

    eng4.set_output_format(16000, S16)
    th = threading.Thread(target=flip)
    th.start()
    rids, seen = [], set()
    try:
        for i in range(64):
            try:
                rid = eng4.submit(prompt, max_steps=1, seed=95, mask_eos=True, want_pcm=True)
            except gpu.Q3Error as ex:
                assert any(t in str(ex) for t in KNOWN_REFUSALS), str(ex)
                continue
            rids.append(rid)
            pair = (eng4.request_format(rid), eng4.request_speech_rate(rid))
            assert pair in stood, pair
            seen.add(pair)
    finally:
        stop.set()
        th.join(WAIT_MS / 1e3)
        eng4.set_speech_rate(100)
        eng4.set_output_format(None)
    assert not th.is_alive() and not failed, failed
    print("%d of 64 accepted, pairs seen: %s" % (len(rids), sorted(seen)))
    _until(eng4, lambda: all(eng4.poll(r)["state"] == gpu.REQ_DONE for r in rids), limit=20000)
    for r in rids:
        eng4.release(r)
    _drain(eng4)


def test_under_the_ggml_arithmetic(gpu, tiny_model, vivian):
    old = os.environ.get("Q3_SPEC")
    os.environ["Q3_SPEC"] = "ggml"
    try:
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    finally:
        if old is None:
            os.environ.pop("Q3_SPEC")
        else:
            os.environ["Q3_SPEC"] = old
    try:
        takes = Takes(gpu, ge, vivian)
        ref = takes(81, 6)
        r = _run(ge, gpu, takes.prompt(81), 6, 120, seed=81)
        assert np.array_equal(r["codes"], ref["codes"])
        _check(gpu, r["pcm"], ref["pcm"], 120, "Q3_SPEC=ggml")
        assert ge.volume_stats() == dict(chunks=2, samples=6 * SPF)
    finally:
        ge.close()


# -------------------------------------------------------- 6: refusals --------------------------------------------------------
def test_refusals(gpu, tiny_model, eng4, takes):
    for db10 in (-401, 201, 1000):
        with pytest.raises(gpu.Q3Error, match="volume out of range"):
            eng4.set_volume(db10)
    rid = eng4.submit(takes.prompt(80), max_steps=1, seed=80, mask_eos=True, want_pcm=True)   # a refused call changed nothing
    assert eng4.request_volume(rid) == 0
    eng4.set_volume(120)                                                   # rate and pitch at a resampled format stay refused, with a volume too
    eng4.set_speech_rate(125)
    eng4.set_output_format(16000, gpu.PCM_S16)
    with pytest.raises(gpu.Q3Error, match="24000"):
        eng4.submit(takes.prompt(80), max_steps=4, seed=80, mask_eos=True, want_pcm=True)
    eng4.set_output_format(None)
    eng4.set_speech_rate(100)
    ok = eng4.submit(takes.prompt(80), max_steps=2, seed=80, mask_eos=True, want_pcm=True)
    eng4.set_volume(0)
    assert ok == rid + 1 and eng4.request_volume(ok) == 120                # request ids are handed out at the queue: the refused submit took none
    _until(eng4, lambda: all(eng4.poll(r)["state"] == gpu.REQ_DONE for r in (rid, ok)))
    for r in (rid, ok):
        eng4.release(r)
    _drain(eng4)
    bare = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    for db10 in (60, 0):
        with pytest.raises(gpu.Q3Error, match="codec"):
            bare.set_volume(db10)
    assert bare.volume_stats() == NO_VOLUME
    bare.close()
