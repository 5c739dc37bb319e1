"""[EXT] output formats through the engine (q3tts_engine_set_output_format, q3tts_request_format, q3tts_fetch_pcm16 and the group forms;
include/q3tts_spec.h "output formats").  The codes of a request never depend on its format; its PCM is the float64 conversion
(tests/pcm_out_ref.py, the library's own table) of the PCM the same request delivers natively, within the standing PCM tolerance of 1e-4 RMS
-- plus, for int16, the quantisation noise of 1 LSB / sqrt(12).  Tiny model, Q8_0, max_steps <= 24.  The scheduler is stepped by hand and
every wait is bounded.  Reference takes come from a one-slot native engine."""
import ctypes as C

import numpy as np
import pytest

import pcm_out_ref as R

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
S16_RMS_TOL = 1.1e-4          # 1e-4 and 1 / (32767 sqrt(12)) = 8.8e-6 of quantisation noise, summed
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
    """take(p, n): the request of prompt p run alone, natively, with PCM on a one-slot engine for exactly n frames (greedy, mask_eos)"""

    def __init__(self, gpu, model, vivian):
        self.ge = gpu.Engine(model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
        self.vivian, self.memo = vivian, {}

    def prompt(self, p):
        return _prompt(self.ge, self.vivian, p)

    def __call__(self, p, n):
        if (p, n) not in self.memo:
            rid = self.ge.submit(self.prompt(p), max_steps=n, seed=p, mask_eos=True, want_pcm=True)
            assert self.ge.wait(rid, WAIT_MS)
            assert self.ge.request_format(rid) == (24000, 0)
            r = self.ge.result(rid, want_pcm=True)
            assert r["state"] == 3 and r["codes"].shape == (n, 16) and r["pcm"].size == n * SPF and r["pcm"].dtype == np.float32
            r["codes"].setflags(write=False), r["pcm"].setflags(write=False)
            self.memo[(p, n)] = r
        return self.memo[(p, n)]


@pytest.fixture(scope="module")
def takes(gpu, tiny_model, vivian):
    t = Takes(gpu, tiny_model, vivian)
    yield t
    t.ge.close()


@pytest.fixture(scope="module")
def eng3(gpu, tiny_model):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=3, max_steps=24, load_codec=True)
    yield ge
    ge.close()


def _want(gpu, pcm, rate):
    """the float64 conversion of native PCM over the library's table"""
    return R.convert(pcm, rate, gpu.pcm_out_filter(rate) if rate != R.NATIVE else None)[0]


def _check(gpu, got, native_pcm, rate, enc, what):
    want = _want(gpu, native_pcm, rate)
    assert got.size == want.size == gpu.pcm_out_samples(rate, native_pcm.size), (what, got.size, want.size)
    assert got.dtype == (np.int16 if enc else np.float32)
    rms = _rms(got / 32767.0 if enc else got, want)
    print("%s: %d Hz %s rms %.3e" % (what, rate, "s16" if enc else "f32", rms))
    assert rms < (S16_RMS_TOL if enc else PCM_RMS_TOL), "%s: rms %.3e" % (what, rms)
    return rms


def _run(ge, gpu, takes, p, n, rate, enc, **kw):
    ge.set_output_format(rate, enc)
    rid = ge.submit(takes.prompt(p), max_steps=n, seed=p, mask_eos=True, want_pcm=True, **kw)
    ge.set_output_format(None)
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    assert ge.request_format(rid) == (rate, enc)
    return ge.result(rid, want_pcm=True)


# -------------------------------------------------------- 1: never set --------------------------------------------------------
def test_native_when_never_set(gpu, tiny_model, takes):
    ref = takes(11, 6)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=True)
    rid = ge.submit(takes.prompt(11), max_steps=6, seed=11, mask_eos=True, want_pcm=True)
    assert ge.request_format(rid) == (24000, gpu.PCM_F32)
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    with pytest.raises(gpu.Q3Error, match="f32"):
        ge.fetch_pcm16(rid, 0, 16)
    r = ge.result(rid, want_pcm=True)
    assert np.array_equal(r["codes"], ref["codes"]) and r["pcm"].dtype == np.float32 and r["sample_rate"] == 24000
    assert r["pcm"].size == ref["pcm"].size and _rms(r["pcm"], ref["pcm"]) < PCM_RMS_TOL
    assert ge.pcm_out_stats() == dict(chunks_converted=0, samples_out=0)
    with pytest.raises(gpu.Q3Error, match="unknown request id"):
        ge.request_format(rid)
    ge.close()


# -------------------------------------------------------- 2: {16000, s16} --------------------------------------------------------
def test_16k_s16_streams_chunk_by_chunk(gpu, eng3, takes):
    ref = takes(12, 10)
    s0 = eng3.pcm_out_stats()
    eng3.set_output_format(16000, gpu.PCM_S16)
    rid = eng3.submit(takes.prompt(12), max_steps=10, seed=12, mask_eos=True, want_pcm=True)
    eng3.set_output_format(None)
    seen = [0]
    for _ in range(4000):
        st = eng3.poll(rid)
        assert st["n_pcm"] >= seen[-1] and st["n_pcm"] % 1280 == 0     # whole frames of 1920 * 2 / 3 output samples
        if st["n_pcm"] != seen[-1]:
            seen.append(st["n_pcm"])
            part = eng3.fetch_pcm16(rid, 0, st["n_pcm"])                # what is there can be fetched while the request runs
            assert part.size == st["n_pcm"]
        if st["state"] == gpu.REQ_DONE:
            break
        eng3.sched_step()
    assert seen[-1] == 10 * 1280 and set(seen) <= {0, 4 * 1280, 8 * 1280, 10 * 1280}, seen
    whole = eng3.fetch_pcm16(rid, 0, 10 * 1280)
    assert np.array_equal(whole[: part.size], part)
    for off, cap in ((1, 7), (1279, 3), (5119, 1283), (12799, 50), (12800, 5), (0, 20000)):
        assert np.array_equal(eng3.fetch_pcm16(rid, off, cap), whole[off: off + cap]), (off, cap)
    codes, none = eng3.fetch(rid, 0, 10)                                # the codes half of q3tts_fetch works as ever
    assert np.array_equal(codes, ref["codes"]) and none.size == 0
    with pytest.raises(gpu.Q3Error, match="int16"):
        eng3.fetch(rid, 0, 10, 0, 16)                                   # but not its PCM half
    r = eng3.result(rid, want_pcm=True)
    assert r["sample_rate"] == 16000 and r["n_pcm"] == 10 * 1280 and np.array_equal(r["pcm"], whole)
    assert np.array_equal(r["codes"], ref["codes"])                     # the format never reaches the talker
    _check(gpu, whole, ref["pcm"], 16000, 1, "16 kHz s16")
    s1 = eng3.pcm_out_stats()
    assert s1["chunks_converted"] - s0["chunks_converted"] == 3 and s1["samples_out"] - s0["samples_out"] == 10 * 1280


# -------------------------------------------------------- 3: {8000, f32} --------------------------------------------------------
def test_8k_f32_through_fetch(gpu, eng3, takes):
    ref = takes(13, 9)
    r = _run(eng3, gpu, takes, 13, 9, 8000, gpu.PCM_F32)
    assert r["sample_rate"] == 8000 and np.array_equal(r["codes"], ref["codes"])
    _check(gpu, r["pcm"], ref["pcm"], 8000, 0, "8 kHz f32")
    eng3.set_output_format(8000, gpu.PCM_F32)
    rid = eng3.submit(takes.prompt(13), max_steps=4, seed=13, mask_eos=True, want_pcm=True)
    eng3.set_output_format(None)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_DONE)
    with pytest.raises(gpu.Q3Error, match="f32"):
        eng3.fetch_pcm16(rid, 0, 16)
    assert eng3.fetch(rid, 0, 4, 3, 100)[1].size == 100
    eng3.release(rid)


# -------------------------------------------------------- 4: two formats in one pass --------------------------------------------------------
def test_format_is_read_at_submit(gpu, eng3, takes):
    refs = [takes(14 + i, 8) for i in range(3)]
    fmts = [(16000, 1), (48000, 1), None]
    rids = []
    for i, f in enumerate(fmts):
        eng3.set_output_format(*(f if f else (None,)))
        rids.append(eng3.submit(takes.prompt(14 + i), max_steps=8, seed=14 + i, mask_eos=True, want_pcm=True))
    eng3.set_output_format(None)
    assert [eng3.request_format(r) for r in rids] == [(16000, 1), (48000, 1), (24000, 0)]
    _until(eng3, lambda: all(eng3.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [eng3.result(r, want_pcm=True) for r in rids]
    for o, ref in zip(out, refs):
        assert np.array_equal(o["codes"], ref["codes"])
    assert [o["n_pcm"] for o in out] == [8 * 1280, 8 * 3840, 8 * 1920] and [o["sample_rate"] for o in out] == [16000, 48000, 24000]
    _check(gpu, out[0]["pcm"], refs[0]["pcm"], 16000, 1, "A")
    _check(gpu, out[1]["pcm"], refs[1]["pcm"], 48000, 1, "B")
    assert out[2]["pcm"].dtype == np.float32 and _rms(out[2]["pcm"], refs[2]["pcm"]) < PCM_RMS_TOL


# -------------------------------------------------------- 5: decode-only and resume --------------------------------------------------------
def test_decode_only_and_resumed_requests_convert(gpu, eng3, takes):
    ref = takes(20, 10)
    gen = _run(eng3, gpu, takes, 20, 10, 22050, gpu.PCM_S16)
    _check(gpu, gen["pcm"], ref["pcm"], 22050, 1, "generated, 22.05 kHz")
    eng3.set_output_format(22050, gpu.PCM_S16)
    rid = eng3.submit_decode(ref["codes"])
    eng3.set_output_format(None)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_DONE)
    dec = eng3.result(rid, want_pcm=True)
    assert dec["sample_rate"] == 22050 and dec["pcm"].dtype == np.int16 and dec["pcm"].size == gen["pcm"].size == 10 * 1764
    assert _rms(dec["pcm"] / 32767.0, gen["pcm"] / 32767.0) < S16_RMS_TOL
    whole = _run(eng3, gpu, takes, 20, 10, 16000, gpu.PCM_S16)
    res = _run(eng3, gpu, takes, 20, 10, 16000, gpu.PCM_S16, prefix_codes=ref["codes"][:5])
    assert np.array_equal(res["codes"], ref["codes"]) and res["pcm"].dtype == np.int16
    assert res["pcm"].size == whole["pcm"].size and _rms(res["pcm"] / 32767.0, whole["pcm"] / 32767.0) < S16_RMS_TOL


# -------------------------------------------------------- 6: cancel and candidates --------------------------------------------------------
def test_cancel_keeps_whole_chunks_and_candidates_share_the_format(gpu, eng3, takes):
    full = _run(eng3, gpu, takes, 21, 24, 16000, gpu.PCM_S16)
    eng3.set_output_format(16000, gpu.PCM_S16)
    rid = eng3.submit(takes.prompt(21), max_steps=24, seed=21, mask_eos=True, want_pcm=True)
    eng3.set_output_format(None)
    _until(eng3, lambda: eng3.poll(rid)["n_frames"] >= 9 and eng3.poll(rid)["n_pcm"] >= 4 * 1280)
    assert eng3.cancel(rid)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_CANCELLED)
    r = eng3.result(rid, want_pcm=True)
    assert r["n_pcm"] > 0 and r["n_pcm"] % (4 * 1280) == 0 and r["n_pcm"] <= 24 * 1280 and r["pcm"].size == r["n_pcm"]
    assert _rms(r["pcm"] / 32767.0, full["pcm"][: r["n_pcm"]] / 32767.0) < S16_RMS_TOL
    eng3.set_output_format(16000, gpu.PCM_S16)
    rids = eng3.submit_candidates(takes.prompt(22), [1, 2, 3], max_steps=5, temperature=0.9, top_k=50, top_p=1.0, want_pcm=True)
    eng3.set_output_format(None)
    _until(eng3, lambda: all(eng3.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    for x in rids:
        assert eng3.request_format(x) == (16000, 1)
        o = eng3.result(x, want_pcm=True)
        assert o["pcm"].dtype == np.int16 and o["pcm"].size == 5 * 1280 and np.abs(o["pcm"]).max() > 0
    _drain(eng3)


# -------------------------------------------------------- 7: a group --------------------------------------------------------
def test_group_of_two_engines_on_one_device(gpu, tiny_model, takes, eng3):
    ref = takes(20, 10)
    eng3.set_output_format(16000, gpu.PCM_S16)
    rid = eng3.submit_decode(ref["codes"])
    eng3.set_output_format(None)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_DONE)
    single = eng3.result(rid, want_pcm=True)["pcm"]
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
        with pytest.raises(gpu.Q3Error):
            gpu.group_set_output_format(g, 32000, gpu.PCM_F32)
        gpu.group_set_output_format(g, 16000, gpu.PCM_S16)
        for idx in (0, 1):                                                  # both engines took the format
            rid = gpu.group_submit_decode(g, idx, ref["codes"])
            assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            st = gpu.ReqStatus()
            gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
            assert (st.state, st.n_frames, st.n_pcm) == (gpu.REQ_DONE, 10, 10 * 1280)
            assert gpu.group_request_format(g, rid) == (16000, 1)
            pcm = gpu.group_fetch_pcm16(g, rid, 0, st.n_pcm)
            assert pcm.size == single.size and _rms(pcm / 32767.0, single / 32767.0) < S16_RMS_TOL
            buf, gp = np.zeros(16, np.float32), C.c_int64()
            assert L.q3tts_group_fetch(g, rid, None, 0, 0, gpu._p(buf), 0, 16, None, C.byref(gp)) < 0   # the f32 PCM half is refused
            gpu._chk(L.q3tts_group_release(g, rid))
        gpu.group_set_output_format(g, None)
        rid = gpu.group_submit_decode(g, 0, ref["codes"][:4])
        assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0 and gpu.group_request_format(g, rid) == (24000, 0)
        with pytest.raises(gpu.Q3Error):
            gpu.group_fetch_pcm16(g, rid, 0, 16)
        gpu._chk(L.q3tts_group_release(g, rid))
    finally:
        L.q3tts_group_destroy(g)


# -------------------------------------------------------- 8: refusals --------------------------------------------------------
def test_set_output_format_refusals(gpu, tiny_model, eng3, takes):
    for rate, enc, why in ((11025, 1, "rate"), (16000, 2, "encoding"), (32000, 0, "24000")):
        with pytest.raises(gpu.Q3Error, match=why):
            eng3.set_output_format(rate, enc)
    rid = eng3.submit(takes.prompt(30), max_steps=1, seed=30, mask_eos=True, want_pcm=True)   # a refused call changed nothing
    assert eng3.request_format(rid) == (24000, 0)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_DONE)
    eng3.release(rid)
    bare = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    for args in ((16000, 1), (None,), (24000, 0)):
        with pytest.raises(gpu.Q3Error, match="codec"):
            bare.set_output_format(*args)
    assert bare.pcm_out_stats() == dict(chunks_converted=0, samples_out=0)
    bare.close()
