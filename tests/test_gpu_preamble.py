"""[EXT] codec preambles through the engine (q3tts_preamble_*, q3tts_voice_set_preamble, q3tts_engine_set_preamble and the group forms;
include/q3tts_spec.h "codec preambles").  P1: the PCM of a primed request is the CPU oracle's decode of preamble ++ frames without the
preamble's samples, within the standing 1e-4 RMS, at the sample count of the unprimed request.  P2: codes never change.  P3: a converting
request delivers the float64 conversion (tests/pcm_out_ref.py) of preamble_pcm ++ primed native pcm without the preamble's output samples.
Tiny model, Q8_0, max_steps <= 24; the scheduler is stepped by hand unless the test is about the driver thread, and every wait is bounded."""
import ctypes as C

import numpy as np
import pytest

import pcm_out_ref as R

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
S16_RMS_TOL = 1.1e-4          # 1e-4 and 1 / (32767 sqrt(12)) of quantisation noise, summed (test_gpu_pcm_out_engine.py)
WAIT_MS = 60000.0
SPF = 1920
M = 9                         # frames of the engine-level preamble: past the tiny window of 8 and off the 4-frame chunk grid


def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def _until(ge, cond, limit=4000):
    for _ in range(limit):
        if cond():
            return
        ge.sched_step()
    raise AssertionError("condition not reached")


def _done(ge, gpu, rid):
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    return ge.result(rid, want_pcm=True)


def _prompt(ge, vivian, seed, n=8):
    rng = np.random.default_rng(seed)
    return ge.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=vivian)


def _ready(ge, gpu, codes):
    pid = ge.preamble_create(codes)
    assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, len(codes))
    return pid


class Oracle:
    """the CPU oracle's codec: cold(c) = decode(c) from a reset, primed(p, c) = decode(p ++ c) without the first len(p) * 1920 samples.
    p is cut into 4-frame chunks plus a tail, then c the same way (the oracle is chunk-invariant bit for bit; the cut is the definition's)"""

    def __init__(self, oracle, model):
        self.c = oracle.Codec(model + "/onnx/q3tts_codec.gguf")
        self.memo = {}

    def _feed(self, codes):
        codes = np.minimum(np.asarray(codes, np.int64).reshape(-1, 16), 2047)    # every code is clamped to [0, 2047]
        return [self.c.decode(codes[i: i + 4]) for i in range(0, len(codes), 4)]

    def primed(self, p, c):
        key = (np.asarray(p).tobytes(), np.asarray(c).tobytes())
        if key not in self.memo:
            self.c.reset()
            self._feed(p)
            out = np.concatenate(self._feed(c))
            out.setflags(write=False)
            self.memo[key] = out
        return self.memo[key]

    def cold(self, c):
        return self.primed(np.zeros((0, 16), np.int64), c)


@pytest.fixture(scope="module")
def orc(oracle, tiny_model):
    o = Oracle(oracle, tiny_model)
    yield o
    o.c.close()


@pytest.fixture(scope="module")
def pre():
    rng = np.random.default_rng(7)
    p = rng.integers(0, 2048, (M, 16)).astype(np.int32)
    p.setflags(write=False)
    return p


class Solo:
    """a one-slot engine with the engine-level preamble `pre` READY (self.pid, not set): run(p, n, primed, **kw) = the request of prompt p
    alone, natively, for exactly n frames"""

    def __init__(self, gpu, model, vivian, pre):
        self.gpu, self.vivian, self.memo = gpu, vivian, {}
        self.ge = gpu.Engine(model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
        self.pid = _ready(self.ge, gpu, pre)

    def prompt(self, p):
        return _prompt(self.ge, self.vivian, p)

    def run(self, p, n, primed=True, **kw):
        key = (p, n, primed, tuple(sorted(kw.items())))
        if key not in self.memo:
            self.ge.set_preamble(self.pid if primed else None)
            kw.setdefault("seed", p)
            rid = self.ge.submit(self.prompt(p), max_steps=n, mask_eos=True, want_pcm=True, **kw)
            self.ge.set_preamble(None)
            assert self.ge.request_preamble(rid) == (self.pid if primed else -1)
            assert self.ge.wait(rid, WAIT_MS)
            r = self.ge.result(rid, want_pcm=True)
            assert r["state"] == 3 and r["codes"].shape == (n, 16) and r["pcm"].size == n * SPF and r["pcm"].dtype == np.float32
            r["codes"].setflags(write=False), r["pcm"].setflags(write=False)
            self.memo[key] = r
        return self.memo[key]


@pytest.fixture(scope="module")
def solo(gpu, tiny_model, vivian, pre):
    s = Solo(gpu, tiny_model, vivian, pre)
    yield s
    s.ge.close()


@pytest.fixture(scope="module")
def eng3(gpu, tiny_model, pre):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=3, max_steps=24, load_codec=True)
    ge.pid = _ready(ge, gpu, pre)
    yield ge
    ge.close()


# -------------------------------------------------------- P1 / P2 against the CPU oracle --------------------------------------------------------
def test_p1_pcm_is_the_oracles_decode_behind_the_preamble(gpu, tiny_model, vivian, pre, orc):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        prompt = _prompt(ge, vivian, 41)
        assert ge.preamble_stats()["built"] == 0 and ge.preamble_stats()["restores"] == 0
        cold = _done(ge, gpu, ge.submit(prompt, max_steps=9, seed=41, mask_eos=True, want_pcm=True))
        pid = ge.preamble_create(pre)
        assert ge.preamble_poll(pid) == (gpu.PREAMBLE_BUILDING, M)
        with pytest.raises(gpu.Q3Error, match="building"):                # a setter refuses a BUILDING preamble
            ge.set_preamble(pid)
        vid = ge.register_voice(vivian)
        with pytest.raises(gpu.Q3Error, match="building"):
            ge.voice_set_preamble(vid, pid)
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, M)
        ge.set_preamble(pid)
        rid = ge.submit(prompt, max_steps=9, seed=41, mask_eos=True, want_pcm=True)
        assert ge.request_preamble(rid) == pid
        r = _done(ge, gpu, rid)
        assert np.array_equal(r["codes"], cold["codes"])                  # P2: nothing of the talker or the predictor knows
        want, want_cold = orc.primed(pre, r["codes"]), orc.cold(r["codes"])
        first = _rms(want[:SPF], want_cold[:SPF])
        print("oracle, primed against cold, first frame: rms %.3f" % first)
        assert first >= 0.05                                              # the comparison below can tell the two apart
        assert r["pcm"].size == cold["pcm"].size == want.size == 9 * SPF
        rms, rms_cold = _rms(r["pcm"], want), _rms(cold["pcm"], want_cold)
        print("primed rms %.3e, unprimed rms %.3e" % (rms, rms_cold))
        assert rms < PCM_RMS_TOL and rms_cold < PCM_RMS_TOL
        st = ge.preamble_stats()
        assert st["built"] == 1 and st["restores"] == 1 and st["bytes_per_snapshot"] > 0
        # want_pcm = 0 ignores the setting; so does a blocking batch
        rid = ge.submit(prompt, max_steps=9, seed=41, mask_eos=True, want_pcm=False)
        assert ge.request_preamble(rid) == -1
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        assert np.array_equal(ge.result(rid)["codes"], cold["codes"])
        b = ge.generate_batch([prompt], max_steps=9, seed=41, mask_eos=True, want_pcm=True)[0]
        assert np.array_equal(b["codes"], cold["codes"]) and _rms(b["pcm"], want_cold) < PCM_RMS_TOL
        assert ge.preamble_stats()["restores"] == 1
    finally:
        ge.close()


# -------------------------------------------------------- the voice path --------------------------------------------------------
def test_a_primed_clone_voice_beside_a_preset_voice(gpu, tiny_model, vivian, eng3, orc):
    rng = np.random.default_rng(19)
    ref_codes, ref_text = rng.integers(0, 2048, (5, 16)).astype(np.int32), rng.integers(0, 4000, 3).astype(np.int32)
    text = [rng.integers(0, 4000, 6).astype(np.int32) for _ in range(2)]

    def voices(ge):
        clone, preset = ge.register_voice(vivian, ref_codes, ref_text), ge.register_voice(vivian)
        with pytest.raises(gpu.Q3Error, match="reference codes"):
            ge.prime_voice(preset)
        return clone, preset, ge.prime_voice(clone, WAIT_MS)

    one = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        c1, p1, _ = voices(one)
        alone = []
        for v, t in ((c1, text[0]), (p1, text[1])):
            rid = one.submit_text(v, t, max_steps=9, seed=5, mask_eos=True, want_pcm=True)
            alone.append(_done(one, gpu, rid))
    finally:
        one.close()
    clone, preset, pid = voices(eng3)
    assert eng3.preamble_poll(pid) == (gpu.PREAMBLE_READY, 5)             # prime_voice released the creator's reference; the voice holds it
    eng3.set_preamble(eng3.pid)                                           # the engine-level setting does not apply to text forms
    rids = [eng3.submit_text(clone, text[0], max_steps=9, seed=5, mask_eos=True, want_pcm=True),
            eng3.submit_text(preset, text[1], max_steps=9, seed=5, mask_eos=True, want_pcm=True)]
    eng3.set_preamble(None)
    assert [eng3.request_preamble(r) for r in rids] == [pid, -1]
    _until(eng3, lambda: all(eng3.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [eng3.result(r, want_pcm=True) for r in rids]
    for o, a in zip(out, alone):
        assert np.array_equal(o["codes"], a["codes"]) and o["pcm"].size == a["pcm"].size == 9 * SPF
        assert _rms(o["pcm"], a["pcm"]) < PCM_RMS_TOL
    assert _rms(out[0]["pcm"], orc.primed(ref_codes, out[0]["codes"])) < PCM_RMS_TOL      # primed with the voice's own reference frames
    assert _rms(out[1]["pcm"], orc.cold(out[1]["codes"])) < PCM_RMS_TOL                   # the preset voice starts cold
    assert _rms(orc.primed(ref_codes, out[0]["codes"])[:SPF], orc.cold(out[0]["codes"])[:SPF]) >= 0.05
    eng3.voice_set_preamble(clone, None)                                  # the last holder goes: the preamble is recycled
    with pytest.raises(gpu.Q3Error, match="unknown preamble"):
        eng3.preamble_poll(pid)
    rid = eng3.submit_text(clone, text[0], max_steps=4, seed=5, mask_eos=True, want_pcm=True)
    assert eng3.request_preamble(rid) == -1
    _done(eng3, gpu, rid)


# -------------------------------------------------------- resume, candidates, decode-only, cancel --------------------------------------------------------
@pytest.mark.parametrize("k", (3, 5))
def test_resume_restores_first_then_the_prefix(gpu, eng3, solo, pre, orc, k):
    full = solo.run(50, 10)
    eng3.set_preamble(eng3.pid)
    rid = eng3.submit(solo.prompt(50), max_steps=10, seed=50, mask_eos=True, want_pcm=True, prefix_codes=full["codes"][:k])
    eng3.set_preamble(None)
    assert eng3.request_preamble(rid) == eng3.pid
    r = _done(eng3, gpu, rid)
    assert np.array_equal(r["codes"], full["codes"]) and r["pcm"].size == 10 * SPF
    assert _rms(r["pcm"], full["pcm"]) < PCM_RMS_TOL and _rms(r["pcm"], orc.primed(pre, r["codes"])) < PCM_RMS_TOL


def test_every_candidate_restores_the_same_snapshot(gpu, eng3, solo):
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    eng3.set_preamble(eng3.pid)
    rids = eng3.submit_candidates(solo.prompt(51), [1, 2, 3], max_steps=5, want_pcm=True, **kw)
    eng3.set_preamble(None)
    assert [eng3.request_preamble(x) for x in rids] == [eng3.pid] * 3
    _until(eng3, lambda: all(eng3.poll(x)["state"] == gpu.REQ_DONE for x in rids))
    for seed, x in zip((1, 2, 3), rids):
        o, a = eng3.result(x, want_pcm=True), solo.run(51, 5, seed=seed, **kw)
        assert np.array_equal(o["codes"], a["codes"]) and o["pcm"].size == 5 * SPF and _rms(o["pcm"], a["pcm"]) < PCM_RMS_TOL, seed


def test_decode_only(gpu, eng3, solo, pre, orc):
    codes = solo.run(50, 10)["codes"]
    eng3.set_preamble(eng3.pid)
    rid = eng3.submit_decode(codes)
    eng3.set_preamble(None)
    assert eng3.request_preamble(rid) == eng3.pid
    r = _done(eng3, gpu, rid)
    assert np.array_equal(r["codes"], codes) and r["pcm"].size == 10 * SPF
    assert _rms(r["pcm"], orc.primed(pre, codes)) < PCM_RMS_TOL
    rid = eng3.submit_decode(codes)                                       # and without the setting, cold as ever
    assert eng3.request_preamble(rid) == -1
    assert _rms(_done(eng3, gpu, rid)["pcm"], orc.cold(codes)) < PCM_RMS_TOL


def test_cancel_mid_utterance_keeps_the_primed_prefix(gpu, eng3, solo):
    full = solo.run(52, 24)
    eng3.set_preamble(eng3.pid)
    rid = eng3.submit(solo.prompt(52), max_steps=24, seed=52, mask_eos=True, want_pcm=True)
    eng3.set_preamble(None)
    _until(eng3, lambda: eng3.poll(rid)["n_frames"] >= 9 and eng3.poll(rid)["n_pcm"] >= 4 * SPF)
    assert eng3.cancel(rid)
    _until(eng3, lambda: eng3.poll(rid)["state"] == gpu.REQ_CANCELLED)
    assert eng3.request_preamble(rid) == eng3.pid
    r = eng3.result(rid, want_pcm=True)
    assert r["n_pcm"] > 0 and r["n_pcm"] % (4 * SPF) == 0 and r["n_pcm"] <= 24 * SPF and r["pcm"].size == r["n_pcm"]
    assert np.array_equal(r["codes"], full["codes"][: len(r["codes"])])
    assert _rms(r["pcm"], full["pcm"][: r["n_pcm"]]) < PCM_RMS_TOL
    assert _rms(r["pcm"][:SPF], solo.run(52, 24, primed=False)["pcm"][:SPF]) >= 0.05      # it is the primed run's prefix, not the cold one's


# -------------------------------------------------------- P3: formats --------------------------------------------------------
@pytest.mark.parametrize("rate,enc", ((16000, 1), (8000, 0)))
def test_p3_converted_stream_continues_the_preambles(gpu, eng3, solo, pre, rate, enc):
    native = solo.run(53, 9)
    pre_pcm = _done(eng3, gpu, eng3.submit_decode(pre))["pcm"]            # unprimed, native: the preamble's own PCM
    assert pre_pcm.size == M * SPF
    eng3.set_output_format(rate, enc)
    eng3.set_preamble(eng3.pid)
    rid = eng3.submit(solo.prompt(53), max_steps=9, seed=53, mask_eos=True, want_pcm=True)
    eng3.set_preamble(None)
    eng3.set_output_format(None)
    assert eng3.request_format(rid) == (rate, enc) and eng3.request_preamble(rid) == eng3.pid
    r = _done(eng3, gpu, rid)
    assert np.array_equal(r["codes"], native["codes"])
    L, Mq, _, _ = R.plan(rate)
    whole = R.convert(np.concatenate([pre_pcm, native["pcm"]]), rate, gpu.pcm_out_filter(rate))[0]
    want = whole[M * SPF * L // Mq:]
    got = r["pcm"]
    assert got.size == want.size == gpu.pcm_out_samples(rate, 9 * SPF) and got.dtype == (np.int16 if enc else np.float32)
    rms = _rms(got / 32767.0 if enc else got, want)
    zeros = R.convert(native["pcm"], rate, gpu.pcm_out_filter(rate))[0]   # what a converter history of zeros would have given
    print("%d Hz %s: rms %.3e (against a zero history: %.3e)" % (rate, "s16" if enc else "f32", rms, _rms(want, zeros)))
    assert rms < (S16_RMS_TOL if enc else PCM_RMS_TOL)


# -------------------------------------------------------- lifecycle --------------------------------------------------------
def test_release_while_a_queued_request_holds_the_preamble(gpu, tiny_model, vivian, pre, solo):
    want = solo.run(54, 6)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        pid = _ready(ge, gpu, pre)
        ge.set_preamble(pid)
        rid = ge.submit(solo.prompt(54), max_steps=6, seed=54, mask_eos=True, want_pcm=True)      # queued: nothing steps the scheduler
        gone = ge.submit(solo.prompt(54), max_steps=6, seed=54, mask_eos=True, want_pcm=True)
        ge.set_preamble(None)
        ge.preamble_release(pid)
        with pytest.raises(gpu.Q3Error, match="already been released"):
            ge.preamble_release(pid)
        assert ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, M)           # the queued requests hold it
        with pytest.raises(gpu.Q3Error):
            ge.set_preamble(-3)
        assert ge.cancel(gone) and ge.poll(gone)["state"] == gpu.REQ_CANCELLED                    # cancelled in the queue: its reference goes at once
        assert ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, M)
        r = _done(ge, gpu, rid)
        assert np.array_equal(r["codes"], want["codes"]) and _rms(r["pcm"], want["pcm"]) < PCM_RMS_TOL
        with pytest.raises(gpu.Q3Error, match="unknown preamble"):        # the last reference went with the request's fence
            ge.preamble_poll(pid)
        with pytest.raises(gpu.Q3Error, match="unknown preamble"):
            ge.set_preamble(pid)
        ge.release(gone)
    finally:
        ge.close()


def test_the_65th_preamble_is_refused_until_one_is_released(gpu, tiny_model, pre, orc):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        rng = np.random.default_rng(3)
        codes = rng.integers(0, 2048, (gpu.MAX_PREAMBLES, 1, 16)).astype(np.int32)
        pids = [ge.preamble_create(c) for c in codes]
        assert pids == list(range(gpu.MAX_PREAMBLES))
        with pytest.raises(gpu.Q3Error, match="Q3TTS_MAX_PREAMBLES"):
            ge.preamble_create(pre)
        for bad, why in ((np.zeros((0, 16), np.int32), "n must be >= 1"), (np.full((25, 16), 7, np.int32), "max_steps"),
                         (np.full((2, 16), 2150, np.int32), "EOS")):
            with pytest.raises(gpu.Q3Error, match=why):
                ge.preamble_create(bad)
        for p in pids:
            assert ge.preamble_wait(p, WAIT_MS) and ge.preamble_poll(p) == (gpu.PREAMBLE_READY, 1)
        assert ge.preamble_stats()["built"] == gpu.MAX_PREAMBLES
        ge.preamble_release(pids[10])
        new = ge.preamble_create(pre)
        assert new == gpu.MAX_PREAMBLES                                   # ids are never reused
        assert ge.preamble_wait(new, WAIT_MS)
        with pytest.raises(gpu.Q3Error, match="Q3TTS_MAX_PREAMBLES"):
            ge.preamble_create(pre)
        # the snapshots did not disturb each other: the first, the last and the one in the recycled slot
        gen = np.random.default_rng(4).integers(0, 2048, (5, 16)).astype(np.int32)
        for pid, p in ((pids[0], codes[0]), (pids[-1], codes[-1]), (new, pre)):
            ge.set_preamble(pid)
            rid = ge.submit_decode(gen)
            ge.set_preamble(None)
            assert _rms(_done(ge, gpu, rid)["pcm"], orc.primed(p, gen)) < PCM_RMS_TOL, pid
    finally:
        ge.close()


def test_under_the_driver_thread(gpu, tiny_model, pre, solo):
    want = solo.run(55, 9)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=True)
    try:
        ge.sched_start()
        pid = ge.preamble_create(pre)
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, M)
        ge.set_preamble(pid)
        rids = [ge.submit(solo.prompt(55), max_steps=9, seed=55, mask_eos=True, want_pcm=True) for _ in range(3)]
        ge.set_preamble(None)
        ge.preamble_release(pid)
        for rid in rids:
            assert ge.wait(rid, WAIT_MS) and ge.request_preamble(rid) == pid
            r = ge.result(rid, want_pcm=True)
            assert np.array_equal(r["codes"], want["codes"]) and _rms(r["pcm"], want["pcm"]) < PCM_RMS_TOL
        ge.sched_stop()
        with pytest.raises(gpu.Q3Error, match="unknown preamble"):
            ge.preamble_poll(pid)
    finally:
        ge.close()


@pytest.mark.parametrize("n_eng", (1, 2))
def test_groups_on_one_device(gpu, tiny_model, vivian, pre, orc, n_eng):
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
    L.q3tts_group_voice_register.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    devs, g = np.zeros(n_eng, np.int32), C.c_void_p()
    gpu._chk(L.q3tts_group_create(C.byref(p), gpu._p(devs), n_eng, C.byref(g)))
    try:
        rng = np.random.default_rng(23)
        gen = rng.integers(0, 2048, (6, 16)).astype(np.int32)
        ref_codes, ref_text = rng.integers(0, 2048, (5, 16)).astype(np.int32), rng.integers(0, 4000, 3).astype(np.int32)
        text, vid, rid = rng.integers(0, 4000, 6).astype(np.int32), C.c_int32(), C.c_int64()
        gpu._chk(L.q3tts_group_voice_register(g, gpu._p(vivian), gpu._p(ref_codes), ref_codes.size, gpu._p(ref_text), ref_text.size, C.byref(vid)))

        def fetch(rid, n):
            assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            st = gpu.ReqStatus()
            gpu._chk(L.q3tts_group_poll(g, rid, C.byref(st)))
            assert (st.state, st.n_frames, st.n_pcm) == (gpu.REQ_DONE, n, n * SPF)
            codes, pcm, gf, gp = np.zeros((n, 16), np.int32), np.zeros(n * SPF, np.float32), C.c_int32(), C.c_int64()
            gpu._chk(L.q3tts_group_fetch(g, rid, gpu._p(codes), 0, n, gpu._p(pcm), 0, pcm.size, C.byref(gf), C.byref(gp)))
            assert (gf.value, gp.value) == (n, n * SPF)
            gpu._chk(L.q3tts_group_release(g, rid))
            return codes, pcm

        pid = gpu.group_preamble_create(g, pre)
        vpid = gpu.group_preamble_create(g, ref_codes)
        assert (pid, vpid) == (0, 1)                                      # one id on every engine
        with pytest.raises(gpu.Q3Error, match="building"):                # no engine has stepped: all engines or none
            gpu.group_set_preamble(g, pid)
        assert gpu.group_preamble_wait(g, pid, WAIT_MS) and gpu.group_preamble_wait(g, vpid, WAIT_MS)
        gpu.group_set_preamble(g, pid)
        gpu.group_voice_set_preamble(g, vid.value, vpid)
        gpu.group_preamble_release(g, vpid)                               # the voice holds it on every engine
        for idx in range(n_eng):                                          # every engine took the preamble and the setting
            rid_d = gpu.group_submit_decode(g, idx, gen)
            assert gpu.group_request_preamble(g, rid_d) == pid
            assert _rms(fetch(rid_d, 6)[1], orc.primed(pre, gen)) < PCM_RMS_TOL, idx
        for _ in range(n_eng):                                            # round robin: a text request on every engine, primed with its voice's
            sc = gpu.SamplerConfig(0.0, 40, 0.9, 1, 5)
            gpu._chk(L.q3tts_group_submit_text_ex(g, vid.value, gpu._p(text), text.size, 2055, None, 0, C.byref(sc), 6, 1, 1, None, C.byref(rid)))
            assert gpu.group_request_preamble(g, rid.value) == vpid
            codes, pcm = fetch(rid.value, 6)
            assert _rms(pcm, orc.primed(ref_codes, codes)) < PCM_RMS_TOL
        gpu.group_set_preamble(g, None)
        gpu.group_preamble_release(g, pid)
        rid_d = gpu.group_submit_decode(g, 0, gen)
        assert gpu.group_request_preamble(g, rid_d) == -1
        assert _rms(fetch(rid_d, 6)[1], orc.cold(gen)) < PCM_RMS_TOL
        with pytest.raises(gpu.Q3Error, match="unknown preamble"):
            gpu.group_set_preamble(g, pid)
    finally:
        L.q3tts_group_destroy(g)
