"""[EXT] loudness through the engine (q3tts_engine_set_loudness, q3tts_fetch_loudness, q3tts_request_loudness, q3tts_request_metered,
q3tts_engine_loudness_stats and the group forms; include/q3tts_spec.h "loudness").  A metered request has the codes and the PCM of the
unmetered one, bit for bit, and its rows are the segmented float64 restatement (tests/loudness_ref.py, fed the library's tables) over its
own native PCM, bit for bit -- whatever it is delivered as, since the meter reads in front of every output stage.  Tiny model, Q8_0,
max_steps <= 24.  The scheduler is stepped by hand and every wait is bounded."""
import ctypes as C
import os

import numpy as np
import pytest

import loudness_ref as R

pytestmark = pytest.mark.gpu
WAIT_MS = 60000.0
SPF = R.FRAME
NOTHING = dict(chunks=0, blocks=0)


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


@pytest.fixture(scope="module")
def tab(gpu):
    coef, M = gpu.loudness_tables()
    coef.setflags(write=False); M.setflags(write=False)
    return coef, M


@pytest.fixture(scope="module")
def eng4(gpu, tiny_model):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=True)
    yield ge
    ge.close()


def bits32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def restated(tab, pcm):
    """the rows of a native stream from its reset"""
    pcm = np.asarray(pcm, np.float32)
    assert pcm.size % SPF == 0 and float(np.sqrt(np.mean(pcm.astype(np.float64) ** 2))) >= 1e-3, "the take is silent: the check would be vacuous"
    return R.segmented(pcm, tab[0], tab[1])[0]


def run(ge, gpu, prompt, n, metered, fmt=None, rate=100, pitch=100, vol=0, **kw):
    """one request for exactly n frames with the given settings: (result, rows or None)"""
    if fmt:
        ge.set_output_format(*fmt)
    ge.set_speech_rate(rate); ge.set_pitch(pitch); ge.set_volume(vol); ge.set_loudness(metered)
    rid = ge.submit(prompt, max_steps=n, mask_eos=True, want_pcm=True, **kw)
    ge.set_loudness(False); ge.set_volume(0); ge.set_pitch(100); ge.set_speech_rate(100); ge.set_output_format(None)
    assert ge.request_metered(rid) == bool(metered)
    _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
    rows = ge.fetch_loudness(rid) if metered else None
    return ge.result(rid, want_pcm=True), rows


# -------------------------------------------------------- 1: per request --------------------------------------------------------
@pytest.mark.parametrize("n", (4, 5, 6, 9))
def test_a_metered_request_is_the_unmetered_one_and_its_rows_are_the_restatement(gpu, eng4, vivian, tab, n):
    prompt = _prompt(eng4, vivian, 60)
    ref, none = run(eng4, gpu, prompt, n, False, seed=60)
    assert none is None and ref["pcm"].size == n * SPF
    s0 = eng4.loudness_stats()
    eng4.set_loudness(True)
    rid = eng4.submit(prompt, max_steps=n, seed=60, mask_eos=True, want_pcm=True)
    eng4.set_loudness(False)
    assert eng4.request_metered(rid)
    seen = [0]
    for _ in range(4000):
        st = eng4.poll(rid)
        got = eng4.fetch_loudness(rid).shape[0]
        assert got == st["n_pcm"] // R.BLOCK and got >= seen[-1]            # the rows grow with n_pcm
        seen.append(got)
        if st["state"] == gpu.REQ_DONE:
            break
        eng4.sched_step()
    rows = eng4.fetch_loudness(rid)
    summary = eng4.request_loudness(rid)
    r = eng4.result(rid, want_pcm=True)
    assert np.array_equal(r["codes"], ref["codes"]) and np.array_equal(bits32(r["pcm"]), bits32(ref["pcm"]))
    assert rows.shape == ((4 * n) // 5, 2) and same(rows, restated(tab, r["pcm"]))
    assert summary == gpu.loudness_gate(rows) and summary["n_blocks"] == rows.shape[0]
    print("n = %d: %s" % (n, summary))
    s1 = eng4.loudness_stats()
    assert (s1["chunks"] - s0["chunks"], s1["blocks"] - s0["blocks"]) == (-(-n // 4), (4 * n) // 5)
    if n == 9:
        assert np.isfinite(summary["integrated_lufs"]) and summary["n_gated"] >= 1 and np.isfinite(summary["peak_dbfs"])
        assert abs(summary["peak_dbfs"] - 20.0 * np.log10(float(np.abs(r["pcm"][: 7 * R.BLOCK]).max()))) <= 1e-12


@pytest.mark.parametrize("what", ["volume +6 dB", "s16 at 8000 Hz", "rate 150", "pitch 80"])
def test_rows_do_not_depend_on_what_the_request_is_delivered_as(gpu, eng4, vivian, tab, what):
    n, prompt = 9, _prompt(eng4, vivian, 61)
    plain, rows0 = run(eng4, gpu, prompt, n, True, seed=61)
    assert same(rows0, restated(tab, plain["pcm"])) and rows0.shape == (7, 2)
    kw = {"volume +6 dB": dict(vol=60), "s16 at 8000 Hz": dict(fmt=(8000, gpu.PCM_S16)), "rate 150": dict(rate=150), "pitch 80": dict(pitch=80)}[what]
    r, rows = run(eng4, gpu, prompt, n, True, seed=61, **kw)
    assert np.array_equal(r["codes"], plain["codes"]) and same(rows, rows0), what
    assert r["pcm"].size > 0 and (r["pcm"].size != plain["pcm"].size or not np.array_equal(r["pcm"].view(np.uint8), plain["pcm"].view(np.uint8)))


# -------------------------------------------------------- 2: side by side, the other submit forms --------------------------------------------------------
def test_metered_and_unmetered_requests_share_passes(gpu, eng4, vivian, tab):
    n, prompts = 8, [_prompt(eng4, vivian, 70 + i) for i in range(4)]

    def together(flags):
        rids = []
        for i, on in enumerate(flags):
            eng4.set_loudness(on)
            rids.append(eng4.submit(prompts[i], max_steps=n, seed=70 + i, mask_eos=True, want_pcm=True))
        eng4.set_loudness(False)
        _until(eng4, lambda: all(eng4.poll(r)["state"] == gpu.REQ_DONE for r in rids))
        return rids

    refs = [eng4.result(r, want_pcm=True) for r in together([False] * 4)]
    s0 = eng4.loudness_stats()
    flags = [True, False, True, False]
    rids = together(flags)
    assert [eng4.request_metered(r) for r in rids] == flags
    s1 = eng4.loudness_stats()
    assert (s1["chunks"] - s0["chunks"], s1["blocks"] - s0["blocks"]) == (2 * 2, 2 * 6)   # the metered streams' chunks alone
    for r, on, ref in zip(rids, flags, refs):
        if on:
            rows = eng4.fetch_loudness(r)
        else:
            with pytest.raises(gpu.Q3Error, match="not metered"):
                eng4.fetch_loudness(r)
            with pytest.raises(gpu.Q3Error, match="not metered"):
                eng4.request_loudness(r)
        o = eng4.result(r, want_pcm=True)
        assert np.array_equal(o["codes"], ref["codes"]) and np.array_equal(bits32(o["pcm"]), bits32(ref["pcm"]))
        if on:
            assert rows.shape == (6, 2) and same(rows, restated(tab, o["pcm"]))
    with pytest.raises(gpu.Q3Error, match="unknown request id"):
        eng4.fetch_loudness(rids[0])


def test_decode_only_request_and_candidate_set(gpu, eng4, vivian, tab):
    ref, _ = run(eng4, gpu, _prompt(eng4, vivian, 71), 10, False, seed=71)
    eng4.set_loudness(True)
    rid = eng4.submit_decode(ref["codes"])
    kw = dict(temperature=0.9, top_k=50, top_p=1.0)
    cands = eng4.submit_candidates(_prompt(eng4, vivian, 72), [1, 2, 3], max_steps=5, want_pcm=True, **kw)
    eng4.set_loudness(False)
    assert eng4.request_metered(rid) and all(eng4.request_metered(c) for c in cands)   # read once per request, once per set
    _until(eng4, lambda: all(eng4.poll(x)["state"] == gpu.REQ_DONE for x in [rid] + cands))
    rows = eng4.fetch_loudness(rid)
    dec = eng4.result(rid, want_pcm=True)
    assert rows.shape == (8, 2) and same(rows, restated(tab, dec["pcm"]))
    seen = []
    for c in cands:
        rows = eng4.fetch_loudness(c)
        o = eng4.result(c, want_pcm=True)
        assert rows.shape == (4, 2) and same(rows, restated(tab, o["pcm"]))
        seen.append(rows[:, 0].tobytes())
    assert len(set(seen)) == 3                                               # three different takes
    _drain(eng4)


def test_fetch_offsets_and_counts(gpu, eng4, vivian):
    eng4.set_loudness(True)
    rid = eng4.submit(_prompt(eng4, vivian, 73), max_steps=9, seed=73, mask_eos=True, want_pcm=True)
    eng4.set_loudness(False)
    _until(eng4, lambda: eng4.poll(rid)["state"] == gpu.REQ_DONE)
    rows = eng4.fetch_loudness(rid)
    assert rows.shape == (7, 2)
    assert same(eng4.fetch_loudness(rid, 2, 3), rows[2:5]) and same(eng4.fetch_loudness(rid, 5, 100), rows[5:])
    assert eng4.fetch_loudness(rid, 7, 4).shape == (0, 2) and eng4.fetch_loudness(rid, 100, 4).shape == (0, 2) and eng4.fetch_loudness(rid, 0, 0).shape == (0, 2)
    L, got, buf = gpu.lib(), C.c_int64(-1), np.full((3, 2), 7.0)
    assert L.q3tts_fetch_loudness(eng4.h, rid, buf.ctypes.data, -1, 2, C.byref(got)) < 0 and got.value == -1 and np.all(buf == 7.0)
    assert L.q3tts_fetch_loudness(eng4.h, rid, buf.ctypes.data, 6, 3, C.byref(got)) == 0 and got.value == 1
    assert same(buf[0], rows[6]) and np.all(buf[1:] == 7.0)                  # nothing behind the rows it reports
    assert L.q3tts_fetch_loudness(eng4.h, rid, None, 0, 2, C.byref(got)) < 0 and L.q3tts_fetch_loudness(eng4.h, rid, buf.ctypes.data, 0, 2, None) < 0
    eng4.release(rid)


# -------------------------------------------------------- 3: cancel, stream reuse, preamble --------------------------------------------------------
def test_a_cancelled_request_keeps_the_rows_of_the_chunks_it_keeps(gpu, eng4, vivian, tab):
    eng4.set_loudness(True)
    rid = eng4.submit(_prompt(eng4, vivian, 74), max_steps=23, seed=74, mask_eos=True, want_pcm=True)
    eng4.set_loudness(False)
    _until(eng4, lambda: eng4.poll(rid)["n_frames"] >= 9 and eng4.poll(rid)["n_pcm"] >= 4 * SPF)
    assert eng4.cancel(rid)
    _until(eng4, lambda: eng4.poll(rid)["state"] == gpu.REQ_CANCELLED)
    rows = eng4.fetch_loudness(rid)
    r = eng4.result(rid, want_pcm=True)
    assert r["n_pcm"] % SPF == 0 and 4 * SPF <= r["n_pcm"] < 23 * SPF
    assert rows.shape == (r["n_pcm"] // R.BLOCK, 2) and same(rows, restated(tab, r["pcm"]))
    _drain(eng4)


def test_a_reused_codec_stream_and_an_engine_that_never_meters(gpu, tiny_model, vivian, tab):
    one = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    fresh = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        pa, pb = _prompt(one, vivian, 75), _prompt(one, vivian, 76)
        _, rows_a = run(one, gpu, pa, 7, True, seed=75)                      # leaves the stream's meter in the middle of a block
        b1, rows_b1 = run(one, gpu, pb, 6, True, seed=76)
        assert fresh.loudness_stats() == NOTHING
        unmetered, _ = run(fresh, gpu, pb, 6, False, seed=76)
        assert fresh.loudness_stats() == NOTHING                             # never enabled: nothing ran, nothing was allocated
        b2, rows_b2 = run(fresh, gpu, pb, 6, True, seed=76)
        assert rows_a.shape == (5, 2) and rows_b1.shape == (4, 2)
        assert np.array_equal(bits32(b1["pcm"]), bits32(b2["pcm"])) and np.array_equal(bits32(b2["pcm"]), bits32(unmetered["pcm"]))
        assert same(rows_b1, rows_b2) and same(rows_b1, restated(tab, b1["pcm"]))   # the rows of a fresh engine
        assert fresh.loudness_stats() == dict(chunks=2, blocks=4)
        fresh.set_loudness(True)                                             # not metered: no PCM wanted, scoring
        rid = fresh.submit(pb, max_steps=6, seed=76, mask_eos=True, want_pcm=False)
        sid = fresh.submit_score(pb, b2["codes"])
        fresh.set_loudness(False)
        assert not fresh.request_metered(rid) and not fresh.request_metered(sid)
        _until(fresh, lambda: fresh.poll(rid)["state"] == gpu.REQ_DONE and fresh.poll(sid)["state"] == gpu.REQ_DONE)
        fresh.release(rid); fresh.release(sid)
        assert fresh.loudness_stats() == dict(chunks=2, blocks=4)
    finally:
        one.close()
        fresh.close()


def test_a_primed_request_starts_the_meter_from_a_reset(gpu, tiny_model, vivian, tab):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=24, load_codec=True)
    try:
        pre, _ = run(ge, gpu, _prompt(ge, vivian, 77), 9, False, seed=77)
        ge.set_loudness(True)                                               # a preamble build is never metered
        pid = ge.preamble_create(np.ascontiguousarray(pre["codes"]))
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, 9)
        assert ge.loudness_stats() == NOTHING
        ge.set_preamble(pid)
        rid = ge.submit(_prompt(ge, vivian, 78), max_steps=10, seed=78, mask_eos=True, want_pcm=True)
        ge.set_preamble(None); ge.set_loudness(False)
        assert ge.request_preamble(rid) == pid and ge.request_metered(rid)
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        rows = ge.fetch_loudness(rid)
        r = ge.result(rid, want_pcm=True)
        assert rows.shape == (8, 2) and same(rows, restated(tab, r["pcm"]))   # the restatement starts from zeros: so did the meter
    finally:
        ge.close()


# -------------------------------------------------------- 4: group, ggml, refusals --------------------------------------------------------
def test_group_of_one(gpu, tiny_model, eng4, vivian, tab):
    codes = run(eng4, gpu, _prompt(eng4, vivian, 71), 10, False, seed=71)[0]["codes"]
    L = gpu.lib()
    p = gpu.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 16, 1
    L.q3tts_group_create.argtypes = [C.POINTER(gpu.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs, g = np.zeros(1, np.int32), C.c_void_p()
    gpu._chk(L.q3tts_group_create(C.byref(p), gpu._p(devs), 1, C.byref(g)))
    try:
        def decode():
            rid = gpu.group_submit_decode(g, 0, codes)
            assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
            return rid

        rid = decode()
        assert not gpu.group_request_metered(g, rid)
        with pytest.raises(gpu.Q3Error, match="not metered"):
            gpu.group_fetch_loudness(g, rid)
        gpu._chk(L.q3tts_group_release(g, rid))
        gpu.group_set_loudness(g, True)
        rid = decode()
        gpu.group_set_loudness(g, False)
        assert gpu.group_request_metered(g, rid)
        rows = gpu.group_fetch_loudness(g, rid)
        buf, gp = np.zeros(10 * SPF, np.float32), C.c_int64()
        gpu._chk(L.q3tts_group_fetch(g, rid, None, 0, 0, gpu._p(buf), 0, buf.size, None, C.byref(gp)))
        assert gp.value == 10 * SPF and rows.shape == (8, 2) and same(rows, restated(tab, buf))
        assert gpu.group_request_loudness(g, rid) == gpu.loudness_gate(rows)
        gpu._chk(L.q3tts_group_release(g, rid))
    finally:
        L.q3tts_group_destroy(g)


def test_under_the_ggml_arithmetic(gpu, tiny_model, vivian, tab):
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
        prompt = _prompt(ge, vivian, 81)
        ref, _ = run(ge, gpu, prompt, 6, False, seed=81)
        r, rows = run(ge, gpu, prompt, 6, True, seed=81)
        assert np.array_equal(r["codes"], ref["codes"]) and np.array_equal(bits32(r["pcm"]), bits32(ref["pcm"]))
        assert rows.shape == (4, 2) and same(rows, restated(tab, r["pcm"])) and ge.loudness_stats() == dict(chunks=2, blocks=4)
    finally:
        ge.close()


def test_an_engine_without_a_codec_refuses(gpu, tiny_model):
    bare = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    try:
        for on in (True, False):
            with pytest.raises(gpu.Q3Error, match="codec"):
                bare.set_loudness(on)
        assert bare.loudness_stats() == NOTHING
    finally:
        bare.close()
