"""[EXT] candidate sets on the GPU (q3tts_submit_candidates, q3tts_group_submit_candidates, q3tts_op_kv_fork; include/q3tts_spec.h "candidate
sets").  The kernel: the copied logical pages of every destination equal the source's bit for bit in both planes and every other byte of both
caches is unchanged.  The engine: every candidate of a set -- prefilled once, its KV pages copied into the other members' -- equals, bit for
bit, the plain request with its seed run alone on a one-slot engine: across prompt lengths around the page size and beyond one prefill chunk,
sampler modes, graph and eager, two quantisations, in-line and asynchronous waves, beside other requests, through cancels at every point,
with PCM, with log-probability recording, through a group and at full size.  The scheduler is stepped by hand where order matters; every
wait is bounded."""
import ctypes as C

import numpy as np
import pytest

import synth_models

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
WAIT_MS = 60000.0
SEEDS = [901, 902, 903, 904]


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


def _rows(ge, vivian, seed, n):
    """a prompt of exactly n rows, cut or tiled from build_core rows"""
    rng = np.random.default_rng(seed)
    base = ge.assets.build_core(rng.integers(0, 4000, 9).astype(np.int32), lang_id=2055, spk_emb=vivian)
    return np.ascontiguousarray(base[np.arange(n) % base.shape[0]], np.float32)


class Solo:
    """plain submissions, one at a time, on a one-slot engine: the reference of every comparison here"""

    def __init__(self, gpu, model, quant="q8_0", use_graph=True, load_codec=False, logprobs=False, max_steps=40):
        self.ge = gpu.Engine(model, quant, max_batch=1, max_steps=max_steps, load_codec=load_codec, use_graph=use_graph)
        self.codec = load_codec
        if logprobs:
            self.ge.set_logprobs(True)

    def run(self, prompt, seed, steps=8, trail=None, want_pcm=False, prefix=None, **kw):
        rid = self.ge.submit(prompt, max_steps=steps, seed=seed, mask_eos=True, want_pcm=want_pcm and self.codec, trailing_ids=trail,
                             prefix_codes=prefix, **kw)
        assert self.ge.wait(rid, WAIT_MS)
        return self.ge.result(rid, want_pcm=want_pcm and self.codec)

    def close(self):
        self.ge.close()


def _delta(ge, before):
    now = ge.candidate_stats()
    return {k: now[k] - before[k] for k in now}


# ---------------------------------------------------------------- the kernel ----------------------------------------------------------------
@pytest.fixture(scope="module")
def fork_world():
    """n_layer = 2, n_kv = 2, 12 physical pages of distinct random bits, 5 sequences of 3 logical pages, a scrambled page table.  Sequences 0..3
    own the 12 pages between them, so a copy of fewer than 3 pages, or to fewer than 3 destinations, leaves pages nobody named; sequence 4's
    row is not a real one (page 11 three times) and serves the refusals"""
    rng = np.random.default_rng(2024)
    k = rng.integers(0, 65536, (12, 2, 2, 8192)).astype(np.uint16)
    v = rng.integers(0, 65536, (12, 2, 2, 8192)).astype(np.uint16)
    pt = np.array([[7, 2, 9], [0, 10, 4], [5, 1, 8], [3, 6, 11], [11, 11, 11]], np.int32)
    k.setflags(write=False), v.setflags(write=False), pt.setflags(write=False)
    return k, v, pt


def _check_fork(k0, v0, k1, v1, pt, src, dsts, n_positions):
    np_ = (n_positions + 63) // 64
    wk, wv = k0.copy(), v0.copy()
    for d in dsts:
        for lp in range(np_):
            wk[pt[d, lp]] = k0[pt[src, lp]]
            wv[pt[d, lp]] = v0[pt[src, lp]]
    # the copied pages equal the source's; every other byte -- the source, the destinations' later pages, the unowned pages -- is unchanged
    assert np.array_equal(k1, wk) and np.array_equal(v1, wv)


@pytest.mark.parametrize("n_dst", [1, 3])
@pytest.mark.parametrize("n_positions", [1, 63, 64, 65, 128, 129, 192])
def test_op_kv_fork(gpu, fork_world, n_positions, n_dst):
    k, v, pt = fork_world
    src, dsts = 2, [0, 3, 1][:n_dst]
    k1, v1 = gpu.op_kv_fork(k, v, pt, src, dsts, n_positions)
    _check_fork(k, v, k1, v1, pt, src, dsts, n_positions)
    assert not np.array_equal(k1, k)                                     # something was copied


def test_op_kv_fork_at_the_talker_page_size(gpu):
    """28 layers x 8 kv heads = 229 376 16-byte pieces a plane page: 224 tiles a page over a grid row of fewer workgroups"""
    rng = np.random.default_rng(7)
    k = rng.integers(0, 65536, (7, 28, 8, 8192), dtype=np.uint16)
    v = rng.integers(0, 65536, (7, 28, 8, 8192), dtype=np.uint16)
    pt = np.array([[4, 1], [6, 0], [2, 5]], np.int32)                     # page 3 unowned
    k1, v1 = gpu.op_kv_fork(k, v, pt, 1, [2, 0], 65)
    _check_fork(k, v, k1, v1, pt, 1, [2, 0], 65)


def test_op_kv_fork_refusals_leave_the_buffers_untouched(gpu, fork_world):
    k0, v0, pt = fork_world
    k, v = k0.copy(), v0.copy()
    L = gpu.lib()

    def fork(table=pt, n_seq=5, src=2, d=(0, 3), n_dst=None, n_pos=65, n_pages=12):
        ds = np.array(d, np.int32)
        tb = np.ascontiguousarray(table, np.int32)
        return L.q3tts_op_kv_fork(gpu._p(k), gpu._p(v), n_pages, 2, 2, gpu._p(tb), n_seq, 3, src, gpu._p(ds), len(d) if n_dst is None else n_dst, n_pos)
    dup = pt.copy()
    dup[3, 1] = pt[0, 0]                                                  # a destination's page is another destination's
    own = pt.copy()
    own[0, 0] = pt[2, 1]                                                  # a destination's page is the source's
    for why, bad in (("n_dst", dict(n_dst=0)), ("out of range", dict(src=5)), ("out of range", dict(src=-1)), ("out of range", dict(d=(0, 5))),
                     ("out of range", dict(d=(-1,))), ("equals the source", dict(d=(0, 2))), ("listed twice", dict(d=(0, 3, 0))),
                     ("n_positions", dict(n_pos=0)), ("n_positions", dict(n_pos=193)), ("page table entry", dict(n_pages=10, n_pos=192)),
                     ("page table entry", dict(d=(4,), n_pages=11)), ("coincide", dict(table=dup, n_pos=128)), ("coincide", dict(table=own, n_pos=128)),
                     ("coincide", dict(d=(4,), n_pos=128))):
        assert fork(**bad) < 0 and why.encode() in L.q3tts_last_error(), (why, bad, L.q3tts_last_error())
    assert np.array_equal(k, k0) and np.array_equal(v, v0)
    assert fork(table=dup, n_pos=64) == 0                                 # the clash lies beyond the copied range
    _check_fork(k0, v0, k, v, dup, 2, [0, 3], 64)


# ------------------------------------------------------------- equals solo -------------------------------------------------------------
@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_every_candidate_equals_its_solo_run(gpu, tiny_model, vivian, quant, use_graph):
    ge = gpu.Engine(tiny_model, quant, max_batch=4, max_steps=12, load_codec=False, use_graph=use_graph)
    solo = Solo(gpu, tiny_model, quant, use_graph)
    pw = ge.prefill_width()
    assert pw + 7 <= 1024
    trail = np.random.default_rng(3).integers(0, 4000, 5).astype(np.int32)
    modes = [("sampled", SAMPLED, None), ("upstream", dict(SAMPLED, **UPSTREAM), None), ("trail", SAMPLED, trail)]
    for n_prompt in (5, 63, 64, 65, 130, pw + 7):                         # the last one spans prefill chunks
        prompt = _rows(ge, vivian, n_prompt, n_prompt)
        for name, kw, tr in modes:
            before = ge.candidate_stats()
            ids = ge.submit_candidates(prompt, SEEDS, max_steps=8, trailing_ids=tr, **kw)
            assert len(ids) == 4 and len(set(ids)) == 4
            _drain(ge)
            assert _delta(ge, before) == dict(sets=1, prefill_rows_saved=3 * n_prompt, pages_copied=3 * ((n_prompt + 63) // 64)), (n_prompt, name)
            got = [ge.result(r) for r in ids]
            for i, g in enumerate(got):
                want = solo.run(prompt, SEEDS[i], 8, trail=tr, **kw)
                assert g["state"] == gpu.REQ_DONE and g["codes"].shape == (8, 16), (n_prompt, name, i)
                assert np.array_equal(g["codes"], want["codes"]), (n_prompt, name, i)
            assert len({g["codes"].tobytes() for g in got}) > 1, (n_prompt, name)   # the seeds do differ
    ge.close()
    solo.close()


def test_greedy_set_and_set_of_one(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=12, load_codec=False)
    solo = Solo(gpu, tiny_model)
    prompt = _rows(ge, vivian, 11, 70)
    want = solo.run(prompt, 5, 8)["codes"]
    ids = ge.submit_candidates(prompt, [5, 6, 7], max_steps=8)            # temperature 0: every candidate is the plain greedy run
    _drain(ge)
    for r in ids:
        assert np.array_equal(ge.result(r)["codes"], want)
    assert ge.candidate_stats() == dict(sets=1, prefill_rows_saved=140, pages_copied=4)
    # n = 1 is a plain submission: nothing is copied
    one = ge.submit_candidates(prompt, [SEEDS[2]], max_steps=8, **SAMPLED)
    assert len(one) == 1
    _drain(ge)
    assert np.array_equal(ge.result(one[0])["codes"], solo.run(prompt, SEEDS[2], 8, **SAMPLED)["codes"])
    assert ge.candidate_stats() == dict(sets=1, prefill_rows_saved=140, pages_copied=4)
    # refusals that need the engine: too many candidates, bad options, an empty seed list; nothing is queued
    for bad in (dict(seeds=[1, 2, 3, 4, 5]), dict(seeds=[]), dict(seeds=[1, 2], repetition_penalty=0.0), dict(seeds=[1, 2], max_steps=13)):
        sd = bad.pop("seeds")
        with pytest.raises(gpu.Q3Error):
            ge.submit_candidates(prompt, sd, **dict(dict(max_steps=8), **bad))
    assert not ge.sched_step()
    ge.close()
    solo.close()


# ------------------------------------------------------------- mixed waves -------------------------------------------------------------
def test_mixed_waves_in_line_and_asynchronous(gpu, tiny_model, vivian):
    solo = Solo(gpu, tiny_model)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=8, max_steps=24, load_codec=False)
    # in-line: a set of 3, two plain requests and a resumed one in one wave of an idle engine
    ps, p1, p2, p3 = _rows(ge, vivian, 20, 66), _rows(ge, vivian, 21, 9), _rows(ge, vivian, 22, 17), _rows(ge, vivian, 23, 12)
    whole = solo.run(p3, 33, 16, **SAMPLED)["codes"]
    a = ge.submit(p1, max_steps=12, seed=31, **SAMPLED)
    ids = ge.submit_candidates(ps, SEEDS[:3], max_steps=10, **dict(SAMPLED, **UPSTREAM))
    b = ge.submit(p2, max_steps=8, seed=32)
    c = ge.submit(p3, max_steps=16, seed=33, prefix_codes=whole[:5], **SAMPLED)
    _steps(ge, 1)
    assert [ge.poll(r)["state"] for r in [a] + ids + [b, c]] == [gpu.REQ_RUNNING] * 6
    assert [ge.poll(r)["n_frames"] for r in [a] + ids + [b]] == [4] * 5 and ge.candidate_stats()["pages_copied"] == 4
    _drain(ge)
    assert np.array_equal(ge.result(a)["codes"], solo.run(p1, 31, 12, **SAMPLED)["codes"])
    assert np.array_equal(ge.result(b)["codes"], solo.run(p2, 32, 8)["codes"])
    assert np.array_equal(ge.result(c)["codes"], whole)
    for i, r in enumerate(ids):
        assert np.array_equal(ge.result(r)["codes"], solo.run(ps, SEEDS[i], 10, **dict(SAMPLED, **UPSTREAM))["codes"]), i
    # asynchronous: three requests run; a set of 4 is prefilled on the second stream and joins them
    run = [(_rows(ge, vivian, 24 + i, 7 + 3 * i), 40 + i, 20 + 2 * i) for i in range(3)]
    rids = [ge.submit(p, max_steps=s, seed=seed, **SAMPLED) for p, seed, s in run]
    _steps(ge, 1)
    pa = _rows(ge, vivian, 30, 130)
    before = ge.candidate_stats()
    ids = ge.submit_candidates(pa, SEEDS, max_steps=12, **SAMPLED)
    _steps(ge, 1)
    assert [(ge.poll(r)["state"], ge.poll(r)["n_frames"]) for r in ids] == [(gpu.REQ_RUNNING, 0)] * 4   # inside the wave
    assert [ge.poll(r)["n_frames"] for r in rids] == [8] * 3
    _drain(ge)
    assert _delta(ge, before) == dict(sets=1, prefill_rows_saved=390, pages_copied=9)
    for (p, seed, s), r in zip(run, rids):                                # the running requests are undisturbed
        assert np.array_equal(ge.result(r)["codes"], solo.run(p, seed, s, **SAMPLED)["codes"])
    for i, r in enumerate(ids):
        assert np.array_equal(ge.result(r)["codes"], solo.run(pa, SEEDS[i], 12, **SAMPLED)["codes"]), i
    ge.close()
    solo.close()


def test_a_set_is_admitted_whole_and_in_order(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=False)
    pa, pb, ps, pp = _rows(ge, vivian, 50, 8), _rows(ge, vivian, 51, 10), _rows(ge, vivian, 52, 65), _rows(ge, vivian, 53, 6)
    a = ge.submit(pa, max_steps=12, seed=60, **SAMPLED)
    b = ge.submit(pb, max_steps=24, seed=61, **SAMPLED)
    _steps(ge, 1)
    ids = ge.submit_candidates(ps, SEEDS[:3], max_steps=8, **SAMPLED)
    plain = ge.submit(pp, max_steps=8, seed=62, **SAMPLED)
    saw_wait = saw_set_first = False
    for _ in range(200):
        two_run = ge.poll(a)["state"] == gpu.REQ_RUNNING                  # a and b hold two of the four slots: fewer than 3 are free
        busy = ge.sched_step()
        sq = [ge.poll(r)["state"] == gpu.REQ_QUEUED for r in ids]
        pq = ge.poll(plain)["state"] == gpu.REQ_QUEUED
        assert all(sq) or not any(sq)                                     # whole or not at all
        if two_run:
            assert all(sq) and pq                                         # neither the set nor what stands behind it
            saw_wait = True
        if all(sq):
            assert pq                                                     # nothing overtakes the set
        elif pq:
            saw_set_first = True                                          # the set took the three slots; the plain request waits for the next
        if not busy:
            break
    assert saw_wait and saw_set_first and not ge.sched_step()
    got = {r: ge.result(r)["codes"] for r in [a, b, plain] + ids}
    ge.close()
    solo = Solo(gpu, tiny_model)
    assert np.array_equal(got[a], solo.run(pa, 60, 12, **SAMPLED)["codes"]) and np.array_equal(got[b], solo.run(pb, 61, 24, **SAMPLED)["codes"])
    assert np.array_equal(got[plain], solo.run(pp, 62, 8, **SAMPLED)["codes"])
    for i, r in enumerate(ids):
        assert np.array_equal(got[r], solo.run(ps, SEEDS[i], 8, **SAMPLED)["codes"]), i
    solo.close()


# ---------------------------------------------------------------- cancel ----------------------------------------------------------------
def test_cancel_at_every_point(gpu, tiny_model, vivian):
    solo = Solo(gpu, tiny_model)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=False)
    prompt = _rows(ge, vivian, 70, 67)
    want = [solo.run(prompt, s, 12, **SAMPLED)["codes"] for s in SEEDS]
    # in the queue: the members leave the set -- the first one too, so the second is the one prefilled
    before = ge.candidate_stats()
    ids = ge.submit_candidates(prompt, SEEDS, max_steps=12, **SAMPLED)
    assert ge.cancel(ids[0]) is True and ge.cancel(ids[2]) is True
    assert [ge.poll(r)["state"] for r in ids] == [gpu.REQ_CANCELLED, gpu.REQ_QUEUED, gpu.REQ_CANCELLED, gpu.REQ_QUEUED]
    _drain(ge)
    assert _delta(ge, before) == dict(sets=1, prefill_rows_saved=67, pages_copied=2)
    for i in (1, 3):
        assert np.array_equal(ge.result(ids[i])["codes"], want[i]), i
    for i in (0, 2):
        assert ge.poll(ids[i])["n_frames"] == 0 and ge.cancel(ids[i]) is False
        ge.release(ids[i])
    # mid-run: after two groups
    ids = ge.submit_candidates(prompt, SEEDS[:3], max_steps=12, **SAMPLED)
    _steps(ge, 2)
    assert ge.cancel(ids[1]) is True
    _drain(ge)
    got = [ge.result(r) for r in ids]
    assert [g["state"] for g in got] == [gpu.REQ_DONE, gpu.REQ_CANCELLED, gpu.REQ_DONE]
    assert got[1]["codes"].shape == (8, 16) and np.array_equal(got[1]["codes"], want[1][:8])
    assert np.array_equal(got[0]["codes"], want[0]) and np.array_equal(got[2]["codes"], want[2])
    # the prefilled member, inside an asynchronous wave: the copy was enqueued behind its last chunk, the survivors have their pages
    other = _rows(ge, vivian, 71, 9)
    r0 = ge.submit(other, max_steps=24, seed=77, **SAMPLED)
    _steps(ge, 1)
    ids = ge.submit_candidates(prompt, SEEDS[:3], max_steps=12, **SAMPLED)
    _steps(ge, 1)
    assert [(ge.poll(r)["state"], ge.poll(r)["n_frames"]) for r in ids] == [(gpu.REQ_RUNNING, 0)] * 3
    assert ge.cancel(ids[0]) is True
    _drain(ge)
    st = ge.poll(ids[0])
    assert (st["state"], st["n_frames"]) == (gpu.REQ_CANCELLED, 0)
    ge.release(ids[0])
    assert np.array_equal(ge.result(ids[1])["codes"], want[1]) and np.array_equal(ge.result(ids[2])["codes"], want[2])
    assert np.array_equal(ge.result(r0)["codes"], solo.run(other, 77, 24, **SAMPLED)["codes"])
    # all of them, mid-run; then the four slots and their pages serve a full-width batch as a fresh engine would
    ids = ge.submit_candidates(prompt, SEEDS, max_steps=12, **SAMPLED)
    _steps(ge, 1)
    for r in ids:
        assert ge.cancel(r) is True
    _drain(ge)
    for i, r in enumerate(ids):
        g = ge.result(r)
        assert g["state"] == gpu.REQ_CANCELLED and np.array_equal(g["codes"], want[i][:4]), i
    nxt = [(_rows(ge, vivian, 80 + i, 60 + 3 * i), 90 + i) for i in range(4)]
    rids = [ge.submit(p, max_steps=10, seed=s, **SAMPLED) for p, s in nxt]
    _drain(ge)
    for (p, s), r in zip(nxt, rids):
        assert np.array_equal(ge.result(r)["codes"], solo.run(p, s, 10, **SAMPLED)["codes"])
    assert not ge.sched_step()
    ge.close()
    solo.close()


# --------------------------------------------------- PCM, log-probabilities, slot reuse ---------------------------------------------------
def test_pcm_of_every_candidate(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=16, load_codec=True)
    solo = Solo(gpu, tiny_model, load_codec=True)
    prompt = _rows(ge, vivian, 100, 65)
    ids = ge.submit_candidates(prompt, SEEDS[:3], max_steps=12, want_pcm=True, **SAMPLED)
    _drain(ge)
    for i, r in enumerate(ids):
        g, w = ge.result(r, want_pcm=True), solo.run(prompt, SEEDS[i], 12, want_pcm=True, **SAMPLED)
        assert np.array_equal(g["codes"], w["codes"]), i
        assert g["pcm"].size == w["pcm"].size > 0 and _rms(g["pcm"], w["pcm"]) < PCM_RMS_TOL, i
    ge.close()
    solo.close()


def test_logprob_rows_of_every_candidate(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=24, load_codec=False)
    solo = Solo(gpu, tiny_model, logprobs=True)
    ge.set_logprobs(True)
    kw = dict(SAMPLED, **UPSTREAM)
    prompt = _rows(ge, vivian, 110, 64)
    want = [solo.run(prompt, s, 8, **kw) for s in SEEDS[:3]]
    for beside in (False, True):                                          # an in-line wave, then an asynchronous one
        if beside:
            r0 = ge.submit(_rows(ge, vivian, 111, 8), max_steps=24, seed=1)
            _steps(ge, 1)
        ids = ge.submit_candidates(prompt, SEEDS[:3], max_steps=8, **kw)
        _drain(ge)
        for i, r in enumerate(ids):
            g = ge.result(r)
            assert np.array_equal(g["codes"], want[i]["codes"]), (beside, i)
            assert g["logprobs"].shape == (8, 17) and np.array_equal(g["logprobs"], want[i]["logprobs"]), (beside, i)   # frame 0 included
            assert np.all(g["logprobs"] <= 0.0)
        if beside:
            ge.release(r0)
    ge.close()
    solo.close()


def test_slots_of_a_retired_set_serve_plain_requests(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=16, load_codec=False)
    ids = ge.submit_candidates(_rows(ge, vivian, 120, 129), SEEDS, max_steps=8, **SAMPLED)
    _drain(ge)
    for r in ids:
        ge.release(r)
    nxt = [(_rows(ge, vivian, 121 + i, 5 + 40 * i), 130 + i, SAMPLED if i % 2 else {}) for i in range(4)]
    rids = [ge.submit(p, max_steps=12, seed=s, **kw) for p, s, kw in nxt]
    _drain(ge)
    got = [ge.result(r)["codes"] for r in rids]
    ge.close()
    solo = Solo(gpu, tiny_model)
    for (p, s, kw), g in zip(nxt, got):
        assert np.array_equal(g, solo.run(p, s, 12, **kw)["codes"])
    solo.close()


# ---------------------------------------------------------------- group ----------------------------------------------------------------
@pytest.mark.parametrize("n_eng", [1, 2])
def test_group_routes_a_set_to_one_engine(gpu, tiny_model, vivian, n_eng):
    q3 = gpu
    L = q3.lib()
    p = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 4, 16, 0
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_engine.restype = C.c_void_p
    L.q3tts_group_engine.argtypes = [C.c_void_p, C.c_int32]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs = np.zeros(n_eng, np.int32)                                      # two engines: the device listed twice
    g = C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(p), q3._p(devs), n_eng, C.byref(g)))
    solo = Solo(gpu, tiny_model)
    try:
        assets = q3.Assets(handle=L.q3tts_engine_assets(L.q3tts_group_engine(g, 0)))
        rng = np.random.default_rng(140)
        base = assets.build_core(rng.integers(0, 4000, 9).astype(np.int32), lang_id=2055, spk_emb=vivian)
        prompt = np.ascontiguousarray(base[np.arange(66) % base.shape[0]], np.float32)
        gf, gp = C.c_int32(), C.c_int64()
        engines = []
        for rnd, eng in enumerate([-1, -1, n_eng - 1]):                   # round robin twice, then a named engine
            ids = q3.group_submit_candidates(g, eng, prompt, SEEDS[:3], max_steps=8, **SAMPLED)
            assert len({i & 255 for i in ids}) == 1 and len(set(ids)) == 3   # one engine index on every id of the set
            engines.append(ids[0] & 255)
            for i, rid in enumerate(ids):
                assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
                out = np.zeros(16 * 16, np.int32)
                q3._chk(L.q3tts_group_fetch(g, rid, q3._p(out), 0, 16, None, 0, 0, C.byref(gf), C.byref(gp)))
                assert gf.value == 8 and np.array_equal(out[:128].reshape(8, 16), solo.run(prompt, SEEDS[i], 8, **SAMPLED)["codes"]), (rnd, i)
                q3._chk(L.q3tts_group_release(g, rid))
        assert engines == [0, 1 % n_eng, n_eng - 1]
        ids = np.full(3, -9, np.int64)
        assert q3.lib().q3tts_group_submit_candidates(g, n_eng, None, 0, None, None, 0, None, 3, q3._p(ids)) < 0 and np.all(ids == -9)
        with pytest.raises(q3.Q3Error, match="engine_index"):
            q3.group_submit_candidates(g, n_eng, prompt, SEEDS[:3], max_steps=8)
    finally:
        L.q3tts_group_destroy(g)
        solo.close()


# -------------------------------------------------------------- full size --------------------------------------------------------------
def test_fullsize_set_of_8_beside_8_plain_requests(gpu, vivian):
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=16, max_steps=8, max_prompt=128, load_codec=False)
    ps = _rows(ge, vivian, 200, 75)
    plain = [(_rows(ge, vivian, 201 + i, 6 + 2 * i), 300 + i) for i in range(8)]
    seeds = list(range(500, 508))
    rids = [ge.submit(p, max_steps=6, seed=s, **SAMPLED) for p, s in plain]
    ids = ge.submit_candidates(ps, seeds, max_steps=6, **SAMPLED)
    _drain(ge)
    assert ge.candidate_stats() == dict(sets=1, prefill_rows_saved=7 * 75, pages_copied=14)
    got = [ge.result(r)["codes"] for r in rids + ids]
    ge.close()
    ref = gpu.Engine(model, "q8_0", max_batch=2, max_steps=8, max_prompt=128, load_codec=False)
    todo = plain + [(ps, s) for s in seeds]
    for i in range(0, 16, 2):                                             # the same requests, two at a time
        pair = [ref.submit(p, max_steps=6, seed=s, **SAMPLED) for p, s in todo[i:i + 2]]
        for j, r in enumerate(pair):
            assert ref.wait(r, WAIT_MS)
            w = ref.result(r)["codes"]
            assert w.shape == (6, 16) and np.array_equal(got[i + j], w), i + j
    ref.close()
