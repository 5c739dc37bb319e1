"""[EXT] scoring given frames on the GPU (q3tts_submit_score, q3tts_group_submit_score, q3tts_engine_score_width, q3tts_op_score_rows,
q3tts_op_score_inputs; include/q3tts_spec.h "scoring").  Op level: k_score_rows against the float64 log-softmax and k_score_inputs against
numpy, with canaries around the outputs.  Engine level: the rows equal tests/score_ref.py (the oracle's logits under forced codes, float64) for
on-policy and off-policy codes, both quantisations, graph and eager, every pass-width / KV-page / prefill-chunk boundary, in-line and
asynchronous; they agree with the rows the same engine recorded while generating those codes; scoring disturbs no running request and leaves
nothing behind in its slot; and the request lifecycle is that of include/q3tts.h.

Tolerances.  Against float64: |lp - lp64| <= 1e-5 * max(1, |lp64|) (q3tts_spec.h "token log-probabilities").  Scored against recorded:
2e-5 * max(1, |lp|) -- derived, not measured: both lie within 1e-5 * max(1, |lp|) of one float64 value, given bit-identical logits."""
import ctypes as C
import os

import numpy as np
import pytest

import logprob_ref as LR
import score_ref as SR

pytestmark = pytest.mark.gpu
UPSTREAM = dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
WAIT_MS = 60000.0
SAMPLE_END, CODEC_EOS = 2160, 2150


# ---------------------------------------------------------------- op level ----------------------------------------------------------------
def _rows(F, n, rng):
    """[F][n] logits rows that meet every content kind, and a chosen index per row (0 and n - 1 among them)"""
    x = rng.normal(0.0, 3.0, (F, n)).astype(np.float32)
    c = rng.integers(0, n, F).astype(np.int32)
    for f in range(F):
        kind = f % 6
        if kind == 1:
            c[f] = 0
        elif kind == 2:
            c[f] = n - 1
        elif kind == 3:
            idx = rng.choice(n, size=9, replace=False)
            x[f, idx[idx != c[f]]] = -np.inf
        elif kind == 4:
            x[f] += np.float32(80.0)
        elif kind == 5:
            x[f] -= np.float32(80.0)
    return x, c


@pytest.mark.parametrize("F", [1, 7, 16, 17])
@pytest.mark.parametrize("t_stride", [2176, 2161])
def test_op_score_rows_against_float64(gpu, F, t_stride):
    rng = np.random.default_rng(100 * F + t_stride)
    tl = np.full((F, t_stride), 1e30, np.float32)                       # canaries behind every talker row: they must not reach the result
    tl[:, :SAMPLE_END], c0 = _rows(F, SAMPLE_END, rng)
    c0[c0 == CODEC_EOS] = 3
    pl = np.zeros((15, F, 2048), np.float32)
    codes = np.zeros((F, 16), np.int32)
    codes[:, 0] = c0
    for q in range(15):
        pl[q], codes[:, q + 1] = _rows(F, 2048, np.random.default_rng(7 * F + q))
        pl[q], codes[:, q + 1] = np.roll(pl[q], q, axis=0), np.roll(codes[:, q + 1], q)   # every head meets every kind, at F = 1 head by head
    if F > 3:
        tl[3, CODEC_EOS] = -np.inf                                       # column 16 of an -inf EOS logit
    buf = np.full((F + 2, 17), -555.0, np.float32)                       # canary rows around the host output
    gpu._chk(gpu.lib().q3tts_op_score_rows(gpu._p(tl), t_stride, gpu._p(pl), gpu._p(codes), F, C.c_void_p(buf.ctypes.data + 17 * 4)))
    assert np.all(buf[0] == -555.0) and np.all(buf[-1] == -555.0)
    got = buf[1:-1]
    assert np.array_equal(got, gpu.op_score_rows(tl, pl, codes))
    want = np.zeros((F, 17), np.float64)
    for f in range(F):
        want[f, 0], want[f, 16] = LR.log_softmax64(tl[f, :SAMPLE_END], codes[f, 0]), LR.log_softmax64(tl[f, :SAMPLE_END], CODEC_EOS)
        for q in range(15):
            want[f, q + 1] = LR.log_softmax64(pl[q, f], codes[f, q + 1])
    assert not np.isnan(got).any() and np.all(got[~np.isneginf(got)] <= 0.0)
    ok, ratio = LR.close(got, want)
    print("F %d t_stride %d: worst error %.3f of the bound" % (F, t_stride, ratio))
    assert ok, (ratio, np.argwhere(~np.isclose(got, want, rtol=1e-5, atol=1e-5))[:4])
    if F > 3:
        assert got[3, 16] == -np.inf


@pytest.mark.parametrize("F", [1, 15, 16, 17])
def test_op_score_inputs_against_numpy(gpu, F):
    rng = np.random.default_rng(F)
    dP = 48
    tabs = [rng.normal(0, 1, (2048 if q % 2 == 0 else 2040, dP)).astype(np.float32) for q in range(15)]   # odd books end before 2047
    hp = rng.normal(0, 1, (F, dP)).astype(np.float32)
    codes = rng.integers(0, 2040, (F, 16)).astype(np.int32)
    codes[0, :] = 0
    codes[F - 1, :] = 2047                                               # past the end of the odd books: a zero row there
    if F > 2:
        codes[1, :] = -1                                                 # a negative code reads row 0
    buf = np.full((16 * F + 2, dP), -555.0, np.float32)
    ptrs = (C.c_void_p * 15)(*[t.ctypes.data for t in tabs])
    rows = np.array([t.shape[0] for t in tabs], np.int64)
    gpu._chk(gpu.lib().q3tts_op_score_inputs(gpu._p(hp), ptrs, gpu._p(rows), dP, gpu._p(codes), F, C.c_void_p(buf.ctypes.data + dP * 4)))
    assert np.all(buf[0] == -555.0) and np.all(buf[-1] == -555.0)
    got = buf[1:-1].reshape(16, F, dP)
    assert np.array_equal(buf[1:-1], gpu.op_score_inputs(hp, tabs, codes))
    assert np.array_equal(got[0], hp)                                    # position 0: the given projected row, bit for bit
    for p in range(1, 16):
        t = tabs[p - 1]
        for f in range(F):
            c = max(int(codes[f, p - 1]), 0)
            want = t[c] if c < t.shape[0] else np.zeros(dP, np.float32)
            assert np.array_equal(got[p, f], want), (p, f, c)


# -------------------------------------------------------------- engine level --------------------------------------------------------------
def _drain(ge, limit=4000):
    for _ in range(limit):
        if not ge.sched_step():
            return
    raise AssertionError("the scheduler did not go idle")


@pytest.fixture(scope="module")
def assets(gpu, tiny_model):
    a = gpu.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    yield a
    a.close()


@pytest.fixture(scope="module")
def world(oracle, tiny_model, assets, vivian):
    """prompts, codes and float64 references, each computed once on the oracle and shared: get(name, quant) -> (prompt, codes, trail, lp64)"""
    pad, engines, cache = assets.tts_pad(), {}, {}

    def prompt(seed, n_text):
        rng = np.random.default_rng(seed)
        return assets.build_core(rng.integers(0, 4000, n_text).astype(np.int32), lang_id=2055, spk_emb=vivian)

    def oe(quant):
        if quant not in engines:
            engines[quant] = oracle.Engine(os.path.join(tiny_model, "gguf_" + quant), None, 4)
        return engines[quant]

    def random_codes(seed, n):
        rng = np.random.default_rng(seed)
        c = rng.integers(0, 2048, (n, 16)).astype(np.int32)
        c[0, 0], c[n - 1, 15] = 0, 2047
        return c

    def get(name, quant="q8_0"):
        if (name, quant) in cache:
            return cache[(name, quant)]
        trail = ()
        if name == "greedy":
            p = prompt(11, 8)
            codes, _ = LR.generate(oe(quant), pad, p, 12, seed=42, mask_eos=True)
        elif name == "upstream":
            p = prompt(13, 9)
            codes, _ = LR.generate(oe(quant), pad, p, 12, seed=44, mask_eos=True, **UPSTREAM)
        elif name == "offpolicy":
            p, codes, trail = prompt(15, 7), random_codes(3, 10), (17, 400, 3999)
        elif name.startswith("n="):                                      # n=<frames>: random codes behind a short prompt
            p, codes = prompt(21, 6), random_codes(5, int(name[2:]))
        elif name.startswith("rows="):                                   # rows=<n_prompt>,<frames>: a prompt of exactly that many rows
            n_prompt, n = (int(x) for x in name[5:].split(","))
            short = prompt(23, 6)
            p = prompt(23, 6 + n_prompt - short.shape[0])
            assert p.shape[0] == n_prompt, (p.shape, n_prompt)
            codes = random_codes(9, n)
        else:
            raise KeyError(name)
        cache[(name, quant)] = (p, codes, trail, SR.score(oe(quant), pad, p, codes, trail))
        return cache[(name, quant)]
    yield get
    for e in engines.values():
        e.close()


def _score(ge, case, wait=True):
    p, codes, trail, _ = case
    rid = ge.submit_score(p, codes, trailing_ids=trail if len(trail) else None)
    if not wait:
        return rid
    assert ge.wait(rid, WAIT_MS)
    return ge.result(rid)


def _check(got, case, what):
    _, codes, _, lp64 = case
    assert got["state"] == 3 and got["n_frames"] == codes.shape[0] and got["n_pcm"] == 0, (what, got["state"], got["n_frames"])
    assert np.array_equal(got["codes"], codes), (what, "fetch returns the given codes")
    lp = got["logprobs"]
    assert lp.dtype == np.float32 and lp.shape == (codes.shape[0], 17), (what, lp.shape)
    assert np.all(lp <= 0.0), (what, "a real value is never positive", lp.max())
    ok, ratio = LR.close(lp, lp64)
    print("%s: worst error %.3f of the bound" % (what, ratio))
    assert ok, (what, ratio, np.argwhere(np.abs(lp - lp64) > LR.TOL * np.maximum(1, np.abs(lp64)))[:4])


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
def test_engine_against_the_reference(gpu, tiny_model, world, quant, use_graph):
    ge = gpu.Engine(tiny_model, quant, max_batch=1, max_steps=16, load_codec=False, use_graph=use_graph)
    for name in ("greedy", "upstream", "offpolicy"):
        _check(_score(ge, world(name, quant)), world(name, quant), "%s %s graph=%s" % (name, quant, use_graph))
    ge.close()


def test_score_against_the_rows_recorded_while_generating(gpu, tiny_model, world):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    ge.set_logprobs(True)
    worst = 0.0
    for name, seed, kw in (("greedy", 42, {}), ("upstream", 44, UPSTREAM)):
        p, codes, _, _ = world(name)
        rid = ge.submit(p, max_steps=12, seed=seed, mask_eos=True, **kw)
        assert ge.wait(rid, WAIT_MS)
        rec = ge.result(rid)
        assert np.array_equal(rec["codes"], codes), name
        got = _score(ge, world(name))
        ok, ratio = LR.close(got["logprobs"], rec["logprobs"], tol=2e-5)
        worst = max(worst, ratio)
        print("%s: scored against recorded, worst %.4f of the 2e-5 bound; bit-equal: %s" % (name, ratio, np.array_equal(got["logprobs"], rec["logprobs"])))
        assert ok, (name, ratio)
    ge.close()


def test_boundaries_of_the_pass_width_and_the_kv_page(gpu, tiny_model, world):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=80, load_codec=False)
    W = ge.score_width()
    assert W >= 16
    for n in (1, W - 1, W, W + 1, 2 * W + 1):
        _check(_score(ge, world("n=%d" % n)), world("n=%d" % n), "n = %d (W = %d)" % (n, W))
    case = world("rows=60,8")                                            # positions 59 .. 66: across the 64-position KV page
    assert case[0].shape[0] + 8 > 64 > case[0].shape[0]
    _check(_score(ge, case), case, "across a KV page")
    ge.close()


@pytest.mark.parametrize("max_batch", [1, 4])
def test_rows_across_the_prefill_chunk(gpu, tiny_model, world, max_batch):
    """the talker rows n_prompt - 1 .. n_prompt + n - 2 straddle the prefill width: in line (one slot) and in an asynchronous wave beside a
    running request (four slots)"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=max_batch, max_prompt=1024, max_steps=48, load_codec=False)
    chunk = ge.prefill_width()
    case = world("rows=%d,12" % (chunk - 5))                             # rows chunk-6 .. chunk+5
    if max_batch > 1:
        p, codes, _, _ = world("greedy")
        gen = ge.submit(p, max_steps=40, seed=42, mask_eos=True)
        assert ge.sched_step() and ge.poll(gen)["n_frames"] == 4
        rid = _score(ge, case, wait=False)
        assert ge.sched_step() and ge.poll(rid)["state"] == 1 and ge.poll(gen)["n_frames"] == 8   # the wave runs beside the frame graph
        _drain(ge)
        got = ge.result(rid)
        assert np.array_equal(ge.result(gen)["codes"][:12], codes)
    else:
        got = _score(ge, case)
    _check(got, case, "across the prefill chunk, max_batch %d" % max_batch)
    ge.close()


def test_scoring_disturbs_no_running_request(gpu, tiny_model, world):
    """two generators under the driver thread, a score request admitted beside them: their codes and PCM are those of their solo runs bit for
    bit, and the scored rows those of the same request scored alone.  Only the first generator asks for PCM: the codec decodes the chunks of
    several requests in one grouped pass whose GEMM split depends on the group size, so PCM is bit-reproducible at equal group size only (across
    group sizes the project pins it to 1e-4 RMS); with one PCM request every chunk is decoded alone, as in its solo run"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=32, load_codec=True)
    gens = [(world("greedy")[0], dict(seed=42, want_pcm=True)), (world("upstream")[0], dict(seed=44, want_pcm=False, **UPSTREAM))]
    solo = []
    for p, kw in gens:
        rid = ge.submit(p, max_steps=28, mask_eos=True, **kw)
        assert ge.wait(rid, WAIT_MS)
        solo.append(ge.result(rid, want_pcm=True))
    assert solo[0]["pcm"].size > 0 and solo[0]["codes"].shape == solo[1]["codes"].shape == (28, 16)
    alone = _score(ge, world("offpolicy"))
    _check(alone, world("offpolicy"), "alone")
    ge.sched_start()
    try:
        rids = [ge.submit(p, max_steps=28, mask_eos=True, **kw) for p, kw in gens]
        while ge.poll(rids[0])["n_frames"] < 4:                          # the generators are stepping: the score request joins a running batch
            assert ge.poll(rids[0])["state"] in (0, 1)
        sid = _score(ge, world("offpolicy"), wait=False)
        for r in rids + [sid]:
            assert ge.wait(r, WAIT_MS)
    finally:
        ge.sched_stop()
    for r, want in zip(rids, solo):
        got = ge.result(r, want_pcm=True)
        assert np.array_equal(got["codes"], want["codes"]) and np.array_equal(got["pcm"], want["pcm"])
    beside = ge.result(sid)
    assert np.array_equal(beside["logprobs"], alone["logprobs"])         # batch invariance: exactly
    ge.close()


def test_slot_reuse_after_a_score(gpu, tiny_model, world):
    p, codes, _, _ = world("upstream")
    fresh = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=False)
    fresh.set_logprobs(True)
    rid = fresh.submit(p, max_steps=12, seed=44, mask_eos=True, **UPSTREAM)
    assert fresh.wait(rid, WAIT_MS)
    want = fresh.result(rid)
    fresh.close()
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=False)
    ge.set_logprobs(True)
    sid = _score(ge, world("offpolicy"), wait=False)
    rid = ge.submit(p, max_steps=12, seed=44, mask_eos=True, **UPSTREAM)  # queued behind the score request, takes its slot
    _drain(ge)
    _check(ge.result(sid), world("offpolicy"), "before the generation")
    got = ge.result(rid)
    assert np.array_equal(got["codes"], want["codes"]) and np.array_equal(got["codes"], codes)
    assert np.array_equal(got["logprobs"], want["logprobs"])             # recording on, no stale row
    ge.close()


def test_lifecycle_and_refusals(gpu, tiny_model, world):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_prompt=64, max_steps=16, load_codec=False)
    case = world("greedy")
    p, codes, _, _ = case
    rid = _score(ge, case, wait=False)
    st = ge.poll(rid)
    assert st["state"] == 0 and st["n_frames"] == 0
    assert ge.fetch(rid, 0, 64)[0].shape == (0, 16) and ge.fetch_logprobs(rid, 0, 64).shape == (0, 17)
    with pytest.raises(gpu.Q3Error, match="open trail"):
        ge.trail_append(rid, [5])
    queued = _score(ge, case, wait=False)                                # one slot: this one stays in the queue
    assert ge.cancel(queued) is True
    assert ge.poll(queued)["state"] == gpu.REQ_CANCELLED and ge.fetch(queued, 0, 64)[0].shape == (0, 16)
    assert ge.fetch_logprobs(queued, 0, 64).shape == (0, 17)
    ge.release(queued)
    assert ge.wait(rid, WAIT_MS)
    assert ge.poll(rid)["state"] == 3 and ge.poll(rid)["n_frames"] == 12
    assert np.array_equal(ge.fetch(rid, 0, 64)[0], codes) and ge.fetch_logprobs(rid, 0, 64).shape == (12, 17)
    assert np.array_equal(ge.fetch_logprobs(rid, 5, 3), ge.fetch_logprobs(rid, 0, 64)[5:8])
    assert ge.cancel(rid) is False                                       # it has ended
    _check(ge.result(rid), case, "lifecycle")
    # every refusal: < 0, a reason, nothing queued
    bad0, bad_eos, bad_res = codes.copy(), codes.copy(), codes.copy()
    bad0[3, 0], bad_eos[2, 0], bad_res[1, 7] = SAMPLE_END, CODEC_EOS, 2048
    long_prompt = np.zeros((65, 2048), np.float32)
    for args, why in (((p, codes[:0]), "n must be"), ((p, np.zeros((17, 16), np.int32)), "max_steps"), ((long_prompt, codes), "prompt length"),
                      ((p[:0], codes), "prompt"), ((p, bad0), "code_0"), ((p, bad_eos), "EOS"), ((p, bad_res), "residual"),
                      ((p, codes, np.zeros(65, np.int32)), "n_trail")):
        with pytest.raises(gpu.Q3Error, match=why):
            ge.submit_score(*args)
    L, out = gpu.lib(), C.c_int64(-5)
    for args in ((None, p.shape[0], None, 0, gpu._p(codes), 12), (gpu._p(p), p.shape[0], None, 0, None, 12), (gpu._p(p), p.shape[0], None, 2, gpu._p(codes), 12),
                 (gpu._p(p), p.shape[0], None, -1, gpu._p(codes), 12)):
        assert L.q3tts_submit_score(ge.h, *args, C.byref(out)) < 0 and L.q3tts_last_error() and out.value == -5
    assert not ge.sched_step()                                           # nothing was queued
    ge.close()
    # (n_prompt + n beyond the KV capacity cannot be reached through an engine: its pages hold max_prompt + max_steps + 1 positions; the rule's
    # own test in tests/test_score_cpu.py covers it)


def test_ggml_mode_refuses(gpu, tiny_model, world):
    old = os.environ.get("Q3_SPEC")
    os.environ["Q3_SPEC"] = "ggml"
    try:
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=False)
    finally:
        if old is None:
            os.environ.pop("Q3_SPEC")
        else:
            os.environ["Q3_SPEC"] = old
    p, codes, _, _ = world("greedy")
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.submit_score(p, codes)
    assert not ge.sched_step()
    ge.close()


def test_group_of_one_engine(gpu, tiny_model, world):
    q3 = gpu
    L = q3.lib()
    prm = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(prm))
    prm.model_dir, prm.quant, prm.max_batch, prm.max_steps, prm.load_codec = tiny_model.encode(), b"q8_0", 2, 16, 0
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs = np.zeros(1, np.int32)
    g = C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(prm), q3._p(devs), 1, C.byref(g)))
    try:
        case = world("offpolicy")
        p, codes, trail, lp64 = case
        rid = q3.group_submit_score(g, -1, p, codes, trailing_ids=trail)
        with pytest.raises(q3.Q3Error, match="engine_index"):
            q3.group_submit_score(g, 3, p, codes)
        assert L.q3tts_group_wait(g, rid, WAIT_MS) == 0
        out, gf, gp = np.zeros(16 * 16, np.int32), C.c_int32(), C.c_int64()
        q3._chk(L.q3tts_group_fetch(g, rid, q3._p(out), 0, 16, None, 0, 0, C.byref(gf), C.byref(gp)))
        lp = q3.group_fetch_logprobs(g, rid)
        assert gf.value == codes.shape[0] and np.array_equal(out[: gf.value * 16].reshape(-1, 16), codes) and lp.shape == (gf.value, 17)
        assert LR.close(lp, lp64)[0]
        q3._chk(L.q3tts_group_release(g, rid))
    finally:
        L.q3tts_group_destroy(g)
