"""[EXT] token log-probabilities on the GPU (q3tts_engine_set_logprobs, q3tts_fetch_logprobs, the group forms, q3tts_op_logprob_rows;
include/q3tts_spec.h "token log-probabilities").  Op level: k_logprob_rows against the float64 log-softmax over row counts, widths, strides and
row contents that exercise the 16-byte path, its tail and its alignment fallback.  Engine level: recording changes neither codes nor PCM; the
values equal tests/logprob_ref.py (the oracle's logits, float64) on every path a frame's talker and predictor columns can take -- in-line and
asynchronous prefill, graph and eager, mixed batches, stalls, cancel and resume, slot reuse, a group.  The GPU's codes are compared with the
restatement's first, so a log-probability mismatch can only be the kernel or the row bookkeeping.

Tolerance: |lp - lp64| <= 1e-5 * max(1, |lp64|) (derived in q3tts_spec.h; tests/test_logprobs_cpu.py measures the q3_expf share)."""
import ctypes as C
import os

import numpy as np
import pytest

import logprob_ref as R

pytestmark = pytest.mark.gpu
PCM_RMS_TOL = 1e-4
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
WAIT_MS = 60000.0
NONE = np.float32(1.0)
# name -> (prompt seed, text ids, steps, request seed, mask_eos, sampler / options)
CASES = {
    "greedy": (11, 8, 12, 42, True, {}),
    "sampled": (12, 7, 12, 43, True, SAMPLED),
    "upstream": (13, 9, 12, 44, True, dict(SAMPLED, **UPSTREAM)),
    "nomask": (14, 6, 8, 45, False, SAMPLED),
}


# ---------------------------------------------------------------- op level ----------------------------------------------------------------
KINDS = ("normal", "some_inf", "chosen_inf", "plus80", "minus80", "all_equal", "spike")


def _row(kind, n, rng):
    """(row [n] f32, chosen index, check) for one content kind"""
    x = rng.normal(0.0, 3.0, n).astype(np.float32)
    c = int(rng.integers(0, n))
    if kind == "some_inf":
        idx = rng.choice(n, size=min(5, n - 1), replace=False)
        x[idx[idx != c]] = -np.inf
    elif kind == "chosen_inf":
        x[c] = -np.inf
    elif kind == "plus80":
        x += np.float32(80.0)
    elif kind == "minus80":
        x -= np.float32(80.0)
    elif kind == "all_equal":
        x[:] = np.float32(rng.normal(0.0, 3.0))
    elif kind == "spike":
        x[c] = np.max(np.delete(x, c)) + np.float32(60.0)
    return x, c


def _op_raw(gpu, lg, n, chosen, extra_idx):
    """the C entry point on output arrays with guard elements on either side"""
    B, stride = lg.shape
    oc, oe = np.full(B + 4, -555.0, np.float32), np.full(B + 4, -555.0, np.float32)
    gpu._chk(gpu.lib().q3tts_op_logprob_rows(gpu._p(lg), B, n, stride, gpu._p(chosen), extra_idx, C.c_void_p(oc.ctypes.data + 8),
                                             C.c_void_p(oe.ctypes.data + 8) if extra_idx >= 0 else None))
    assert np.all(oc[:2] == -555.0) and np.all(oc[B + 2:] == -555.0) and np.all(oe[:2] == -555.0) and np.all(oe[B + 2:] == -555.0)
    if extra_idx < 0:
        assert np.all(oe == -555.0)
    return oc[2:B + 2].copy(), oe[2:B + 2].copy()


@pytest.mark.parametrize("B", [1, 7, 64])
@pytest.mark.parametrize("n,stride", [(2048, 2048), (2160, 2176), (33, 48), (257, 257)])
def test_op_against_float64(gpu, B, n, stride):
    rng = np.random.default_rng(1000 * B + n)
    batches = [[k] for k in KINDS] if B == 1 else [[KINDS[b % len(KINDS)] for b in range(B)]]   # one row at a time still meets every kind
    worst = 0.0
    for kinds in batches:
        lg = np.full((len(kinds), stride), 1e30, np.float32)             # canaries behind every row: they must not reach the result
        chosen = np.zeros(len(kinds), np.int32)
        for b, k in enumerate(kinds):
            lg[b, :n], chosen[b] = _row(k, n, rng)
        extra = n - 1                                                    # the row's last element: inside the scalar tail when n % 4 != 0
        got_c, got_e = _op_raw(gpu, lg, n, chosen, extra)
        only_c, _ = _op_raw(gpu, lg, n, chosen, -1)
        assert np.array_equal(only_c, got_c, equal_nan=True)
        assert np.all(got_c[~np.isneginf(got_c)] <= 0.0) and np.all(got_e[~np.isneginf(got_e)] <= 0.0) and not np.isnan(got_c).any()
        for b, k in enumerate(kinds):
            want_c, want_e = R.log_softmax64(lg[b, :n], chosen[b]), R.log_softmax64(lg[b, :n], extra)
            for got, want in ((got_c[b], want_c), (got_e[b], want_e)):
                ok, ratio = R.close(np.array([got]), np.array([want]))
                worst = max(worst, ratio)
                assert ok, (k, b, got, want, ratio)
            if k == "chosen_inf":
                assert got_c[b] == -np.inf
            if k == "all_equal":
                assert abs(got_c[b] + np.log(n)) <= 1e-5 * np.log(n)
            if k == "spike":
                assert -1e-5 <= got_c[b] <= 0.0
    print("B %d n %d stride %d: worst error %.3f of the bound" % (B, n, stride, worst))


def test_op_wrapper_and_code_outside_the_row(gpu):
    rng = np.random.default_rng(5)
    lg = rng.normal(0, 3, (3, 40)).astype(np.float32)
    out, extra = gpu.op_logprob_rows(lg, [0, 39, 17], extra_idx=5)
    for b, c in enumerate((0, 39, 17)):
        assert R.close([out[b], extra[b]], [R.log_softmax64(lg[b], c), R.log_softmax64(lg[b], 5)])[0]
    out = gpu.op_logprob_rows(lg, [40, -1, 3], n=33)                     # a code that is not in the row has no probability
    assert out[0] == NONE and out[1] == NONE and R.close([out[2]], [R.log_softmax64(lg[2, :33], 3)])[0]


# -------------------------------------------------------------- engine level --------------------------------------------------------------
def _rms(a, b):
    return 0.0 if a.size == 0 else float(np.sqrt(np.mean((a - b) ** 2)))


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
def prompts(assets, vivian):
    out = {}
    for name, (pseed, n_text, _, _, _, _) in CASES.items():
        rng = np.random.default_rng(pseed)
        out[name] = assets.build_core(rng.integers(0, 4000, n_text).astype(np.int32), lang_id=2055, spk_emb=vivian)
    return out


@pytest.fixture(scope="module")
def refs(oracle, tiny_model, assets, prompts):
    """(codes, float64 logprobs) of every case on the oracle, computed once per quantisation and shared"""
    pad, cache, engines = assets.tts_pad(), {}, {}

    def get(name, quant="q8_0"):
        if (name, quant) not in cache:
            if quant not in engines:
                engines[quant] = oracle.Engine(os.path.join(tiny_model, "gguf_" + quant), None, 4)
            _, _, steps, seed, mask, kw = CASES[name]
            cache[(name, quant)] = R.generate(engines[quant], pad, prompts[name], steps, seed=seed, mask_eos=mask, **kw)
        return cache[(name, quant)]
    yield get
    for e in engines.values():
        e.close()


def _submit(ge, prompts, name, pcm=False, **over):
    _, _, steps, seed, mask, kw = CASES[name]
    return ge.submit(prompts[name], max_steps=steps, seed=seed, mask_eos=mask, want_pcm=pcm, **dict(kw, **over))


def _run(ge, prompts, name, pcm=False, **over):
    rid = _submit(ge, prompts, name, pcm, **over)
    assert ge.wait(rid, WAIT_MS)
    return ge.result(rid, want_pcm=pcm)


def _check(got, ref, what):
    codes, lp64 = ref
    assert np.array_equal(got["codes"], codes), (what, "codes differ from the restatement: not a log-probability question")
    lp = got["logprobs"]
    assert lp.dtype == np.float32 and lp.shape == (codes.shape[0], 17), (what, lp.shape)
    assert np.all(lp <= 0.0), (what, "a real value is never positive", lp.max())
    ok, ratio = R.close(lp, lp64)
    print("%s: worst error %.3f of the bound" % (what, ratio))
    assert ok, (what, ratio, np.argwhere(np.abs(lp - lp64) > R.TOL * np.maximum(1, np.abs(lp64)))[:4])


@pytest.mark.parametrize("use_graph", [True, False])
def test_recording_changes_neither_codes_nor_pcm(gpu, tiny_model, prompts, use_graph):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=True, use_graph=use_graph)
    offs = {}
    for name in ("greedy", "sampled"):
        off = offs[name] = _run(ge, prompts, name, pcm=True)
        assert "logprobs" not in off
        rid = _submit(ge, prompts, name)
        assert ge.wait(rid, WAIT_MS) and not ge.records(rid)
        with pytest.raises(gpu.Q3Error, match="does not record"):
            ge.fetch_logprobs(rid)
        ge.release(rid)
        ge.set_logprobs(True)
        on = _run(ge, prompts, name, pcm=True)
        ge.set_logprobs(False)
        again = _run(ge, prompts, name, pcm=True)
        assert "logprobs" not in again and on["logprobs"].shape == (off["codes"].shape[0], 17)
        for g in (on, again):
            assert np.array_equal(g["codes"], off["codes"]), name
            assert g["pcm"].size == off["pcm"].size and _rms(g["pcm"], off["pcm"]) < PCM_RMS_TOL, name
    # a blocking batch never records, whatever the flag says
    ge.set_logprobs(True)
    _, _, steps, seed, mask, kw = CASES["greedy"]
    r = ge.generate_batch([prompts["greedy"]], max_steps=steps, seed=seed, mask_eos=mask, **kw)[0]
    assert np.array_equal(r["codes"], offs["greedy"]["codes"]) and "logprobs" not in r
    ge.close()


@pytest.mark.parametrize("use_graph", [True, False])
def test_values_match_the_float64_reference(gpu, tiny_model, prompts, refs, use_graph):
    """one slot: every request is prefilled in line.  `upstream` carries the penalty and the sampled predictor: the values are the raw
    logits', not the penalised or tempered ones'.  The masked cases report a finite column 16 that equals the reference although EOS cannot
    be drawn"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=False, use_graph=use_graph)
    ge.set_logprobs(True)
    for name in CASES:
        got = _run(ge, prompts, name)
        _check(got, refs(name), name)
        if CASES[name][4] and got["logprobs"].size:
            assert np.all(np.isfinite(got["logprobs"][:, 16])), name
    ge.close()


def test_values_q5_k_m(gpu, tiny_model, prompts, refs):
    ge = gpu.Engine(tiny_model, "q5_k_m", max_batch=1, max_steps=16, load_codec=False)
    ge.set_logprobs(True)
    _check(_run(ge, prompts, "upstream"), refs("upstream", "q5_k_m"), "upstream q5_k_m")
    ge.close()


def test_mixed_batch_with_an_asynchronous_wave(gpu, tiny_model, prompts, refs):
    """four slots, two recording and two not; the second pair is admitted while the first runs, so it takes the asynchronous prefill"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_steps=16, load_codec=False)
    solo = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=False)
    want = {n: _run(solo, prompts, n)["codes"] for n in ("greedy", "sampled", "upstream")}
    solo.close()
    ge.set_logprobs(True)
    a = _submit(ge, prompts, "upstream")
    ge.set_logprobs(False)
    b = _submit(ge, prompts, "greedy")
    assert ge.sched_step()
    assert [ge.poll(r)["n_frames"] for r in (a, b)] == [4, 4]
    c = _submit(ge, prompts, "sampled")
    ge.set_logprobs(True)
    d = _submit(ge, prompts, "greedy")
    assert ge.sched_step()                                               # a and b run on; c and d are one asynchronous wave
    assert [ge.poll(r)["n_frames"] for r in (a, b, c, d)] == [8, 8, 0, 0]
    _drain(ge)
    assert [ge.records(r) for r in (a, b, c, d)] == [True, False, False, True]
    for rid, name in ((b, "greedy"), (c, "sampled")):
        with pytest.raises(gpu.Q3Error, match="does not record"):
            ge.fetch_logprobs(rid)
        assert np.array_equal(ge.result(rid)["codes"], want[name]), name
    for rid, name in ((a, "upstream"), (d, "greedy")):
        got = ge.result(rid)
        assert np.array_equal(got["codes"], want[name]), name
        _check(got, refs(name), name + " in the mixed batch")
    ge.close()


def test_fetch_and_fetch_logprobs_grow_together(gpu, tiny_model, prompts, refs):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    ge.set_logprobs(True)
    rid = _submit(ge, prompts, "sampled")
    seen_c, seen_l = np.zeros((0, 16), np.int32), np.zeros((0, 17), np.float32)
    for _ in range(64):
        busy = ge.sched_step()
        codes, _ = ge.fetch(rid, 0, 64)
        lp = ge.fetch_logprobs(rid, 0, 64)
        assert codes.shape[0] == lp.shape[0] == ge.poll(rid)["n_frames"]
        assert np.array_equal(codes[:seen_c.shape[0]], seen_c) and np.array_equal(lp[:seen_l.shape[0]], seen_l)   # fetched rows never change
        assert np.all(lp <= 0.0)                                         # a row is complete when it becomes visible
        tail = ge.fetch_logprobs(rid, max(lp.shape[0] - 1, 0), 64)
        assert np.array_equal(tail, lp[max(lp.shape[0] - 1, 0):])
        seen_c, seen_l = codes, lp
        if not busy:
            break
    assert seen_c.shape[0] == 12
    got = ge.result(rid)
    assert np.array_equal(got["logprobs"], seen_l)
    _check(got, refs("sampled"), "stepped by hand")
    ge.close()


def test_a_discarded_stalled_frame_leaves_no_trace(gpu, tiny_model, assets, vivian):
    """an open trail that makes the slot wait before its first frame, after one frame and inside a 4-frame group: the log-probabilities are
    those of the closed submission of the same text, bit for bit (same logits, same kernel)"""
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=24, load_codec=False)
    ge.set_logprobs(True)
    prompt, trail = assets.prompt_build_streaming(np.arange(300, 310, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    kw = dict(SAMPLED, **UPSTREAM)
    rid = ge.submit(prompt, max_steps=12, seed=77, mask_eos=True, trailing_ids=trail, **kw)
    assert ge.wait(rid, WAIT_MS)
    want = ge.result(rid)
    assert want["logprobs"].shape == (12, 17) and np.all(want["logprobs"] <= 0.0)
    for k in (0, 1, 5):
        rid = ge.submit(prompt, max_steps=12, seed=77, mask_eos=True, trailing_ids=trail[:k], open_trail=True, **kw)
        for _ in range(64):
            ge.sched_step()
            if ge.poll(rid)["n_frames"] >= k:
                break
        g0 = ge.stats()["graph_frames"]
        for _ in range(3):
            assert ge.sched_step()
        assert ge.poll(rid)["n_frames"] == k and ge.stats()["graph_frames"] == g0 and ge.fetch_logprobs(rid).shape == (k, 17)
        assert ge.trail_append(rid, trail[k:k + 2]) == 0                 # two frames, then it waits again
        for _ in range(4):
            assert ge.sched_step()
        assert ge.poll(rid)["n_frames"] == k + 2
        assert ge.trail_append(rid, trail[k + 2:], close=True) == 0
        _drain(ge)
        got = ge.result(rid)
        assert np.array_equal(got["codes"], want["codes"]), k
        assert np.array_equal(got["logprobs"], want["logprobs"]), (k, np.argwhere(got["logprobs"] != want["logprobs"])[:4])
    ge.close()


def test_cancel_then_resume(gpu, tiny_model, prompts, refs):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
    ge.set_logprobs(True)
    whole = _run(ge, prompts, "upstream")
    _check(whole, refs("upstream"), "uninterrupted")
    rid = _submit(ge, prompts, "upstream")
    for _ in range(2):
        assert ge.sched_step()
    assert ge.cancel(rid) is True
    _drain(ge)
    part = ge.result(rid)
    assert part["state"] == gpu.REQ_CANCELLED and part["codes"].shape == (8, 16)
    assert part["logprobs"].shape == (8, 17) and np.array_equal(part["logprobs"], whole["logprobs"][:8])   # exactly the rows of the frames it keeps
    for beside in (False, True):                                         # in-line prefix prefill, and asynchronous beside a running request
        if beside:
            other = _submit(ge, prompts, "sampled")
            assert ge.sched_step()
        res = _submit(ge, prompts, "upstream", prefix_codes=part["codes"][:6])
        assert ge.fetch_logprobs(res).shape == (6, 17) and np.all(ge.fetch_logprobs(res) == NONE)   # the prefix is there at once, uncomputed
        _drain(ge)
        got = ge.result(res)
        assert np.array_equal(got["codes"], whole["codes"]), beside
        assert np.all(got["logprobs"][:6] == NONE), beside
        # row 6 included: its columns 0 and 16 come from the prefix prefill's head
        assert np.array_equal(got["logprobs"][6:], whole["logprobs"][6:]), (beside, np.argwhere(got["logprobs"][6:] != whole["logprobs"][6:])[:4])
        if beside:
            _check(ge.result(other), refs("sampled"), "beside the resumed request")
    ge.close()


def test_slot_reuse_leaves_no_stale_rows(gpu, tiny_model, prompts, refs):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=16, load_codec=False)
    ge.set_logprobs(True)
    long_ = _submit(ge, prompts, "upstream")                             # 12 frames
    short = ge.submit(prompts["greedy"], max_steps=5, seed=42, mask_eos=True)
    resumed = _submit(ge, prompts, "greedy", prefix_codes=refs("greedy")[0][:9])
    _drain(ge)
    _check(ge.result(long_), refs("upstream"), "first in the slot")
    got = ge.result(short)
    codes, lp64 = refs("greedy")
    _check(got, (codes[:5], lp64[:5]), "shorter request in the same slot")
    assert got["logprobs"].shape == (5, 17)
    got = ge.result(resumed)
    assert np.array_equal(got["codes"], codes) and np.all(got["logprobs"][:9] == NONE)
    assert R.close(got["logprobs"][9:], lp64[9:])[0]
    ge.close()


def test_ggml_mode_refuses(gpu, tiny_model, prompts):
    old = os.environ.get("Q3_SPEC")
    os.environ["Q3_SPEC"] = "ggml"
    try:
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_steps=8, load_codec=False)
    finally:
        if old is None:
            os.environ.pop("Q3_SPEC")
        else:
            os.environ["Q3_SPEC"] = old
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.set_logprobs(True)
    ge.set_logprobs(False)                                               # switching it off is always fine
    rid = ge.submit(prompts["greedy"], max_steps=4)
    assert ge.wait(rid, WAIT_MS) and not ge.records(rid)
    ge.release(rid)
    ge.close()


def test_group_of_one_engine(gpu, tiny_model, prompts, refs):
    q3 = gpu
    L = q3.lib()
    p = q3.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 16, 0
    L.q3tts_group_create.argtypes = [C.POINTER(q3.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    devs = np.zeros(1, np.int32)
    g = C.c_void_p()
    q3._chk(L.q3tts_group_create(C.byref(p), q3._p(devs), 1, C.byref(g)))
    try:
        _, _, steps, seed, mask, kw = CASES["upstream"]
        prompt = np.ascontiguousarray(prompts["upstream"], np.float32)
        r = q3.Request()
        r.prompt, r.n_prompt, r.max_steps, r.mask_eos = prompt.ctypes.data, prompt.shape[0], steps, 1
        r.sampler = q3.SamplerConfig(kw["temperature"], kw["top_k"], kw["top_p"], 1, seed)
        o = q3.GenOptions(**UPSTREAM)
        plain, rec = C.c_int64(), C.c_int64()
        q3._chk(L.q3tts_group_submit_ex(g, C.byref(r), 0, C.byref(o), C.byref(plain)))
        q3.group_set_logprobs(g, True)
        q3._chk(L.q3tts_group_submit_ex(g, C.byref(r), 0, C.byref(o), C.byref(rec)))
        assert L.q3tts_group_wait(g, plain.value, WAIT_MS) == 0 and L.q3tts_group_wait(g, rec.value, WAIT_MS) == 0
        assert L.q3tts_group_fetch_logprobs(g, plain.value, None, 0, 0, None) < 0 and b"does not record" in L.q3tts_last_error()
        assert L.q3tts_group_fetch_logprobs(g, rec.value | 5, None, 0, 0, None) < 0          # an engine index the group does not have
        codes, gf, gp = np.zeros(steps * 16, np.int32), C.c_int32(), C.c_int64()
        q3._chk(L.q3tts_group_fetch(g, rec.value, q3._p(codes), 0, steps, None, 0, 0, C.byref(gf), C.byref(gp)))
        lp = q3.group_fetch_logprobs(g, rec.value)
        assert lp.shape == (gf.value, 17)
        _check({"codes": codes[: gf.value * 16].reshape(-1, 16), "logprobs": lp}, refs("upstream"), "through the group")
        q3._chk(L.q3tts_group_release(g, plain.value))
        q3._chk(L.q3tts_group_release(g, rec.value))
    finally:
        L.q3tts_group_destroy(g)
