"""[EXT] prompt stems on the GPU (q3tts_stem_*, q3tts_op_kv_stem; include/q3tts_spec.h "prompt stems").  The kernel against numpy: restored and
saved pages equal their sources bit for bit in both planes, and every other byte of the caches and of the store arena is unchanged.  The
engine: a request that takes a stem gives, bit for bit, the codes, log-probability rows and PCM of the same request on the same engine with no
stem set -- across stem and suffix lengths around the page size, graph and eager, two quantisations, sampler modes, the in-line lane and
asynchronous waves -- and every such case also checks q3tts_request_stem and the rows-not-prefilled counter, so a silent fall-back fails.
Then mixed waves, the other submission forms, cancels, the lifecycle, groups and the full-size model.  Every comparison is bit equality; the
scheduler is stepped by hand where order matters and every wait is bounded."""
import ctypes as C
import os

import numpy as np
import pytest

import synth_models

pytestmark = pytest.mark.gpu
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
MODES = (("greedy", {}), ("sampled", SAMPLED), ("options", dict(SAMPLED, **UPSTREAM)))
WAIT_MS = 60000.0
STEMS, SUFFIXES = (1, 63, 64, 65, 128, 200), (1, 2, 40)


def _steps(ge, n):
    for _ in range(n):
        assert ge.sched_step()


def _drain(ge, limit=4000):
    for _ in range(limit):
        if not ge.sched_step():
            return
    raise AssertionError("the scheduler did not go idle")


def _rows(ge, vivian, seed, n):
    """n distinct-looking prompt rows, cut or tiled from build_core rows"""
    rng = np.random.default_rng(seed)
    base = ge.assets.build_core(rng.integers(0, 4000, 9).astype(np.int32), lang_id=2055, spk_emb=vivian)
    return np.ascontiguousarray(base[np.arange(n) % base.shape[0]] * np.float32(1.0 + (seed % 7) / 64.0), np.float32)


def _ready(ge, gpu, rows):
    sid = ge.stem_create(rows)
    assert ge.stem_wait(sid, WAIT_MS) and ge.stem_poll(sid) == (gpu.STEM_READY, rows.shape[0])
    return sid


def _delta(ge, before):
    now = ge.stem_stats()
    return {k: now[k] - before[k] for k in now}


def _env(name, value):
    class Env:
        def __enter__(self):
            self.old = os.environ.get(name)
            if value is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = value

        def __exit__(self, *a):
            if self.old is None:
                os.environ.pop(name, None)
            else:
                os.environ[name] = self.old
    return Env()


def _same(a, b, what):
    assert a["state"] == b["state"] and a["codes"].shape == b["codes"].shape and np.array_equal(a["codes"], b["codes"]), what
    assert ("logprobs" in a) == ("logprobs" in b), what
    if "logprobs" in a:
        assert np.array_equal(a["logprobs"], b["logprobs"]), what
    if a.get("pcm") is not None or b.get("pcm") is not None:
        assert a["pcm"].size == b["pcm"].size > 0 and np.array_equal(a["pcm"], b["pcm"]), what


# ---------------------------------------------------------------- the kernel ----------------------------------------------------------------
def _world(seed, n_layer, n_kv, n_slots, pages_per_slot, n_store):
    """a pool whose slots own scrambled pages, one guard page nobody owns at either end and one in the middle, one guard slot (the last) that
    no job names, and a store arena"""
    rng = np.random.default_rng(seed)
    n_pages = n_slots * pages_per_slot + 3
    owned = [p for p in rng.permutation(n_pages - 2) + 1]
    owned.remove(int(owned[len(owned) // 2]))                            # the middle guard
    pt = np.array(owned[:n_slots * pages_per_slot], np.int32).reshape(n_slots, pages_per_slot)
    shape = (n_pages, n_layer, n_kv, 8192)
    k, v = rng.integers(0, 65536, shape, dtype=np.uint16), rng.integers(0, 65536, shape, dtype=np.uint16)
    sshape = (n_store, n_layer, n_kv, 8192)
    sk, sv = rng.integers(0, 65536, sshape, dtype=np.uint16), rng.integers(0, 65536, sshape, dtype=np.uint16)
    return k, v, pt, sk, sv


def _numpy_stem(k, v, pt, sk, sv, jobs, save):
    wk, wv, wsk, wsv = k.copy(), v.copy(), sk.copy(), sv.copy()
    for page0, n, slots in jobs:
        for lp in range(n):
            if save:
                wsk[page0 + lp], wsv[page0 + lp] = k[pt[slots[0], lp]], v[pt[slots[0], lp]]
            else:
                for b in slots:
                    wk[pt[b, lp]], wv[pt[b, lp]] = sk[page0 + lp], sv[page0 + lp]
    return wk, wv, wsk, wsv


def _check_stem(gpu, world, jobs, save):
    k, v, pt, sk, sv = world
    got = gpu.op_kv_stem(k, v, pt, sk, sv, jobs, save)
    want = _numpy_stem(k, v, pt, sk, sv, jobs, save)
    # the named pages equal their sources; every other byte -- guard pages, the guard slot, later pages, the rest of the arena -- is unchanged
    for g, w, name in zip(got, want, ("k", "v", "store k", "store v")):
        assert np.array_equal(g, w), (name, jobs, save)
    assert not np.array_equal(got[2] if save else got[0], sk if save else k)   # something was copied
    return got


JOB_SHAPES = {
    "one job": lambda n: [(0, n, [1])],
    "three jobs": lambda n: [(0, n, [2]), (n + 1, max(1, n - 1), [0]), (2 * n + 1, 1, [3])],
    "one stem to three slots": lambda n: [(1, n, [3, 0, 2])],
}


@pytest.mark.parametrize("shape", sorted(JOB_SHAPES))
@pytest.mark.parametrize("n_pages", [1, 2, 5])
def test_op_kv_stem_tiny_geometry(gpu, n_pages, shape):
    world = _world(100 + n_pages, 2, 2, 5, 5, 3 * 5 + 2)                  # slot 4 is the guard slot
    jobs = JOB_SHAPES[shape](n_pages)
    _check_stem(gpu, world, jobs, False)
    if shape != "one stem to three slots":
        _check_stem(gpu, world, jobs, True)


@pytest.mark.parametrize("n_pages,shape", [(1, "one job"), (2, "three jobs"), (5, "one stem to three slots")])
def test_op_kv_stem_talker_geometry(gpu, n_pages, shape):
    """28 layers x 8 kv heads: 224 tiles a plane page over a grid row of fewer workgroups"""
    world = _world(200 + n_pages, 28, 8, 4, n_pages, 2 * n_pages + 2)      # slot 3 is the guard slot of the last case
    jobs = JOB_SHAPES[shape](n_pages)
    if shape == "one stem to three slots":
        jobs = [(1, n_pages, [2, 0, 1])]
    _check_stem(gpu, world, jobs, False)


@pytest.mark.parametrize("n_layer,n_kv", [(2, 2), (28, 8)])
def test_op_kv_stem_save_then_restore_round_trips(gpu, n_layer, n_kv):
    k, v, pt, sk, sv = _world(300 + n_layer, n_layer, n_kv, 4, 2, 4)
    k1, v1, sk1, sv1 = _check_stem(gpu, (k, v, pt, sk, sv), [(1, 2, [2])], True)
    assert np.array_equal(k1, k) and np.array_equal(v1, v)
    k2, v2, sk2, sv2 = _check_stem(gpu, (k1, v1, pt, sk1, sv1), [(1, 2, [0, 1])], False)
    for b in (0, 1):
        for lp in range(2):
            assert np.array_equal(k2[pt[b, lp]], k[pt[2, lp]]) and np.array_equal(v2[pt[b, lp]], v[pt[2, lp]])
    assert np.array_equal(sk2, sk1) and np.array_equal(sv2, sv1)


# ------------------------------------------------------- stemmed equals plain, in line -------------------------------------------------------
class World:
    """one engine, its stems by length and the plain runs of every prompt used (same engine, no stem set), computed once"""

    def __init__(self, gpu, model, vivian, quant="q8_0", use_graph=True, max_batch=1, load_codec=False, max_steps=24):
        self.gpu, self.vivian = gpu, vivian
        self.ge = gpu.Engine(model, quant, max_batch=max_batch, max_prompt=256, max_steps=max_steps, load_codec=load_codec, use_graph=use_graph)
        self.heads, self.sids, self.plain = {}, {}, {}

    def stem(self, n):
        if n not in self.sids:
            self.heads[n] = _rows(self.ge, self.vivian, 1000 + n, n)
            self.sids[n] = _ready(self.ge, self.gpu, self.heads[n])
        return self.sids[n]

    def prompt(self, n, suffix, seed=0):
        self.stem(n)
        return np.concatenate([self.heads[n], _rows(self.ge, self.vivian, 5000 + 7 * n + suffix + 100 * seed, suffix)])

    def run_plain(self, key, prompt, steps=8, seed=11, want_pcm=False, **kw):
        if key not in self.plain:
            self.ge.set_stem(None)
            rid = self.ge.submit(prompt, max_steps=steps, seed=seed, mask_eos=True, want_pcm=want_pcm, **kw)
            assert self.ge.request_stem(rid) == (-1, 0)
            _drain(self.ge)
            self.plain[key] = self.ge.result(rid, want_pcm=want_pcm)
        return self.plain[key]

    def submit_stemmed(self, n, prompt, steps=8, seed=11, want_pcm=False, **kw):
        self.ge.set_stem(self.stem(n))
        rid = self.ge.submit(prompt, max_steps=steps, seed=seed, mask_eos=True, want_pcm=want_pcm, **kw)
        self.ge.set_stem(None)
        assert self.ge.request_stem(rid) == (self.sids[n], n), n
        return rid

    def close(self):
        self.ge.close()


@pytest.mark.parametrize("quant", ["q8_0", "q5_k_m"])
@pytest.mark.parametrize("use_graph", [True, False])
def test_stemmed_equals_plain_in_line(gpu, tiny_model, vivian, quant, use_graph):
    w = World(gpu, tiny_model, vivian, quant, use_graph)
    ge = w.ge
    w.stem(1)
    page = ge.stem_stats()["device_bytes"]                                # one page in both planes, whatever the tiny talker's geometry is
    assert page > 0 and page % (2 * 8192 * 2) == 0
    for n in STEMS:
        for suffix in SUFFIXES:
            prompt = w.prompt(n, suffix)
            for name, kw in MODES:
                ge.set_logprobs(name == "options")
                want = w.run_plain((n, suffix, name), prompt, **kw)
                before = ge.stem_stats()
                rid = w.submit_stemmed(n, prompt, **kw)
                _drain(ge)
                assert _delta(ge, before) == dict(built=0, restores=1, rows_not_prefilled=n, pages_copied=(n + 63) // 64, mismatches=0,
                                                  device_bytes=0), (n, suffix, name)
                got = ge.result(rid)
                assert got["state"] == gpu.REQ_DONE and got["codes"].shape == (8, 16)
                _same(got, want, (n, suffix, name))
                if name == "options":
                    assert got["logprobs"].shape == (8, 17)
    st = ge.stem_stats()
    assert st["built"] == len(STEMS) and st["device_bytes"] == sum((n + 63) // 64 for n in STEMS) * page
    w.close()


def test_pcm_is_bit_equal_and_the_oracle_agrees_on_a_clone_voice(gpu, oracle, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, load_codec=True)
    ge = w.ge
    prompt = w.prompt(65, 40)
    want = w.run_plain("pcm", prompt, steps=9, want_pcm=True, **SAMPLED)
    rid = w.submit_stemmed(65, prompt, steps=9, want_pcm=True, **SAMPLED)
    _drain(ge)
    got = ge.result(rid, want_pcm=True)
    assert got["pcm"].size == 9 * 1920
    _same(got, want, "pcm")
    # a clone voice through the text form, stemmed, against the CPU oracle on the prompt the builder makes
    rng = np.random.default_rng(77)
    ref_codes, ref_text, text = rng.integers(0, 2048, (70, 16)).astype(np.int32), rng.integers(0, 4000, 5).astype(np.int32), rng.integers(0, 4000, 7).astype(np.int32)
    vid = ge.register_voice(vivian, ref_codes, ref_text)
    sid = ge.stem_voice(vid, timeout_ms=WAIT_MS)
    full = ge.assets.build_clone(text, ref_codes.reshape(-1), ref_text, vivian)
    n = ge.stem_poll(sid)[1]
    assert n == full.shape[0] - (text.size + 2) and n > 64
    rid = ge.submit_text(vid, text, max_steps=6, temperature=0.0, seed=42, mask_eos=True)
    assert ge.request_stem(rid) == (sid, n)
    _drain(ge)
    got = ge.result(rid)
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), None, 4)
    oc, _ = oe.generate(full, max_steps=6, mask_eos=True)
    oe.close()
    assert np.array_equal(got["codes"], oc)
    w.close()


# ------------------------------------------------------- asynchronous waves, mixed batches -------------------------------------------------------
@pytest.mark.parametrize("async_env", [None, "0"])
def test_stemmed_equals_plain_beside_running_requests(gpu, tiny_model, vivian, async_env):
    """a wave admitted while a request runs: asynchronously on the second lane, or -- Q3_ASYNC_PREFILL=0 -- in line between two frame groups"""
    with _env("Q3_ASYNC_PREFILL", async_env):
        w = World(gpu, tiny_model, vivian, max_batch=4, max_steps=40)
    ge = w.ge
    bg_prompt = _rows(ge, vivian, 31, 12)
    for n, suffix in ((1, 1), (64, 2), (65, 40), (200, 1), (200, 40)):
        prompt = w.prompt(n, suffix)
        for name, kw in MODES:
            ge.set_logprobs(name == "options")
            want = w.run_plain((n, suffix, name), prompt, **kw)
            bg = ge.submit(bg_prompt, max_steps=40, seed=3, mask_eos=True, **SAMPLED)
            _steps(ge, 1)
            before = ge.stem_stats()
            rid = w.submit_stemmed(n, prompt, **kw)
            _steps(ge, 1)
            if async_env is None:
                assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"]) == (gpu.REQ_RUNNING, 0)     # inside the asynchronous wave
            assert ge.wait(rid, WAIT_MS)
            assert _delta(ge, before) == dict(built=0, restores=1, rows_not_prefilled=n, pages_copied=(n + 63) // 64, mismatches=0, device_bytes=0)
            _same(ge.result(rid), want, (n, suffix, name, async_env))
            assert ge.cancel(bg) is True
            _drain(ge)
            ge.release(bg)
    w.close()


def test_a_mixed_asynchronous_wave_then_slot_reuse(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, max_batch=8, max_steps=40)
    ge = w.ge
    pa, pb, pc = w.prompt(65, 40), w.prompt(65, 2, seed=1), w.prompt(128, 40)
    pu = _rows(ge, vivian, 41, 70)                                        # unstemmed: no stem is set when it is submitted
    pm = pa.copy()
    pm[64, 2047] = np.nextafter(pm[64, 2047], np.float32(np.inf))          # one float of the last stem row differs
    want = dict(a=w.run_plain("a", pa, steps=10, seed=21, **SAMPLED), b=w.run_plain("b", pb, steps=8, seed=22),
                c=w.run_plain("c", pc, steps=12, seed=23, **dict(SAMPLED, **UPSTREAM)), u=w.run_plain("u", pu, steps=9, seed=24, **SAMPLED),
                m=w.run_plain("m", pm, steps=10, seed=21, **SAMPLED))
    bg = ge.submit(_rows(ge, vivian, 42, 9), max_steps=40, seed=5, mask_eos=True, **SAMPLED)
    _steps(ge, 1)
    before = ge.stem_stats()
    ra = w.submit_stemmed(65, pa, steps=10, seed=21, **SAMPLED)
    rb = w.submit_stemmed(65, pb, steps=8, seed=22)
    ru = ge.submit(pu, max_steps=9, seed=24, mask_eos=True, **SAMPLED)
    rc = w.submit_stemmed(128, pc, steps=12, seed=23, **dict(SAMPLED, **UPSTREAM))
    ge.set_stem(w.sids[65])
    rm = ge.submit(pm, max_steps=10, seed=21, mask_eos=True, **SAMPLED)
    ge.set_stem(None)
    assert ge.request_stem(rm) == (-1, 0) and ge.request_stem(ru) == (-1, 0)
    _steps(ge, 1)
    assert [(ge.poll(r)["state"], ge.poll(r)["n_frames"]) for r in (ra, rb, ru, rc, rm)] == [(gpu.REQ_RUNNING, 0)] * 5   # one wave holds them all
    for r in (ra, rb, ru, rc, rm):
        assert ge.wait(r, WAIT_MS)
    # two restores of one stem in one job, a second stem in a second job, one mismatch that ran plain
    assert _delta(ge, before) == dict(built=0, restores=3, rows_not_prefilled=65 + 65 + 128, pages_copied=2 + 2 + 2, mismatches=1, device_bytes=0)
    for key, r in (("a", ra), ("b", rb), ("u", ru), ("c", rc), ("m", rm)):
        _same(ge.result(r), want[key], key)
    ge.cancel(bg)
    _drain(ge)
    ge.release(bg)
    # the slots and pages they used serve plain and stemmed requests as before
    rids = [w.submit_stemmed(65, pa, steps=10, seed=21, **SAMPLED), ge.submit(pu, max_steps=9, seed=24, mask_eos=True, **SAMPLED),
            w.submit_stemmed(128, pc, steps=12, seed=23, **dict(SAMPLED, **UPSTREAM)), ge.submit(pm, max_steps=10, seed=21, mask_eos=True, **SAMPLED),
            w.submit_stemmed(65, pb, steps=8, seed=22)]
    _drain(ge)
    for key, r in zip("aucmb", rids):
        _same(ge.result(r), want[key], "reuse " + key)
    w.close()


# ------------------------------------------------------------- the other forms -------------------------------------------------------------
def test_text_forms_take_their_voices_stem(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_prompt=256, max_steps=24, load_codec=False)
    rng = np.random.default_rng(88)
    ref_codes, ref_text = rng.integers(0, 2048, (60, 16)).astype(np.int32), rng.integers(0, 4000, 4).astype(np.int32)
    text, instr = rng.integers(0, 4000, 6).astype(np.int32), rng.integers(0, 4000, 3).astype(np.int32)
    clone, preset = ge.register_voice(vivian, ref_codes, ref_text), ge.register_voice(vivian)

    def run(v, **kw):
        rid = ge.submit_text(v, text, max_steps=8, seed=9, mask_eos=True, **kw)
        took = ge.request_stem(rid)
        if kw.get("open_text"):
            _steps(ge, 1)
            ge.text_append(rid, rng2.integers(0, 4000, 4).astype(np.int32), is_last=True)
        _drain(ge)
        return took, ge.result(rid)

    forms = (dict(SAMPLED), dict(SAMPLED, streaming_text=True), dict(SAMPLED, streaming_text=True, open_text=True), dict(SAMPLED, lang_id=2050),
             dict(SAMPLED, instr_ids=instr))
    plain = {}
    for v in (clone, preset):
        for i, kw in enumerate(forms):
            rng2 = np.random.default_rng(5)
            plain[v, i] = run(v, **kw)
            assert plain[v, i][0] == (-1, 0)
    sids = {v: ge.stem_voice(v, timeout_ms=WAIT_MS) for v in (clone, preset)}
    ns = {v: ge.stem_poll(sids[v])[1] for v in sids}
    assert ns[clone] == ns[preset] + (ref_text.size + 2) + (60 + 2) and ns[preset] == 3 + 4 + 1 + 1   # role, control, speaker, text BOS
    ge.set_stem(sids[clone])                                              # the engine-level setting does not apply to text forms
    for v in (clone, preset):
        for i, kw in enumerate(forms):
            rng2 = np.random.default_rng(5)
            before = ge.stem_stats()
            took, got = run(v, **kw)
            falls_back = i >= 3                                           # a changed lang_id or an instruction makes other rows
            assert took == ((-1, 0) if falls_back else (sids[v], ns[v])), (v, i)
            d = _delta(ge, before)
            assert (d["restores"], d["rows_not_prefilled"], d["mismatches"]) == ((0, 0, 1) if falls_back else (1, ns[v], 0)), (v, i)
            _same(got, plain[v, i][1], (v, i))
    ge.set_stem(None)
    # a stem made for the instruction is taken by requests with it, and by no others
    sid_i = ge.voice_stem_create(clone, 2055, instr)
    assert ge.stem_wait(sid_i, WAIT_MS)
    ge.voice_set_stem(clone, sid_i)
    ge.stem_release(sid_i)
    took, got = run(clone, **forms[4])
    assert took == (sid_i, ns[clone] + 3 + instr.size + 2)
    _same(got, plain[clone, 4][1], "instruction")
    assert run(clone, **forms[0])[0] == (-1, 0)
    for v in (clone, preset):
        ge.voice_set_stem(v, None)
    _drain(ge)
    assert ge.stem_stats()["device_bytes"] == 0
    ge.close()


def test_candidate_sets_restore_then_fork(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, max_batch=4, max_steps=24)
    ge = w.ge
    seeds = [901, 902, 903]
    for n, suffix in ((65, 2), (128, 40)):
        prompt = w.prompt(n, suffix)
        want = [w.run_plain((n, s), prompt, seed=s, **SAMPLED) for s in seeds]
        before, cbefore = ge.stem_stats(), ge.candidate_stats()
        ge.set_stem(w.sids[n])
        ids = ge.submit_candidates(prompt, seeds, max_steps=8, **SAMPLED)
        ge.set_stem(None)
        assert [ge.request_stem(r) for r in ids] == [(w.sids[n], n)] * 3
        _drain(ge)
        d = _delta(ge, before)
        assert (d["restores"], d["rows_not_prefilled"], d["pages_copied"]) == (1, n, (n + 63) // 64)   # the first member; the others are forked
        assert ge.candidate_stats()["pages_copied"] - cbefore["pages_copied"] == 2 * ((n + suffix + 63) // 64)
        for r, wnt in zip(ids, want):
            _same(ge.result(r), wnt, (n, suffix))
    # the first member leaves in the queue: the second one is restored
    prompt = w.prompt(65, 2)
    ge.set_stem(w.sids[65])
    ids = ge.submit_candidates(prompt, seeds, max_steps=8, **SAMPLED)
    ge.set_stem(None)
    assert ge.cancel(ids[0]) is True
    _drain(ge)
    for r, s in zip(ids[1:], seeds[1:]):
        _same(ge.result(r), w.plain[65, s], s)
    ge.release(ids[0])
    w.close()


@pytest.mark.parametrize("n_prompt,k", [(120, 8), (122, 8), (66, 5)])
def test_resume_behind_a_stem(gpu, tiny_model, vivian, n_prompt, k):
    """n_prompt + k = 128: the feedback rows end at a page boundary; 130 and 71: off one"""
    w = World(gpu, tiny_model, vivian, max_batch=2, max_steps=24)
    ge = w.ge
    prompt = w.prompt(65, n_prompt - 65)
    whole = w.run_plain("whole", prompt, steps=16, seed=33, **SAMPLED)
    ge.set_logprobs(True)
    want = w.run_plain("resumed", prompt, steps=16, seed=33, prefix_codes=whole["codes"][:k], **SAMPLED)
    assert np.array_equal(want["codes"], whole["codes"])
    rid = w.submit_stemmed(65, prompt, steps=16, seed=33, prefix_codes=whole["codes"][:k], **SAMPLED)
    _drain(ge)
    _same(ge.result(rid), want, (n_prompt, k))
    w.close()


def test_cancel_inside_the_wave_and_mid_utterance(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, max_batch=4, max_steps=40)
    ge = w.ge
    prompt = w.prompt(128, 2)
    want = w.run_plain("p", prompt, steps=16, seed=44, **SAMPLED)
    bg = ge.submit(_rows(ge, vivian, 61, 9), max_steps=40, seed=6, mask_eos=True, **SAMPLED)
    _steps(ge, 1)
    rid = w.submit_stemmed(128, prompt, steps=16, seed=44, **SAMPLED)
    keep = w.submit_stemmed(128, prompt, steps=16, seed=44, **SAMPLED)
    _steps(ge, 1)
    assert (ge.poll(rid)["state"], ge.poll(rid)["n_frames"]) == (gpu.REQ_RUNNING, 0)                 # inside the wave
    assert ge.cancel(rid) is True
    assert ge.wait(keep, WAIT_MS) and ge.wait(rid, WAIT_MS)
    st = ge.poll(rid)
    assert (st["state"], st["n_frames"]) == (gpu.REQ_CANCELLED, 0)
    ge.release(rid)
    _same(ge.result(keep), want, "wave-mate")
    rid = w.submit_stemmed(128, prompt, steps=16, seed=44, **SAMPLED)                                 # mid-utterance
    while ge.poll(rid)["n_frames"] < 8:
        _steps(ge, 1)
    assert ge.cancel(rid) is True
    assert ge.wait(rid, WAIT_MS)
    got = ge.result(rid)
    nf = got["codes"].shape[0]
    assert got["state"] == gpu.REQ_CANCELLED and 8 <= nf < 16 and np.array_equal(got["codes"], want["codes"][:nf])
    ge.cancel(bg)
    _drain(ge)
    ge.release(bg)
    # every hold was dropped: releasing the creator's reference frees the store
    ge.stem_release(w.sids[128])
    _drain(ge)
    ge.sched_step()
    assert ge.stem_stats()["device_bytes"] == 0
    with pytest.raises(gpu.Q3Error, match="unknown stem"):
        ge.stem_poll(w.sids[128])
    w.close()


def test_a_preamble_together_with_a_stem(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, max_batch=2, load_codec=True)
    ge = w.ge
    pre = np.random.default_rng(9).integers(0, 2048, (6, 16)).astype(np.int32)
    pid = ge.preamble_create(pre)
    assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid)[0] == gpu.PREAMBLE_READY
    ge.set_preamble(pid)
    prompt = w.prompt(64, 40)
    want = w.run_plain("primed", prompt, steps=9, want_pcm=True, **SAMPLED)
    rid = w.submit_stemmed(64, prompt, steps=9, want_pcm=True, **SAMPLED)
    assert ge.request_preamble(rid) == pid
    _drain(ge)
    _same(ge.result(rid, want_pcm=True), want, "primed")
    ge.set_preamble(None)
    cold = w.run_plain("cold", prompt, steps=9, want_pcm=True, **SAMPLED)
    assert np.array_equal(cold["codes"], want["codes"]) and not np.array_equal(cold["pcm"], want["pcm"])   # the preamble did prime the PCM
    w.close()


def test_score_requests_and_blocking_batches_never_take_a_stem(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, max_batch=2)
    ge = w.ge
    prompt = w.prompt(65, 2)
    want = w.run_plain("p", prompt)
    ge.set_stem(w.sids[65])
    before = ge.stem_stats()
    rid = ge.submit_score(prompt, want["codes"])
    assert ge.request_stem(rid) == (-1, 0)
    _drain(ge)
    ge.release(rid)
    got = ge.generate_batch([prompt], max_steps=8, mask_eos=True, seed=11)[0]
    assert np.array_equal(got["codes"], want["codes"])
    assert _delta(ge, before) == dict(built=0, restores=0, rows_not_prefilled=0, pages_copied=0, mismatches=0, device_bytes=0)
    for bad in (prompt[:65], prompt[:64]):                               # n_prompt == n and below: plain, counted
        rid = ge.submit(bad, max_steps=4, seed=1, mask_eos=True)
        assert ge.request_stem(rid) == (-1, 0)
        _drain(ge)
        ge.release(rid)
    assert _delta(ge, before)["mismatches"] == 2
    w.close()


# ---------------------------------------------------------------- lifecycle ----------------------------------------------------------------
def test_release_while_a_queued_request_holds_the_stem(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian)
    ge = w.ge
    prompt = w.prompt(65, 2)
    want = w.run_plain("p", prompt, **SAMPLED)
    sid = w.sids[65]
    with pytest.raises(gpu.Q3Error, match="unknown stem"):
        ge.set_stem(sid + 1)
    rid = w.submit_stemmed(65, prompt, **SAMPLED)                         # queued: no step has run; the engine-level setting is gone again
    ge.stem_release(sid)
    with pytest.raises(gpu.Q3Error, match="already been released"):
        ge.stem_release(sid)
    assert ge.stem_poll(sid) == (gpu.STEM_READY, 65)                      # the request holds it
    assert ge.stem_stats()["device_bytes"] > 0
    _drain(ge)
    _same(ge.result(rid), want, "held")
    ge.sched_step()                                                       # the scheduler frees the store
    assert ge.stem_stats()["device_bytes"] == 0
    with pytest.raises(gpu.Q3Error, match="unknown stem"):
        ge.stem_poll(sid)
    rid = ge.submit(prompt, max_steps=8, seed=11, mask_eos=True, **SAMPLED)
    assert ge.request_stem(rid) == (-1, 0)
    _drain(ge)
    _same(ge.result(rid), want, "after")
    # a stem released while it builds is recycled when the build ends; a setter refuses a building stem
    sid2 = ge.stem_create(w.heads[65])
    with pytest.raises(gpu.Q3Error, match="building"):
        ge.set_stem(sid2)
    assert sid2 == sid + 1 and ge.stem_poll(sid2) == (gpu.STEM_BUILDING, 65)
    ge.stem_release(sid2)
    _drain(ge)
    ge.sched_step()
    with pytest.raises(gpu.Q3Error, match="unknown stem"):
        ge.stem_poll(sid2)
    assert ge.stem_stats()["device_bytes"] == 0 and ge.stem_stats()["built"] == 2
    w.close()


def test_the_65th_stem_is_refused_until_one_is_released(gpu, tiny_model, vivian):
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=4, max_prompt=256, max_steps=8, load_codec=False)
    rows = _rows(ge, vivian, 70, 3)
    for bad, why in ((None, "rows missing"), (rows[:0], "rows missing|n_rows"), (_rows(ge, vivian, 71, 256), "below max_prompt")):
        with pytest.raises(gpu.Q3Error, match=why):
            ge.stem_create(bad)
    sids = [ge.stem_create(rows[:1 + i % 3]) for i in range(gpu.MAX_STEMS)]
    assert sids == list(range(gpu.MAX_STEMS))
    with pytest.raises(gpu.Q3Error, match="Q3TTS_MAX_STEMS"):
        ge.stem_create(rows)
    for s in sids:
        assert ge.stem_wait(s, WAIT_MS) and ge.stem_poll(s)[0] == gpu.STEM_READY
    assert ge.stem_stats()["built"] == 64 and ge.stem_stats()["device_bytes"] > 0 and ge.stem_stats()["device_bytes"] % 64 == 0   # one page each
    with pytest.raises(gpu.Q3Error, match="Q3TTS_MAX_STEMS"):
        ge.stem_create(rows)
    ge.stem_release(sids[10])
    new = ge.stem_create(rows)
    assert new == gpu.MAX_STEMS                                           # ids are never reused
    assert ge.stem_wait(new, WAIT_MS)
    for s in sids[:10] + sids[11:] + [new]:
        ge.stem_release(s)
    ge.sched_step()
    assert ge.stem_stats()["device_bytes"] == 0 and not ge.sched_step()
    ge.close()


def test_under_the_driver_thread(gpu, tiny_model, vivian):
    w = World(gpu, tiny_model, vivian, max_batch=2)
    ge = w.ge
    head = _rows(ge, vivian, 80, 130)
    prompt = np.concatenate([head, _rows(ge, vivian, 81, 5)])
    want = w.run_plain("p", prompt, **SAMPLED)
    ge.sched_start()
    try:
        sid = ge.stem_create(head)
        assert ge.stem_wait(sid, WAIT_MS) and ge.stem_poll(sid) == (gpu.STEM_READY, 130)
        ge.set_stem(sid)
        rids = [ge.submit(prompt, max_steps=8, seed=11, mask_eos=True, **SAMPLED) for _ in range(3)]
        ge.set_stem(None)
        ge.stem_release(sid)
        for rid in rids:
            assert ge.wait(rid, WAIT_MS) and ge.request_stem(rid) == (sid, 130)
            _same(ge.result(rid), want, "driver")
    finally:
        ge.sched_stop()
    ge.sched_step()
    with pytest.raises(gpu.Q3Error, match="unknown stem"):
        ge.stem_poll(sid)
    assert ge.stem_stats()["device_bytes"] == 0
    w.close()


def test_ggml_mode_refuses_create(gpu, tiny_model, vivian):
    with _env("Q3_SPEC", "ggml"):
        ge = gpu.Engine(tiny_model, "q8_0", max_batch=1, max_prompt=256, max_steps=16, load_codec=False)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.stem_create(_rows(ge, vivian, 90, 5))
    vid = ge.register_voice(vivian)
    with pytest.raises(gpu.Q3Error, match="Q3_SPEC=ggml"):
        ge.voice_stem_create(vid)
    assert not ge.sched_step() and ge.stem_stats()["built"] == 0
    ge.close()


@pytest.mark.parametrize("n_eng", (1, 2))
def test_groups_on_one_device(gpu, tiny_model, vivian, n_eng):
    L = gpu.lib()
    p = gpu.EngineParams()
    L.q3tts_engine_params_default(C.byref(p))
    p.model_dir, p.quant, p.max_batch, p.max_prompt, p.max_steps, p.load_codec = tiny_model.encode(), b"q8_0", 2, 256, 16, 0
    L.q3tts_group_create.argtypes = [C.POINTER(gpu.EngineParams), C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.q3tts_group_destroy.argtypes = [C.c_void_p]
    L.q3tts_group_engine.restype = C.c_void_p
    L.q3tts_group_engine.argtypes = [C.c_void_p, C.c_int32]
    L.q3tts_group_wait.argtypes = [C.c_void_p, C.c_int64, C.c_double]
    L.q3tts_group_fetch.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int64,
                                    C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    L.q3tts_group_release.argtypes = [C.c_void_p, C.c_int64]
    L.q3tts_group_submit.argtypes = [C.c_void_p, C.POINTER(gpu.Request), C.c_int32, C.POINTER(C.c_int64)]
    L.q3tts_group_voice_register.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]
    devs, g = np.zeros(n_eng, np.int32), C.c_void_p()
    gpu._chk(L.q3tts_group_create(C.byref(p), gpu._p(devs), n_eng, C.byref(g)))
    try:
        assets = gpu.Assets(handle=L.q3tts_engine_assets(L.q3tts_group_engine(g, 0)))
        rng = np.random.default_rng(150)
        base = assets.build_core(rng.integers(0, 4000, 9).astype(np.int32), lang_id=2055, spk_emb=vivian)
        prompt = np.ascontiguousarray(base[np.arange(70) % base.shape[0]], np.float32)
        gf, gp = C.c_int32(), C.c_int64()

        def run(text=None):
            out = []
            for _ in range(n_eng):                                        # round robin: one on every engine
                rid = C.c_int64()
                if text is None:
                    r = gpu.Request()
                    r.prompt, r.n_prompt, r.max_steps, r.mask_eos = prompt.ctypes.data, 70, 8, 1
                    r.sampler.temperature, r.sampler.top_k, r.sampler.top_p, r.sampler.has_seed, r.sampler.seed = 0.9, 50, 1.0, 1, 7
                    gpu._chk(L.q3tts_group_submit(g, C.byref(r), 0, C.byref(rid)))
                else:
                    sc = gpu.SamplerConfig(0.9, 50, 1.0, 1, 7)
                    gpu._chk(L.q3tts_group_submit_text_ex(g, vid.value, gpu._p(text), text.size, 2055, None, 0, C.byref(sc), 8, 1, 0, None, C.byref(rid)))
                took = gpu.group_request_stem(g, rid.value)
                assert L.q3tts_group_wait(g, rid.value, WAIT_MS) == 0
                codes = np.zeros((8, 16), np.int32)
                gpu._chk(L.q3tts_group_fetch(g, rid.value, gpu._p(codes), 0, 8, None, 0, 0, C.byref(gf), C.byref(gp)))
                assert gf.value == 8
                gpu._chk(L.q3tts_group_release(g, rid.value))
                out.append((took, codes))
            return out

        plain = run()
        assert all(t == (-1, 0) for t, _ in plain)
        sid = gpu.group_stem_create(g, prompt[:65])
        assert sid == 0
        with pytest.raises(gpu.Q3Error, match="building"):                # no engine has stepped: all engines or none
            gpu.group_set_stem(g, sid)
        assert gpu.group_stem_wait(g, sid, WAIT_MS)
        gpu.group_set_stem(g, sid)
        got = run()
        for (t, c), (_, wc) in zip(got, plain):
            assert t == (sid, 65) and np.array_equal(c, wc)
        st = gpu.group_stem_stats(g)
        assert (st["built"], st["restores"], st["rows_not_prefilled"], st["mismatches"]) == (n_eng, n_eng, 65 * n_eng, 0)
        gpu.group_set_stem(g, None)
        gpu.group_stem_release(g, sid)
        # a voice's stem through the group
        vid = C.c_int32()
        ref_codes, ref_text, text = rng.integers(0, 2048, (20, 16)).astype(np.int32), rng.integers(0, 4000, 3).astype(np.int32), rng.integers(0, 4000, 5).astype(np.int32)
        gpu._chk(L.q3tts_group_voice_register(g, gpu._p(vivian), gpu._p(ref_codes), ref_codes.size, gpu._p(ref_text), ref_text.size, C.byref(vid)))
        plain = run(text)
        vsid = gpu.group_voice_stem_create(g, vid.value)
        assert vsid == 1 and gpu.group_stem_wait(g, vsid, WAIT_MS)
        gpu.group_voice_set_stem(g, vid.value, vsid)
        gpu.group_stem_release(g, vsid)
        got = run(text)
        for (t, c), (_, wc) in zip(got, plain):
            assert t[0] == vsid and t[1] > 20 and np.array_equal(c, wc)
        gpu.group_voice_set_stem(g, vid.value, None)
        with pytest.raises(gpu.Q3Error, match="unknown stem"):
            gpu.group_set_stem(g, vsid)
    finally:
        L.q3tts_group_destroy(g)


# -------------------------------------------------------------- full size --------------------------------------------------------------
def test_fullsize_8_requests_behind_a_300_row_stem_beside_8_plain_ones(gpu, vivian):
    model = synth_models.full("q8_0")
    ge = gpu.Engine(model, "q8_0", max_batch=16, max_steps=8, max_prompt=384, load_codec=False)
    head = _rows(ge, vivian, 400, 300)
    stemmed = [(np.concatenate([head, _rows(ge, vivian, 401 + i, 20 + 2 * i)]), 600 + i) for i in range(8)]
    plain = [(_rows(ge, vivian, 421 + i, 30 + 40 * i), 700 + i) for i in range(8)]
    sid = _ready(ge, gpu, head)
    assert ge.stem_stats()["device_bytes"] == 2 * 5 * 28 * 8 * 8192 * 2
    ge.set_stem(sid)
    rids = []
    for i in range(8):                                                    # interleaved in the queue
        rids.append(ge.submit(stemmed[i][0], max_steps=6, seed=stemmed[i][1], mask_eos=True, **SAMPLED))
        rids.append(ge.submit(plain[i][0], max_steps=6, seed=plain[i][1], mask_eos=True, **SAMPLED))
    ge.set_stem(None)
    assert [ge.request_stem(r) for r in rids] == [(sid, 300), (-1, 0)] * 8
    _drain(ge)
    st = ge.stem_stats()
    assert (st["restores"], st["rows_not_prefilled"], st["pages_copied"], st["mismatches"]) == (8, 2400, 40, 8)
    got = [ge.result(r)["codes"] for r in rids]
    ge.close()
    ref = gpu.Engine(model, "q8_0", max_batch=2, max_steps=8, max_prompt=384, load_codec=False)
    todo = [x for pair in zip(stemmed, plain) for x in pair]
    for i in range(0, 16, 2):                                             # the same requests, plain, two at a time
        pair = [ref.submit(p, max_steps=6, seed=s, mask_eos=True, **SAMPLED) for p, s in todo[i:i + 2]]
        for j, r in enumerate(pair):
            assert ref.wait(r, WAIT_MS)
            wc = ref.result(r)["codes"]
            assert wc.shape == (6, 16) and np.array_equal(got[i + j], wc), i + j
    ref.close()
