"""The assembled codec decoder on the GPU against the whole decoder in float64 (tests/codec_f64_ref.py), frame by frame, and the isolation
of the streams of one group pass, bit for bit.  (-m gpu)

Error measure, the same in every case: for the same codes E_gpu[f] / M_gpu[f] are the RMS / the largest absolute value of (GPU - float64)
over frame f (1920 samples), E_orc / M_orc the same for the C oracle, and every frame of every stream checked has to keep

    E_gpu[f] <= K_RMS * max_f E_orc        M_gpu[f] <= K_MAX * max_f M_orc

K_RMS and K_MAX (tests/codec_f64_ref.py) are twice the worst ratio measured on the MI355X over all cases of this file, rounded up, and
neither may pass 16 (profiles/codec_pcm_f64.md has the measured ratios).  The oracle's floor is computed once per codec: on the tiny codec
from the 24 frames of the single-stream case (the run test_codec_f64_ref_cpu.py pins), on the full-size codec from the 8 frames of stream 0
of the group case.  Every case is native 24 kHz float32 at rate 100.

Isolation needs no reference: one group pass mixes the rows of up to 16 streams in the same GEMM tiles, and the decoder is deterministic,
so when stream j's codes change every other stream's samples must keep their bits."""
import collections
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import codec_f64_ref as R
import synth_models
from test_gpu_codec_ops import _staggered

pytestmark = pytest.mark.gpu
SPF = R.SPF
WAIT_MS = 60000.0
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
Floor = collections.namedtuple("Floor", "E M")      # the oracle's worst frame RMS and worst sample against float64


def _f64(path, codes, prime=None):
    t0 = time.time()
    out = R.torch_codec(path, codes, torch.float64, prime=prime)
    n = sum(len(c) for c in codes) if isinstance(codes, list) else len(codes)
    print("float64 reference: %d frames in %.2f s" % (n, time.time() - t0))
    return out


def _oracle_floor(oracle, path, codes, ref):
    c = oracle.Codec(path)
    c.reset()
    t0 = time.time()
    E, M = R.frame_errors(c.decode(codes).copy(), ref)
    c.close()
    print("oracle against float64 (%d frames, %.2f s): frame rms up to %.3g, sample up to %.3g" % (len(codes), time.time() - t0, E.max(), M.max()))
    return Floor(float(E.max()), float(M.max()))


def _hold(case, floor, items):
    """items: (name, got, ref) per stream; every frame of every item is held to the bounds, after the worst ratios are printed"""
    bad, we, wm, ae, am, frames = [], 0.0, 0.0, 0.0, 0.0, 0
    for name, got, ref in items:
        assert np.isfinite(got).all(), "%s, %s: non-finite samples" % (case, name)
        E, M = R.frame_errors(got, ref)
        frames += E.size
        we, wm, ae, am = max(we, E.max() / floor.E), max(wm, M.max() / floor.M), max(ae, E.max()), max(am, M.max())
        for f in np.flatnonzero((E > R.K_RMS * floor.E) | (M > R.K_MAX * floor.M)):
            bad.append("%s frame %d: rms %.3g (%.1f x floor), max %.3g (%.1f x floor)" % (name, f, E[f], E[f] / floor.E, M[f], M[f] / floor.M))
    print("RATIOS %s: %d streams, %d frames: worst frame rms %.3g = %.2f x floor, worst sample %.3g = %.2f x floor"
          % (case, len(items), frames, ae, we, am, wm))
    assert not bad, "%s: %d frames over K_RMS = %s / K_MAX = %s: %s" % (case, len(bad), R.K_RMS, R.K_MAX, "; ".join(bad[:6]))


def _run_group(gpu, path, n_streams, max_group, joins, n_chunks, T, codes):
    """a fresh decoder; stream i (slot (5 i + 3) % n_streams) joins the group at chunk joins[i] and decodes T-frame chunks of codes[i] until
    n_chunks, all live streams in one pass per chunk.  Returns [stream][chunk] PCM"""
    slots = [(5 * i + 3) % n_streams for i in range(len(joins))]
    assert len(set(slots)) == len(joins)
    gd = gpu.Decoder(path, n_streams=n_streams, max_frames=4, max_group=max_group)
    try:
        pcm = [[] for _ in joins]
        for c in range(n_chunks):
            live = [i for i in range(len(joins)) if joins[i] <= c]
            for i in live:
                if joins[i] == c:
                    gd.reset(slots[i])
            batch = np.stack([codes[i][(c - joins[i]) * T: (c - joins[i] + 1) * T] for i in live])
            wav = gd.decode_group([slots[i] for i in live], batch)
            assert wav.shape == (len(live), T * SPF)
            for k, i in enumerate(live):
                pcm[i].append(wav[k].copy())
    finally:
        gd.close()
    return pcm


def _codes_for(seed, joins, n_chunks, T):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 2048, ((n_chunks - j) * T, 16)) for j in joins]


@pytest.fixture(scope="module")
def tiny_path(tiny_model):
    return os.path.join(tiny_model, "onnx", "q3tts_codec.gguf")


@pytest.fixture(scope="module")
def full_path(synth_tool):
    return os.path.join(synth_models.full("q8_0"), "onnx", "q3tts_codec.gguf")


@pytest.fixture(scope="module")
def single(tiny_path, oracle):
    """the single-stream case's codes, their float64 PCM, and the tiny codec's oracle floor from the same 24 frames"""
    codes = np.random.default_rng(7).integers(0, 2048, (24, 16))
    ref = _f64(tiny_path, codes)
    ref.setflags(write=False)
    return codes, ref, _oracle_floor(oracle, tiny_path, codes, ref)


@pytest.fixture(scope="module")
def tiny_floor(single):
    return single[2]


# ------------------------------------------------ against float64, frame by frame ------------------------------------------------
SCHEDULES = ([1] * 24, [4] * 6, [3, 4, 1, 4, 4, 4, 4])


def test_single_stream_every_chunk_schedule(gpu, tiny_path, single):
    """tiny codec (window 8: the cache saturates at 7): frame 0 with an empty history, the saturation frame and every chunk boundary of three
    schedules; the schedules also agree with each other within the same bounds"""
    codes, ref, floor = single
    gd = gpu.Decoder(tiny_path, 2, max_frames=4)
    got = []
    for s, sched in enumerate(SCHEDULES):
        assert sum(sched) == 24
        stream = s % 2
        gd.reset(stream)
        parts, o = [], 0
        for n in sched:
            parts.append(gd.decode(codes[o:o + n], False, stream).copy())
            o += n
        got.append(np.concatenate(parts))
    gd.close()
    _hold("single stream, tiny", floor, [("schedule %s" % (s,), g, ref) for s, g in zip(SCHEDULES, got)])
    _hold("single stream, tiny, schedule against schedule", floor,
          [("%s against %s" % (SCHEDULES[a], SCHEDULES[b]), got[a], got[b]) for a, b in ((0, 1), (0, 2), (1, 2))])


@pytest.mark.parametrize("rest", (0, 7), ids=lambda r: "rest_join_at_%d" % r)
def test_group_of_16_staggered_joins(gpu, tiny_path, tiny_floor, rest):
    """tiny codec, 17 stream slots, a group of up to 16: streams join at chunks 0, 0, 1, 3 and 6 and the other eleven at chunk `rest`,
    ten 4-frame chunks.  With the rest at chunk 0 every pass is wide (52 to 64 rows, the split-f16 forms); with the rest at chunk 7 the
    early passes hold 2 to 5 streams (8 to 20 rows, the narrow forms) with mixed cache lengths before the group fills up.  Every stream,
    every frame"""
    joins = [0, 0, 1, 3, 6] + [rest] * 11
    codes = _codes_for(31 + rest, joins, 10, 4)
    pcm = _run_group(gpu, tiny_path, 17, 16, joins, 10, 4, codes)
    ref = _f64(tiny_path, codes)
    _hold("group of 16, tiny, the rest joins at chunk %d" % rest, tiny_floor,
          [("stream %d (joined at chunk %d)" % (i, joins[i]), np.concatenate(pcm[i]), ref[i]) for i in range(16)])


def test_group_of_5_one_frame_at_a_time(gpu, tiny_path, tiny_floor):
    """T = 1, the skinny forms: five streams, twelve 1-frame chunks, joined at chunks 0, 0, 2, 5 and 9 so the passes mix cache lengths"""
    joins = [0, 0, 2, 5, 9]
    codes = _codes_for(53, joins, 12, 1)
    pcm = _run_group(gpu, tiny_path, 8, 5, joins, 12, 1, codes)
    ref = _f64(tiny_path, codes)
    _hold("group of 5, T = 1, tiny", tiny_floor, [("stream %d (joined at chunk %d)" % (i, joins[i]), np.concatenate(pcm[i]), ref[i]) for i in range(5)])


@pytest.fixture(scope="module")
def full_group(gpu, full_path, oracle):
    """the 16-stream pass of test_fullsize_codec_group16_vs_oracle: codes, PCM, and the full-size oracle floor from stream 0's 8 frames"""
    codes = list(np.random.default_rng(21).integers(0, 2048, (16, 8, 16)))
    pcm = _run_group(gpu, full_path, 17, 16, [0] * 16, 2, 4, codes)
    held = (0, 5, 10, 15)
    ref = dict(zip(held, _f64(full_path, [codes[i] for i in held])))
    return codes, pcm, ref, _oracle_floor(oracle, full_path, codes[0], ref[0])


def test_fullsize_group_of_16(full_group):
    """full-size codec, 16 streams, two 4-frame chunks; streams 0, 5, 10 and 15 against float64 (one batched torch pass), the other twelve
    are covered by the isolation cases"""
    codes, pcm, ref, floor = full_group
    _hold("group of 16, full size", floor, [("stream %d" % i, np.concatenate(pcm[i]), ref[i]) for i in sorted(ref)])


def test_fullsize_staggered_joins_past_the_window(gpu, oracle, full_path, full_group):
    """the full-size case of test_gpu_codec_ops.py (4 streams join at chunks 0, 1, 2 and 5 and decode 20 chunks, past window 72) through
    its own helper; its first and last stream against float64 per frame"""
    codes, pcm = _staggered(gpu, oracle, full_path, 7, 4, [0, 1, 2, 5], 20, (), 41)
    ref = _f64(full_path, [codes[0], codes[3]])
    _hold("staggered joins, full size", full_group[3], [("stream 0 (80 frames)", pcm[0], ref[0]), ("stream 3 (60 frames)", pcm[3], ref[1])])


# ------------------------------------------------ through the engine ------------------------------------------------
N_REQ = 33
MS = [5 + (i + 7) % 8 for i in range(N_REQ)]        # 12, 5, 6, .. ragged: streams end on partial chunks (9 = 4 + 4 + 1); slot 32 runs 12
PRIMED, RESUMED, CHANGED, K_PREFIX = 3, 20, 16, 3


def _until(ge, cond, limit=4000):
    for _ in range(limit):
        if cond():
            return
        ge.sched_step()
    raise AssertionError("condition not reached")


def _batch(ge, gpu, prompts, pid, prefix, seed16):
    """the 33 requests: even ones sampled, odd ones greedy; PRIMED behind the 8-frame preamble, RESUMED handed its first K_PREFIX frames"""
    rids = []
    for i in range(N_REQ):
        kw = dict(SAMPLED) if i % 2 == 0 else {}
        if i == RESUMED:
            kw["prefix_codes"] = prefix
        if i == PRIMED:
            ge.set_preamble(pid)
        rids.append(ge.submit(prompts[i], max_steps=MS[i], seed=seed16 if i == CHANGED else 100 + i, mask_eos=True, want_pcm=True, **kw))
        if i == PRIMED:
            ge.set_preamble(None)
    assert [ge.request_preamble(r) for r in rids] == [pid if i == PRIMED else -1 for i in range(N_REQ)]
    _until(ge, lambda: all(ge.poll(r)["state"] == gpu.REQ_DONE for r in rids))
    out = [ge.result(r, want_pcm=True) for r in rids]
    for i, r in enumerate(out):
        assert r["codes"].shape == (MS[i], 16) and r["pcm"].dtype == np.float32 and r["pcm"].size == MS[i] * SPF, i
    return out


@pytest.fixture(scope="module")
def engine_runs(gpu, tiny_model, vivian):
    """tiny model, 33 slots with the codec on (three codec groups over the lanes, a width that is no power of two): the batch twice, the
    second time with request 16's seed changed"""
    assert 9 in MS and min(MS) == 5 and max(MS) == 12 and MS[RESUMED] > K_PREFIX and CHANGED % 2 == 0
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=N_REQ, max_steps=16, load_codec=True)
    try:
        prompts = []
        for i in range(N_REQ):
            rng = np.random.default_rng(700 + i)
            prompts.append(ge.assets.build_core(rng.integers(0, 4000, 6 + i % 5).astype(np.int32), lang_id=2055, spk_emb=vivian))
        pre = np.random.default_rng(11).integers(0, 2048, (8, 16)).astype(np.int32)
        pid = ge.preamble_create(pre)
        assert ge.preamble_wait(pid, WAIT_MS) and ge.preamble_poll(pid) == (gpu.PREAMBLE_READY, 8)
        rid = ge.submit(prompts[RESUMED], max_steps=MS[RESUMED], seed=100 + RESUMED, mask_eos=True, **SAMPLED)     # the uninterrupted run
        _until(ge, lambda: ge.poll(rid)["state"] == gpu.REQ_DONE)
        whole = ge.result(rid)["codes"]
        ge.reset_stats()
        a = _batch(ge, gpu, prompts, pid, whole[:K_PREFIX], 100 + CHANGED)
        st = ge.stats()
        b = _batch(ge, gpu, prompts, pid, whole[:K_PREFIX], 9999)
    finally:
        ge.close()
    assert np.array_equal(a[RESUMED]["codes"], whole)
    return a, b, pre, st


def test_engine_batch_of_33(engine_runs, tiny_path, tiny_floor):
    """every request's PCM against float64 of its own returned codes, clipped to 0..2047 as the engine clips them; the primed request
    behind its 8 reference frames, the resumed one as the whole utterance"""
    a, _, pre, st = engine_runs
    assert st["slot_frames"] / st["graph_frames"] >= 24, st
    codes = [np.clip(r["codes"], 0, 2047) for r in a]
    ref = _f64(tiny_path, codes, prime=[pre if i == PRIMED else None for i in range(N_REQ)])
    cold = R.torch_codec(tiny_path, codes[PRIMED], torch.float64)
    assert np.sqrt(np.mean((ref[PRIMED][:SPF] - cold[:SPF]) ** 2)) >= 0.05       # the check can tell a primed start from a cold one
    what = lambda i: "request %d (%d frames%s)" % (i, MS[i], ", primed" if i == PRIMED else ", resumed" if i == RESUMED else "")
    _hold("engine, 33 requests, tiny", tiny_floor, [(what(i), a[i]["pcm"], ref[i]) for i in range(N_REQ)])


# ------------------------------------------------ stream isolation, bit for bit ------------------------------------------------
def _differing(a, b):
    """streams whose PCM differs in any bit of any chunk"""
    return [i for i in range(len(a)) if any(not np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a[i], b[i]))]


_base = {}


def _isolation(gpu, path, j, joins, n_chunks):
    """two runs on fresh decoders; the second replaces stream j's codes with other random codes in every chunk"""
    key = (path, tuple(joins))
    codes = _codes_for(61, joins, n_chunks, 4)
    if key not in _base:
        _base[key] = _run_group(gpu, path, 17, 16, joins, n_chunks, 4, codes)
    other = list(codes)
    other[j] = np.random.default_rng(62 + j).integers(0, 2048, codes[j].shape)
    assert (other[j] != codes[j]).any(axis=1).reshape(-1, 4).any(axis=1).all()    # every chunk of stream j changes
    pcm = _run_group(gpu, path, 17, 16, joins, n_chunks, 4, other)
    diff = _differing(_base[key], pcm)
    print("stream %d's codes changed: PCM differs in streams %s" % (j, diff))
    leaked = [i for i in diff if i != j]
    assert not leaked, "stream %d's codes reached the PCM of streams %s" % (j, leaked)
    assert all(not np.array_equal(x, y) for x, y in zip(_base[key][j], pcm[j])), "stream %d's own PCM did not change in every chunk" % j


@pytest.mark.parametrize("j", (0, 7, 15))
def test_isolation_group_of_16(gpu, tiny_path, j):
    _isolation(gpu, tiny_path, j, [0] * 16, 3)


@pytest.mark.parametrize("j", (0, 7, 15))
def test_isolation_group_of_16_fullsize(gpu, full_path, j):
    _isolation(gpu, full_path, j, [0] * 16, 3)


@pytest.mark.parametrize("j", (0, 7, 15))
def test_isolation_staggered_histories(gpu, tiny_path, j):
    """stream j joined two chunks before the other fifteen: its history is 8 frames deep (saturated) when theirs are empty"""
    _isolation(gpu, tiny_path, j, [0 if i == j else 2 for i in range(16)], 5)


def test_isolation_through_the_engine(engine_runs):
    """the 33-request batch again with request 16's seed changed: its codes change, nobody else's do, and every other PCM keeps its bits"""
    a, b, _, _ = engine_runs
    assert not np.array_equal(a[CHANGED]["codes"], b[CHANGED]["codes"]) and not np.array_equal(a[CHANGED]["pcm"], b[CHANGED]["pcm"])
    moved = [i for i in range(N_REQ) if i != CHANGED and not np.array_equal(a[i]["codes"], b[i]["codes"])]
    assert not moved, "codes of requests %s changed with request %d's seed" % (moved, CHANGED)
    leaked = [i for i in range(N_REQ) if i != CHANGED and not np.array_equal(a[i]["pcm"].view(np.uint32), b[i]["pcm"].view(np.uint32))]
    print("request %d's seed changed: PCM differs in requests %s" % (CHANGED, [CHANGED] + leaked))
    assert not leaked, "request %d's codes reached the PCM of requests %s" % (CHANGED, leaked)
