"""[EXT] pitch on the GPU: k_tsm_pitch through q3tts_op_pitch, one launch of the engine's launcher per chunk, against the float64 reference
of tests/pitch_ref.py.  Stage 1's decisions are judged with the kernel's own previous offset (teacher-forced), as the speaking rate's are, and
cross-checked entry for entry against the merged kernel where the tempo is an integer percent.  The delivered samples are judged given the
kernel's trace under the derived bound sum |h32| bz + gamma(K + 1) sum |h32 z64| + 2^-149.  Every output, every trace and both state stores
come back whole and are checked to the last guard element."""
import functools

import numpy as np
import pytest

import pitch_ref as R
import tsm_ref as T

pytestmark = pytest.mark.gpu

FRAME, FILL = 1920, 0x5A
F32, S16 = 0, 1
SCHEDS = ((9,), (4, 4, 1), (1,) * 9, (1, 4, 3, 1))
GUARD = np.float32(-3e38)


def run(gpu, x, sched, rates, pitches, encs=None, slots=None, n_streams=None, flush=False, counts=None, **kw):
    """one q3tts_op_pitch; checks what every case must hold: counts (of an utterance that starts with the call, unless `counts` gives them),
    guards, the unwritten slack"""
    G = len(rates)
    encs = [F32] * G if encs is None else encs
    slots = np.tile(np.arange(G, dtype=np.int32), (len(sched), 1)) if slots is None else np.asarray(slots, np.int32)
    n_streams = G if n_streams is None else n_streams
    outs, traces, wholes, twholes, n_out, hist, zhist = gpu.op_pitch(x, [f * FRAME for f in sched], slots, n_streams, rates, pitches, encs,
                                                                     flush=flush, slack=8, fill=FILL, **kw)
    n_native = sum(sched) * FRAME
    for g, (o, t, w, tw, n) in enumerate(zip(outs, traces, wholes, twholes, n_out)):
        if counts is not None:
            want = counts[g]
        elif pitches[g] != 100:
            want = gpu.pitch_samples(rates[g], pitches[g], n_native, flush)
            assert want == R.n_samples(rates[g], pitches[g], n_native, flush) and t.size == R.n_frames(rates[g], pitches[g], n_native, flush)
        else:
            want = n_native if rates[g] == 100 else gpu.tsm_samples(rates[g], n_native, flush)
        assert n == o.size == want, (g, n, o.size, want)
        assert o.dtype == (np.int16 if encs[g] == S16 and (rates[g] != 100 or pitches[g] != 100) else np.float32)
        assert np.all(np.abs(t) <= R.SEARCH)
        gb = gpu.GLUE_GUARD * o.dtype.itemsize
        assert np.all(w[:gb] == FILL) and np.all(w[gb + o.nbytes:] == FILL), "a write outside the stream's output"
        assert np.all(tw[: gpu.GLUE_GUARD] == 0x5A5A5A5A) and np.all(tw[gpu.GLUE_GUARD + t.size:] == 0x5A5A5A5A), "a write outside the stream's trace"
    for h in (hist, zhist):
        assert np.all(h[: gpu.GLUE_GUARD] == GUARD) and np.all(h[-gpu.GLUE_GUARD:] == GUARD), "state store guards"
    return outs, traces, hist, zhist


def check_against_reference(x, Rt, P, out, trace, flush=False, out16=None, cap=True):
    """the teacher-forced decision check and the output bound given the trace; returns the number of undecided frames"""
    res = R.decisions(x, Rt, P, trace, final=flush)
    undecided = 0
    for k, ((ok, decided, ref), dk) in enumerate(zip(res, trace)):
        assert ok, "frame %d: the cost of offset %d is beyond the running-error factor of the least cost" % (k, dk)
        if decided:
            assert dk == ref, "frame %d: offset %d, the reference decides %d" % (k, dk, ref)
        undecided += not decided
    y, bound, _, _ = R.pitch(x, Rt, P, final=flush, deltas=trace)
    assert out.size == y.size
    err = np.abs(out.astype(np.float64) - y)
    print("rate %d pitch %d: %d frames, %d undecided, %d samples, max err %.3g, max err / bound %.3g"
          % (Rt, P, len(trace), undecided, y.size, err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    assert not cap or undecided <= 0.02 * len(trace)
    if out16 is not None:
        assert np.array_equal(out16, R.s16_of(out))
    return undecided


@pytest.mark.parametrize("pair", R.GPU_PAIRS, ids=lambda p: "r%d_p%d" % p)
@pytest.mark.parametrize("kind", ("speech", "noise"))
def test_decisions_and_output_against_float64(gpu, kind, pair):
    x = T.speech_like(12) if kind == "speech" else T.noise(9)
    outs, traces, _, _ = run(gpu, np.stack([x, x]), (x.size // FRAME,), [pair[0]] * 2, [pair[1]] * 2, [F32, S16])
    assert np.array_equal(traces[0], traces[1])
    check_against_reference(x, pair[0], pair[1], outs[0], traces[0], out16=outs[1])


@pytest.mark.parametrize("pair,pct", (((100, 125), 80), ((100, 80), 125), ((100, 50), 200), ((100, 200), 50), ((150, 75), 200)),
                         ids=lambda v: "r%d_p%d" % v if isinstance(v, tuple) else "tempo%d" % v)
def test_trace_equals_the_merged_kernels_at_an_integer_tempo(gpu, pair, pct):
    x = np.stack([T.speech_like(9, 21), T.noise(9, 22)])
    for flush in (False, True):
        _, traces, _, _ = run(gpu, x, SCHEDS[3], [pair[0]] * 2, [pair[1]] * 2, flush=flush)
        _, ttr, _, _, _, _ = gpu.op_tsm(x, [f * FRAME for f in SCHEDS[3]], np.tile(np.arange(2, dtype=np.int32), (4, 1)), 2, [pct] * 2, [F32] * 2, flush=flush)
        for a, b in zip(traces, ttr):
            assert a.size > 0 and np.array_equal(a, b)   # the same arithmetic


@pytest.mark.parametrize("P", (50, 89, 107, 200))
def test_a_tone_moves_to_the_shifted_frequency(gpu, P):
    x = (0.5 * np.sin(2 * np.pi * 300.0 * np.arange(9 * FRAME) / 24000.0)).astype(np.float32)
    outs, _, _, _ = run(gpu, x[None, :], SCHEDS[1], [100], [P], flush=True)
    assert outs[0].size == gpu.pitch_samples(100, P, x.size, True)
    f, margin = R.crossings_hz(outs[0])
    print("pitch %d: %.3f Hz, wanted %.1f, margin %.3f" % (P, f, 300.0 * P / 100.0, margin))
    assert abs(f - 300.0 * P / 100.0) <= margin


@pytest.mark.parametrize("pair", ((100, 107), (125, 80), (100, 50), (100, 200)), ids=lambda p: "r%d_p%d" % p)
def test_periodic_tables_are_resampled_in_phase(gpu, pair):
    Rt, P = pair
    periods = (96, 75, 201)
    tabs, xs = zip(*[T.periodic(p, 6, 11 + p) for p in periods])
    outs, traces, _, _ = run(gpu, np.stack(xs), (6,), [Rt] * 3, [P] * 3)
    L, M, _, _ = R.plan(P)
    skip = max(64, -(-R.ZHIST * L // M) + 1)                      # behind these no tap reaches below z[0]
    for per, tab, x, o, t in zip(periods, tabs, xs, outs, traces):
        z, d, _ = R.stretch(x, Rt, P)
        assert np.array_equal(t, d), (per, t, d)                  # every cost is exactly 0 or not: the tie rule alone decides
        zp = tab[np.arange(z.size) % per].astype(np.float64)      # the table continued in phase
        bz = 2.0 ** -23 * np.abs(zp) + 2.0 ** -149
        y, bound = R.resample(zp, P, bz, before=lambda m: tab[m % per].astype(np.float64))
        assert o.size == y.size > 4 * skip
        err = np.abs(o.astype(np.float64) - y)[skip:]
        print("period %d: max err / bound %.3g" % (per, (err / bound[skip:]).max()))
        assert np.all(err <= bound[skip:]), per


@functools.lru_cache(maxsize=None)
def sched_signals():
    x = np.stack([T.speech_like(9, 21), T.noise(9, 22), T.periodic(75, 9, 23)[1]])
    x.setflags(write=False)
    return x


SCHED_RATES, SCHED_PITCHES, SCHED_ENCS = [100, 125, 90], [107, 80, 120], [F32, S16, F32]


@functools.lru_cache(maxsize=None)
def whole_run(gpu_mod, flush):
    return run(gpu_mod, sched_signals(), SCHEDS[0], SCHED_RATES, SCHED_PITCHES, SCHED_ENCS, flush=flush)


@pytest.mark.parametrize("flush", (False, True), ids=("streaming", "flushed"))
def test_chunk_schedule_does_not_matter(gpu, flush):
    want, wtr, whist, wz = whole_run(gpu, flush)
    for sched in SCHEDS[1:]:
        outs, traces, hist, zhist = run(gpu, sched_signals(), sched, SCHED_RATES, SCHED_PITCHES, SCHED_ENCS, flush=flush)
        for g in range(3):
            assert np.array_equal(outs[g].view(np.uint8), want[g].view(np.uint8)), (sched, g)
            assert np.array_equal(traces[g], wtr[g]), (sched, g)
        assert np.array_equal(hist.view(np.uint32), whist.view(np.uint32)) and np.array_equal(zhist.view(np.uint32), wz.view(np.uint32))
        core = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, R.HIST)
        assert np.array_equal(core.view(np.uint32), sched_signals()[:, -R.HIST:].view(np.uint32))   # the last 1920 native samples
    # the intermediate history is the last 64 samples of z: within stage 1's bound of the float64 one
    zc = wz[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, R.ZHIST)
    for g in range(3):
        z, _, bz = R.stretch(sched_signals()[g], SCHED_RATES[g], SCHED_PITCHES[g], final=flush, deltas=wtr[g])
        assert np.all(np.abs(zc[g].astype(np.float64) - z[-R.ZHIST:]) <= bz[-R.ZHIST:])


def test_flushed_stream_continues_the_streamed_one(gpu):
    outs, traces, _, _ = whole_run(gpu, True)
    streamed, str_tr, _, _ = whole_run(gpu, False)
    for g, (Rt, P, enc) in enumerate(zip(SCHED_RATES, SCHED_PITCHES, SCHED_ENCS)):
        x = sched_signals()[g]
        L, M, _, _ = R.plan(P)
        nz = 480 * -(-P * x.size // (480 * Rt))
        assert outs[g].size == gpu.pitch_samples(Rt, P, x.size, True) == -(-nz * L // M) > streamed[g].size
        assert np.array_equal(outs[g][: streamed[g].size], streamed[g]) and np.array_equal(traces[g][: str_tr[g].size], str_tr[g])
        if enc == F32:
            check_against_reference(x, Rt, P, outs[g], traces[g], flush=True, cap=g != 2)
        else:
            y, bound, _, _ = R.pitch(x, Rt, P, final=True, deltas=traces[g])
            assert np.all(np.abs(outs[g].astype(np.float64) - y * 32767.0) <= 0.5 + bound * 32767.0)


def test_slots_of_a_larger_store_permuted_between_chunks(gpu):
    sched = SCHEDS[3]
    slots = np.array([[5, 0, 2], [2, 5, 0], [0, 2, 5], [5, 2, 0]], np.int32)   # the slot of each position, per chunk
    sig_of = {5: 0, 0: 1, 2: 2}                                                # which signal lives in which slot
    edges = np.cumsum((0,) + sched) * FRAME
    for Rt, P, enc in ((100, 107, F32), (125, 80, S16)):
        x = np.empty_like(sched_signals())
        for c in range(len(sched)):
            for p in range(3):
                x[p, edges[c]: edges[c + 1]] = sched_signals()[sig_of[slots[c, p]], edges[c]: edges[c + 1]]
        rng = np.random.default_rng(3)
        stores = []
        for width in (R.HIST, R.ZHIST):                                        # somebody else's histories in the other slots
            st = np.zeros((6, width), np.float32)
            st[[1, 3, 4]] = rng.uniform(-1, 1, (3, width)).astype(np.float32)
            stores.append(st)
        guarded = [np.concatenate([np.full(gpu.GLUE_GUARD, GUARD, np.float32), st.reshape(-1), np.full(gpu.GLUE_GUARD, GUARD, np.float32)]) for st in stores]
        ref, rtr, rhist, rz = run(gpu, sched_signals(), sched, [Rt] * 3, [P] * 3, [enc] * 3)
        outs, traces, hist, zhist = run(gpu, x, sched, [Rt] * 3, [P] * 3, [enc] * 3, slots=slots, n_streams=6, hist=guarded[0], zhist=guarded[1])
        oe = [gpu.pitch_samples(Rt, P, int(e), False) for e in edges]
        fe = [gpu.pitch_frames(Rt, P, int(e), False) for e in edges]
        for c in range(len(sched)):
            for p in range(3):
                s = sig_of[slots[c, p]]
                assert np.array_equal(outs[p][oe[c]: oe[c + 1]], ref[s][oe[c]: oe[c + 1]]), (P, c, p)
                assert np.array_equal(traces[p][fe[c]: fe[c + 1]], rtr[s][fe[c]: fe[c + 1]]), (P, c, p)
        for after, st, alone, width in ((hist, stores[0], rhist, R.HIST), (zhist, stores[1], rz, R.ZHIST)):
            after = after[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(6, width)
            alone = alone[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, width)
            assert np.array_equal(after[[1, 3, 4]].view(np.uint32), st[[1, 3, 4]].view(np.uint32))
            for slot, g in sig_of.items():
                assert np.array_equal(after[slot].view(np.uint32), alone[g].view(np.uint32))


def test_reset_starts_a_new_utterance_and_leaves_the_others(gpu):
    sched = SCHEDS[3]
    want, wtr, whist, wz = whole_run(gpu, False)
    reset = np.zeros((len(sched), 3), np.int32)
    reset[2, 1] = 1                                              # stream 1, ahead of the third chunk (frame 5)
    cut = 5 * FRAME
    n = lambda g, N: gpu.pitch_samples(SCHED_RATES[g], SCHED_PITCHES[g], N, False)
    counts = [n(0, 9 * FRAME), n(1, cut) + n(1, 4 * FRAME), n(2, 9 * FRAME)]
    outs, traces, hist, zhist = run(gpu, sched_signals(), sched, SCHED_RATES, SCHED_PITCHES, SCHED_ENCS, reset_before=reset, counts=counts)
    for g in (0, 2):
        assert np.array_equal(outs[g], want[g]) and np.array_equal(traces[g], wtr[g])
    for a, b, width in ((hist, whist, R.HIST), (zhist, wz, R.ZHIST)):   # the other slots' 1920 + 64 history entries: bit-identical
        a, b = a[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, width), b[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, width)
        assert np.array_equal(a[[0, 2]].view(np.uint32), b[[0, 2]].view(np.uint32))
    ocut, fcut = n(1, cut), gpu.pitch_frames(SCHED_RATES[1], SCHED_PITCHES[1], cut, False)
    assert np.array_equal(outs[1][:ocut], want[1][:ocut])
    fresh, ftr, _, _ = run(gpu, sched_signals()[:, cut:], (3, 1), SCHED_RATES, SCHED_PITCHES, SCHED_ENCS)
    assert np.array_equal(outs[1][ocut:], fresh[1]) and np.array_equal(traces[1][fcut:], ftr[1])
    assert ftr[1][0] == 0                                        # frame 0 of an utterance: the template is the candidate at offset 0
    assert not np.array_equal(outs[1][ocut: ocut + 480], want[1][ocut: ocut + 480])   # and that differs from the stream that went on


def test_pitch_rate_only_and_native_streams_in_one_launch(gpu):
    x = sched_signals()
    rates, pitches, encs = [100, 125, 100], [107, 100, 100], [S16, S16, F32]
    outs, traces, hist, zhist = run(gpu, x, SCHEDS[3], rates, pitches, encs, flush=True)
    assert np.array_equal(outs[2].view(np.uint32), x[2].view(np.uint32)) and traces[2].size == 0   # the native stream: the input bits
    touts, ttr, _, _, _, thist = gpu.op_tsm(x[1:2], [f * FRAME for f in SCHEDS[3]], np.zeros((4, 1), np.int32), 1, [125], [S16], flush=True)
    assert outs[1].dtype == np.int16 and np.array_equal(outs[1], touts[0]) and np.array_equal(traces[1], ttr[0])   # the merged kernel's bytes
    alone, atr, _, az = run(gpu, x[0:1], SCHEDS[0], [100], [107], [S16], flush=True)
    assert np.array_equal(outs[0], alone[0]) and np.array_equal(traces[0], atr[0])
    zc = zhist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, R.ZHIST)
    assert not zc[1].any() and not zc[2].any()                   # only a stream with a pitch keeps intermediate history
    assert np.array_equal(zc[0], az[gpu.GLUE_GUARD: -gpu.GLUE_GUARD])
    core = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, R.HIST)
    assert not core[2].any() and np.array_equal(core[1], thist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD])


def test_silence_chooses_offset_zero_and_delivers_zeros(gpu):
    x = np.stack([np.zeros(3 * FRAME, np.float32), T.speech_like(3, 5)])
    outs, traces, _, _ = run(gpu, x, (1, 2), [100, 100], [107, 107], flush=True)
    assert traces[0].size > 0 and not outs[0].any() and not traces[0].any()
    assert outs[1].any()


@pytest.mark.parametrize("what", ["chunk length", "zero chunk", "no stream", "stream twice", "stream out of range", "pitch 49", "pitch 201",
                                  "rate 201", "pair", "encoding"])
def test_launcher_refusals_write_nothing(gpu, what):
    x, rates, pitches, encs, slots, chunks = sched_signals()[:, : 2 * FRAME], [100, 125, 150], [107, 80, 75], [F32, S16, F32], [[0, 1, 2]], [2 * FRAME]
    if what == "chunk length":
        chunks = [2 * FRAME - 920]
    elif what == "zero chunk":
        chunks, x = [0], x[:, :0]
    elif what == "no stream":
        x, rates, pitches, encs, slots = x[:0], [], [], [], [[]]
    elif what == "stream twice":
        slots = [[0, 1, 0]]
    elif what == "stream out of range":
        slots = [[0, 1, 3]]
    elif what == "pitch 49":
        pitches = [107, 49, 75]
    elif what == "pitch 201":
        pitches = [201, 80, 75]
    elif what == "rate 201":
        rates = [100, 201, 150]
    elif what == "pair":
        rates = [100, 125, 151]
    else:
        encs = [F32, 2, F32]
    with pytest.raises(gpu.Q3Error) as ei:
        gpu.op_pitch(x, chunks, slots, 3, rates, pitches, encs, flush=True, slack=8, fill=FILL)
    ex = ei.value
    assert "tsm pitch" in str(ex) and len(ex.wholes) == len(rates)
    assert all(np.all(w == FILL) for w in ex.wholes) and all(np.all(t == 0x5A5A5A5A) for t in ex.twholes) and np.all(ex.n_out == -1)
    for h in (ex.hist, ex.zhist):
        assert not h[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].any() and np.all(h[: gpu.GLUE_GUARD] == GUARD) and np.all(h[-gpu.GLUE_GUARD:] == GUARD)
