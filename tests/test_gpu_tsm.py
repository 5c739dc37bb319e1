"""[EXT] speaking rate on the GPU: k_tsm_stretch through q3tts_op_tsm, one launch of the engine's launcher per chunk, against the float64
reference of tests/tsm_ref.py.  A decision is judged with the kernel's own previous offset (teacher-forced): its float64 cost must lie
within the running-error factor of the least one, and where the float64 costs leave no doubt it must be the reference's.  The output is
judged given the kernel's trace: one product rounding and one fma rounding.  Every output, every trace and the history store come back whole
and are checked to the last guard element."""
import functools

import numpy as np
import pytest

import tsm_ref as R

pytestmark = pytest.mark.gpu

FRAME, FILL = 1920, 0x5A
F32, S16 = 0, 1
SCHEDS = ((9,), (4, 4, 1), (1,) * 9, (1, 4, 3, 1))


def run(gpu, x, sched, rates, encs=None, slots=None, n_streams=None, flush=False, counts=None, **kw):
    """one q3tts_op_tsm; checks what every case must hold: counts (of an utterance that starts with the call, unless `counts` gives them),
    guards, the unwritten slack"""
    G = len(rates)
    encs = [F32] * G if encs is None else encs
    slots = np.tile(np.arange(G, dtype=np.int32), (len(sched), 1)) if slots is None else np.asarray(slots, np.int32)
    n_streams = G if n_streams is None else n_streams
    outs, traces, wholes, twholes, n_out, hist = gpu.op_tsm(x, [f * FRAME for f in sched], slots, n_streams, rates, encs, flush=flush, slack=8,
                                                            fill=FILL, **kw)
    n_native = sum(sched) * FRAME
    for g, (o, t, w, tw, n) in enumerate(zip(outs, traces, wholes, twholes, n_out)):
        want = n_native if rates[g] == 100 else (gpu.tsm_samples(rates[g], n_native, flush) if counts is None else counts[g])
        assert n == o.size == want, (g, n, o.size, want)
        assert o.dtype == (np.int16 if encs[g] == S16 and rates[g] != 100 else np.float32)
        if rates[g] != 100:
            assert want == R.n_samples(rates[g], n_native, flush) or counts is not None
            assert t.size * R.HOP == o.size and np.all(np.abs(t) <= R.SEARCH)
        gb = gpu.GLUE_GUARD * o.dtype.itemsize
        assert np.all(w[:gb] == FILL) and np.all(w[gb + o.nbytes:] == FILL), "a write outside the stream's output"
        assert np.all(tw[: gpu.GLUE_GUARD] == 0x5A5A5A5A) and np.all(tw[gpu.GLUE_GUARD + t.size:] == 0x5A5A5A5A), "a write outside the stream's trace"
    assert np.all(hist[: gpu.GLUE_GUARD] == np.float32(-3e38)) and np.all(hist[-gpu.GLUE_GUARD:] == np.float32(-3e38)), "history guards"
    return outs, traces, hist


def check_against_reference(x, pct, out, trace, flush=False, out16=None, cap=True):
    """the teacher-forced decision check and the output bound given the trace; returns the number of undecided frames.  cap=False for a
    periodic input, where equal candidates cost exactly the same and every frame is a tie by construction"""
    res = R.decisions(x, pct, trace, final=flush)
    undecided = 0
    for k, ((ok, decided, ref), dk) in enumerate(zip(res, trace)):
        assert ok, "frame %d: the cost of offset %d is beyond the running-error factor of the least cost" % (k, dk)
        if decided:
            assert dk == ref, "frame %d: offset %d, the reference decides %d" % (k, dk, ref)
        undecided += not decided
    y, _, bound = R.stretch(x, pct, final=flush, deltas=trace)
    err = np.abs(out.astype(np.float64) - y)
    print("pct %d: %d frames, %d undecided, max err %.3g, max err/bound %.3g" % (pct, len(trace), undecided, err.max(), (err / bound).max()))
    assert np.all(err <= bound)
    assert not cap or undecided <= 0.02 * len(trace)
    if out16 is not None:
        assert np.array_equal(out16, R.s16_of(out))
    return undecided


@pytest.mark.parametrize("pct", (50, 75, 125, 150, 200))
def test_periodic_tables_continue_in_phase(gpu, pct):
    Ps = (96, 75, 201)
    tabs, xs = zip(*[R.periodic(P, 6, 11 + P) for P in Ps])
    outs, traces, _ = run(gpu, np.stack(xs), (6,), [pct] * 3)
    for P, tab, x, o, t in zip(Ps, tabs, xs, outs, traces):
        y, d, _ = R.stretch(x, pct)
        assert np.array_equal(t, d), (P, t, d)                      # every cost is exactly 0 or not: the tie rule alone decides
        want = tab[np.arange(o.size) % P].astype(np.float64)
        assert np.all(np.abs(o.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want) + 2.0 ** -149), P


@pytest.mark.parametrize("pct", (50, 80, 125, 160, 200))
@pytest.mark.parametrize("kind", ("speech", "noise"))
def test_decisions_and_output_against_float64(gpu, kind, pct):
    x = R.speech_like(12) if kind == "speech" else R.noise(9)
    outs, traces, _ = run(gpu, np.stack([x, x]), (x.size // FRAME,), [pct, pct], [F32, S16])
    assert np.array_equal(traces[0], traces[1])
    check_against_reference(x, pct, outs[0], traces[0], out16=outs[1])


@functools.lru_cache(maxsize=None)
def sched_signals():
    x = np.stack([R.speech_like(9, 21), R.noise(9, 22), R.periodic(75, 9, 23)[1]])
    x.setflags(write=False)
    return x


SCHED_RATES, SCHED_ENCS = [50, 125, 200], [F32, S16, F32]


@functools.lru_cache(maxsize=None)
def whole_run(gpu_mod, flush):
    outs, traces, hist = run(gpu_mod, sched_signals(), SCHEDS[0], SCHED_RATES, SCHED_ENCS, flush=flush)
    return outs, traces, hist


@pytest.mark.parametrize("flush", (False, True), ids=("streaming", "flushed"))
def test_chunk_schedule_does_not_matter(gpu, flush):
    want, wtr, _ = whole_run(gpu, flush)
    for sched in SCHEDS[1:]:
        outs, traces, hist = run(gpu, sched_signals(), sched, SCHED_RATES, SCHED_ENCS, flush=flush)
        for g in range(3):
            assert np.array_equal(outs[g].view(np.uint8), want[g].view(np.uint8)), (sched, g)
            assert np.array_equal(traces[g], wtr[g]), (sched, g)
        core = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, R.HIST)
        assert np.array_equal(core.view(np.uint32), sched_signals()[:, -R.HIST:].view(np.uint32))   # the last 1920 native samples


def test_flushed_tail_is_the_reference_with_zeros_appended(gpu):
    outs, traces, _ = whole_run(gpu, True)
    streamed, _, _ = whole_run(gpu, False)
    for g, (pct, enc) in enumerate(zip(SCHED_RATES, SCHED_ENCS)):
        x = sched_signals()[g]
        assert outs[g].size == gpu.tsm_samples(pct, x.size, True) == 480 * -(-100 * x.size // (480 * pct)) > streamed[g].size
        assert np.array_equal(outs[g][: streamed[g].size], streamed[g])
        if enc == F32:
            check_against_reference(x, pct, outs[g], traces[g], flush=True, cap=g != 2)
        else:
            y, _, bound = R.stretch(x, pct, final=True, deltas=traces[g])
            assert np.all(np.abs(outs[g].astype(np.float64) - y * 32767.0) <= 0.5 + bound * 32767.0)
        # the zeros past the end: the same trace teacher-forces the zero-padded stream to the same samples
        yz, _, _ = R.stretch(np.concatenate([x, np.zeros(FRAME, np.float32)]), pct, deltas=np.concatenate([traces[g], np.zeros(8, np.int32)]))
        y, _, _ = R.stretch(x, pct, final=True, deltas=traces[g])
        assert np.array_equal(yz[: y.size], y)


def test_slots_of_a_larger_store_permuted_between_chunks(gpu):
    sched = SCHEDS[3]
    want, wtr, _ = whole_run(gpu, True)
    slots = np.array([[5, 0, 2], [2, 5, 0], [0, 2, 5], [5, 2, 0]], np.int32)   # the slot of each position, per chunk
    sig_of = {5: 0, 0: 1, 2: 2}                                                # which signal lives in which slot
    # a position keeps its rate and encoding, so the signals trade places only among positions of one setting: run each setting alone
    edges = np.cumsum((0,) + sched) * FRAME
    for pct, enc, g0 in zip(SCHED_RATES, SCHED_ENCS, range(3)):
        x = np.empty_like(sched_signals())
        for c in range(len(sched)):
            for p in range(3):
                x[p, edges[c]: edges[c + 1]] = sched_signals()[sig_of[slots[c, p]], edges[c]: edges[c + 1]]
        rng = np.random.default_rng(3)
        store = np.zeros((6, R.HIST), np.float32)
        store[[1, 3, 4]] = rng.uniform(-1, 1, (3, R.HIST)).astype(np.float32)  # somebody else's histories
        hist = np.concatenate([np.full(gpu.GLUE_GUARD, -3e38, np.float32), store.reshape(-1), np.full(gpu.GLUE_GUARD, -3e38, np.float32)])
        ref, rtr, _ = run(gpu, sched_signals(), sched, [pct] * 3, [enc] * 3)
        outs, traces, hist = run(gpu, x, sched, [pct] * 3, [enc] * 3, slots=slots, n_streams=6, hist=hist)
        oe = [gpu.tsm_samples(pct, int(e), False) for e in edges]
        for c in range(len(sched)):
            for p in range(3):
                s = sig_of[slots[c, p]]
                assert np.array_equal(outs[p][oe[c]: oe[c + 1]], ref[s][oe[c]: oe[c + 1]]), (pct, c, p)
                assert np.array_equal(traces[p][oe[c] // 480: oe[c + 1] // 480], rtr[s][oe[c] // 480: oe[c + 1] // 480]), (pct, c, p)
        assert np.array_equal(ref[g0][: want[g0].size], want[g0][: ref[g0].size])
        after = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(6, R.HIST)
        assert np.array_equal(after[[1, 3, 4]].view(np.uint32), store[[1, 3, 4]].view(np.uint32))
        for slot, g in sig_of.items():
            assert np.array_equal(after[slot], sched_signals()[g, -R.HIST:])


def test_reset_starts_a_new_utterance_and_leaves_the_others(gpu):
    sched = SCHEDS[3]
    want, wtr, _ = whole_run(gpu, False)
    reset = np.zeros((len(sched), 3), np.int32)
    reset[2, 1] = 1                                              # stream 1, ahead of the third chunk (frame 5)
    cut = 5 * FRAME
    counts = [gpu.tsm_samples(SCHED_RATES[0], 9 * FRAME, False),
              gpu.tsm_samples(SCHED_RATES[1], cut, False) + gpu.tsm_samples(SCHED_RATES[1], 4 * FRAME, False),
              gpu.tsm_samples(SCHED_RATES[2], 9 * FRAME, False)]
    outs, traces, _ = run(gpu, sched_signals(), sched, SCHED_RATES, SCHED_ENCS, reset_before=reset, counts=counts)
    for g in (0, 2):
        assert np.array_equal(outs[g], want[g]) and np.array_equal(traces[g], wtr[g])
    ocut = gpu.tsm_samples(SCHED_RATES[1], cut, False)
    assert np.array_equal(outs[1][:ocut], want[1][:ocut])
    fresh, ftr, _ = run(gpu, sched_signals()[:, cut:], (3, 1), SCHED_RATES, SCHED_ENCS)
    assert np.array_equal(outs[1][ocut:], fresh[1]) and np.array_equal(traces[1][ocut // 480:], ftr[1])
    assert ftr[1][0] == 0                                        # frame 0 of an utterance: the template is the candidate at offset 0
    assert not np.array_equal(outs[1][ocut: ocut + 480], want[1][ocut: ocut + 480])   # and that differs from the stream that went on


def test_mixed_rates_and_a_native_stream_in_one_launch(gpu):
    x = sched_signals()
    rates, encs = [100, 50, 160], [F32, S16, F32]
    outs, traces, hist = run(gpu, x, SCHEDS[3], rates, encs, flush=True)
    assert np.array_equal(outs[0].view(np.uint32), x[0].view(np.uint32)) and traces[0].size == 0   # the native stream: the input bits
    core = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(3, R.HIST)
    assert not core[0].any()                                     # a native stream keeps no state
    alone, atr, _ = run(gpu, x[1:2], SCHEDS[0], [50], [S16], flush=True)
    assert np.array_equal(outs[1], alone[0]) and np.array_equal(traces[1], atr[0])
    check_against_reference(x[2], 160, outs[2], traces[2], flush=True, cap=False)   # the periodic signal: ties by construction


def test_silence_chooses_offset_zero(gpu):
    x = np.stack([np.zeros(3 * FRAME, np.float32), R.speech_like(3, 5)])
    outs, traces, _ = run(gpu, x, (1, 2), [125, 125])
    assert not outs[0].any() and not traces[0].any()             # all-zero input: offset 0 everywhere


@pytest.mark.parametrize("what", ["chunk length", "zero chunk", "no stream", "stream twice", "stream out of range", "rate 49", "rate 201", "encoding"])
def test_launcher_refusals_write_nothing(gpu, what):
    x, rates, encs, slots, chunks = sched_signals()[:, : 2 * FRAME], [80, 125, 200], [F32, S16, F32], [[0, 1, 2]], [2 * FRAME]
    if what == "chunk length":
        chunks = [2 * FRAME - 920]
    elif what == "zero chunk":
        chunks, x = [0], x[:, :0]
    elif what == "no stream":
        x, rates, encs, slots = x[:0], [], [], [[]]
    elif what == "stream twice":
        slots = [[0, 1, 0]]
    elif what == "stream out of range":
        slots = [[0, 1, 3]]
    elif what == "rate 49":
        rates = [80, 49, 200]
    elif what == "rate 201":
        rates = [201, 125, 200]
    else:
        encs = [F32, 2, F32]
    with pytest.raises(gpu.Q3Error) as ei:
        gpu.op_tsm(x, chunks, slots, 3, rates, encs, flush=True, slack=8, fill=FILL)
    ex = ei.value
    assert "tsm stretch" in str(ex) and len(ex.wholes) == len(rates)
    assert all(np.all(w == FILL) for w in ex.wholes) and all(np.all(t == 0x5A5A5A5A) for t in ex.twholes) and np.all(ex.n_out == -1)
    assert not ex.hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].any() and np.all(ex.hist[: gpu.GLUE_GUARD] == np.float32(-3e38))
