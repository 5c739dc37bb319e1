"""[EXT] volume: the kernel (csrc/volume.hip, k_volume) through q3tts_op_volume against include/q3tts_spec.h "volume" as tests/volume_ref.py
restates it.  Where nothing exceeds 1 the output is fl(G x) delayed by 127 samples, bit for bit; where the limiter works, y lies within
10 u |y64| + 2^-149 of the float64 evaluation of the same f32 v, the gain trace within 8 u |g64|, and |y| <= 1.  The output, the trace and
the state never depend on how the stream was cut into chunks.  Nine frames at most; one reference per signal, shared."""
import functools

import numpy as np
import pytest

import volume_ref as R

pytestmark = pytest.mark.gpu
FRAME, GUARD, FILL = 1920, np.float32(-3e38), 0xA5
SCHEDS = ((9,), (4, 4, 1), (1,) * 9, (1, 4, 3, 1))


@functools.lru_cache(maxsize=None)
def speech():
    x = R.speech_like(9)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(db10):
    """(v, y64, g64) of the speech-like signal at a volume"""
    v = R.scaled(speech(), db10)
    y, g, _ = R.volume64(v)
    return v, y, g


def run(gpu, x, sched, vols, slots=None, n_streams=None, hist=None, reset_before=None, trace=True):
    """x [G][n] through the kernel in chunks of sched frames; checks the counts and every guard; returns (outs, traces, hist)"""
    x = np.atleast_2d(x)
    G = x.shape[0]
    n_streams = n_streams or G
    sl = np.tile(np.arange(G, dtype=np.int32), (len(sched), 1)) if slots is None else slots
    outs, traces, wholes, twholes, n_out, hist = gpu.op_volume(x, [f * FRAME for f in sched], sl, n_streams, vols, reset_before=reset_before,
                                                               hist=hist, trace=trace, slack=8, fill=FILL)
    n = sum(sched) * FRAME
    assert list(n_out) == [n] * G and all(o.size == n for o in outs)
    for w in wholes + twholes:                                   # the guards in front, the slack and the guards behind: untouched
        assert np.all(w[: gpu.GLUE_GUARD * 4] == FILL) and np.all(w[(gpu.GLUE_GUARD + n) * 4:] == FILL)
    assert np.all(hist[: gpu.GLUE_GUARD] == GUARD) and np.all(hist[-gpu.GLUE_GUARD:] == GUARD)
    return outs, traces, hist


def delayed(v):
    return np.concatenate([np.zeros(R.DELAY, np.float32), v[:-R.DELAY]])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def state(gpu, hist, n_streams):
    return hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(n_streams, R.HIST)


# -------------------------------------------------------- 1: nothing exceeds 1 --------------------------------------------------------
@pytest.mark.parametrize("db10,sig", [(-60, "speech"), (-400, "speech"), (60, "quiet")])
def test_attenuation_and_a_quiet_boost_are_the_delayed_product_bit_for_bit(gpu, db10, sig):
    x = speech() if sig == "speech" else R.quiet(9)
    v = R.scaled(x, db10)
    assert 0 < np.abs(v).max() <= 1.0
    outs, traces, hist = run(gpu, x, SCHEDS[1], [db10])
    assert np.array_equal(bits(outs[0]), bits(delayed(v)))
    assert np.all(traces[0] == 1.0)
    assert np.array_equal(bits(state(gpu, hist, 1)[0]), bits(v[-R.HIST:]))   # the state: the last 638 values of v


# -------------------------------------------------------- 2: the limiter engaged --------------------------------------------------------
@pytest.mark.parametrize("db10", (120, 200))
def test_limiter_engaged_stays_inside_the_bound(gpu, db10):
    v, y64, g64 = reference(db10)
    outs, traces, hist = run(gpu, speech(), SCHEDS[0], [db10])
    y, g = outs[0].astype(np.float64), traces[0].astype(np.float64)
    ey, eg = np.abs(y - y64) / R.y_bound(y64), np.abs(g - g64) / R.g_bound(g64)
    y32, g32 = R.volume32(v)
    print("+%d dB: %.1f %% of the samples limited, smallest gain %.4f, y error at most %.3f of the bound, g error at most %.3f of its bound, "
          "equal to the f32 twin: y %s, g %s" % (db10 // 10, 100 * np.mean(g64 < 1), g64.min(), ey.max(), eg.max(),
                                               np.array_equal(bits(outs[0]), bits(y32)), np.array_equal(bits(traces[0]), bits(g32))))
    assert np.mean(g64 < 1) > 0.4 and g64.min() < 0.5            # the limiter is at work on a large share of the signal
    assert np.all(ey <= 1.0), ey.max()
    assert np.all(eg <= 1.0), eg.max()
    assert np.abs(outs[0]).max() <= 1.0 and np.abs(outs[0]).max() > 0.9
    assert np.array_equal(bits(state(gpu, hist, 1)[0]), bits(v[-R.HIST:]))


def test_the_impulse(gpu):
    x = np.zeros(3 * FRAME, np.float32)
    x[1000] = 1.0
    outs, traces, _ = run(gpu, x, (1, 1, 1), [200])
    y, g = outs[0], traces[0]
    below = np.nonzero(g < 1.0)[0]
    assert below[0] == 1000 and below[-1] == 1638 and below.size == 639         # g < 1 exactly on [1000, 1638]
    assert np.all(np.abs(g[1127:1512].astype(np.float64) - 0.1) <= 8 * R.U * 0.1)   # g = 0.1 on [1127, 1511]
    assert abs(float(y[1127]) - 1.0) <= float(R.y_bound(1.0)) and np.count_nonzero(y) == 1


@pytest.mark.parametrize("at", (0, FRAME - 1, FRAME, FRAME + 126, FRAME + 127, FRAME + 637))
def test_a_peak_at_every_history_edge(gpu, at):
    """[1, 1, 1] frames: a peak at the chunk's first and last sample and where the next chunk's delay line and hold window begin and end"""
    x = (np.float32(0.05) * R.speech_like(3, 7)).astype(np.float32)
    x[at] = np.float32(-0.8)
    v = R.scaled(x, 200)
    y64, g64, _ = R.volume64(v)
    outs, traces, _ = run(gpu, x, (1, 1, 1), [200])
    y, g = outs[0].astype(np.float64), traces[0].astype(np.float64)
    assert np.all(np.abs(y - y64) <= R.y_bound(y64)) and np.all(np.abs(g - g64) <= R.g_bound(g64))
    assert np.all(traces[0][at: at + R.HIST + 1] < 1.0) and np.all(traces[0][:at] == 1.0) and np.all(traces[0][at + R.HIST + 1:] == 1.0)
    assert abs(abs(y[at + R.DELAY]) - 1.0) <= 1e-6


def test_silence_and_negative_zero(gpu):
    x = np.stack([np.zeros(2 * FRAME, np.float32), np.full(2 * FRAME, -0.0, np.float32)])
    outs, traces, hist = run(gpu, x, (1, 1), [120, 120])
    assert not bits(outs[0]).any()                                              # +0 everywhere
    assert not bits(outs[1][: R.DELAY]).any() and np.all(bits(outs[1][R.DELAY:]) == 0x80000000)   # v[n < 0] = +0, then G * -0 = -0
    assert np.all(traces[0] == 1.0) and np.all(traces[1] == 1.0)
    assert np.all(bits(state(gpu, hist, 2)[1]) == 0x80000000)


# -------------------------------------------------------- 3: chunking, slots, resets --------------------------------------------------------
@functools.lru_cache(maxsize=None)
def three():
    x = np.stack([speech(), R.speech_like(9, 11), R.quiet(9)])
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def whole(gpu):
    """the three signals in one chunk of nine frames: what every other schedule must reproduce"""
    return run(gpu, three(), SCHEDS[0], [120, 200, -60])


@pytest.mark.parametrize("sched", SCHEDS[1:])
def test_schedules_give_bit_identical_outputs_traces_and_state(gpu, whole, sched):
    want, wtr, whist = whole
    outs, traces, hist = run(gpu, three(), sched, [120, 200, -60])
    for g in range(3):
        assert np.array_equal(bits(outs[g]), bits(want[g])) and np.array_equal(bits(traces[g]), bits(wtr[g])), g
    assert np.array_equal(bits(hist), bits(whist))
    v = R.scaled(three()[0], 120)
    y64, g64, _ = R.volume64(v)
    assert np.all(np.abs(outs[0].astype(np.float64) - y64) <= R.y_bound(y64))


def test_slots_of_a_larger_store_permuted_between_chunks(gpu):
    sched = SCHEDS[3]
    slots = np.array([[5, 0, 2], [2, 5, 0], [0, 2, 5], [5, 2, 0]], np.int32)   # the slot of each position, per chunk
    sig_of = {5: 0, 0: 1, 2: 2}                                                # which signal lives in which slot
    edges = np.cumsum((0,) + sched) * FRAME
    sig = three()
    x = np.empty_like(sig)
    for c in range(len(sched)):
        for p in range(3):
            x[p, edges[c]: edges[c + 1]] = sig[sig_of[slots[c, p]], edges[c]: edges[c + 1]]
    store = np.zeros((6, R.HIST), np.float32)
    store[[1, 3, 4]] = np.random.default_rng(3).uniform(-1, 1, (3, R.HIST)).astype(np.float32)   # somebody else's state in the other slots
    guarded = np.concatenate([np.full(gpu.GLUE_GUARD, GUARD, np.float32), store.reshape(-1), np.full(gpu.GLUE_GUARD, GUARD, np.float32)])
    ref, rtr, rhist = run(gpu, sig, sched, [200] * 3)
    outs, traces, hist = run(gpu, x, sched, [200] * 3, slots=slots, n_streams=6, hist=guarded)
    for c in range(len(sched)):
        for p in range(3):
            s = sig_of[slots[c, p]]
            assert np.array_equal(bits(outs[p][edges[c]: edges[c + 1]]), bits(ref[s][edges[c]: edges[c + 1]])), (c, p)
            assert np.array_equal(bits(traces[p][edges[c]: edges[c + 1]]), bits(rtr[s][edges[c]: edges[c + 1]])), (c, p)
    after, alone = state(gpu, hist, 6), state(gpu, rhist, 3)
    assert np.array_equal(bits(after[[1, 3, 4]]), bits(store[[1, 3, 4]]))
    for slot, g in sig_of.items():
        assert np.array_equal(bits(after[slot]), bits(alone[g]))


def test_reset_starts_a_new_utterance_and_leaves_the_others(gpu, whole):
    sched = SCHEDS[3]
    want, wtr, whist = whole
    reset = np.zeros((len(sched), 3), np.int32)
    reset[2, 1] = 1                                              # stream 1, ahead of the third chunk (frame 5)
    cut = 5 * FRAME
    outs, traces, hist = run(gpu, three(), sched, [120, 200, -60], reset_before=reset)
    for g in (0, 2):
        assert np.array_equal(bits(outs[g]), bits(want[g])) and np.array_equal(bits(traces[g]), bits(wtr[g]))
    assert np.array_equal(bits(state(gpu, hist, 3)), bits(state(gpu, whist, 3)))   # the state is the chunk's last values, whatever came before
    assert np.array_equal(bits(outs[1][:cut]), bits(want[1][:cut]))
    fresh, ftr, _ = run(gpu, three()[:, cut:], (3, 1), [120, 200, -60])
    assert np.array_equal(bits(outs[1][cut:]), bits(fresh[1])) and np.array_equal(bits(traces[1][cut:]), bits(ftr[1]))
    assert not outs[1][cut: cut + R.DELAY].any()                 # a new utterance: 127 zeros first
    assert not np.array_equal(bits(outs[1][cut: cut + R.HIST]), bits(want[1][cut: cut + R.HIST]))   # which the stream that went on does not have


def test_mixed_volumes_leave_a_stream_without_one_untouched(gpu):
    x = three()
    outs, traces, hist = run(gpu, x, SCHEDS[3], [200, 0, -60])
    want, wtr, whist = run(gpu, x[[0, 2]], SCHEDS[3], [200, -60])
    assert np.array_equal(bits(outs[1]), bits(x[1]))             # volume 0: the input's bytes, not delayed
    assert np.all(traces[1].view(np.uint8) == FILL)              # and no trace
    assert not state(gpu, hist, 3)[1].any()                      # and no state
    for g, w in ((0, 0), (2, 1)):
        assert np.array_equal(bits(outs[g]), bits(want[w])) and np.array_equal(bits(traces[g]), bits(wtr[w]))
        assert np.array_equal(bits(state(gpu, hist, 3)[g]), bits(state(gpu, whist, 2)[w]))
    quiet, _, qh = run(gpu, x, (2,), [0, 0, 0], trace=False)     # no stream has a volume: nothing runs
    assert np.array_equal(bits(np.stack(quiet)), bits(x[:, : 2 * FRAME])) and not state(gpu, qh, 3).any()


# -------------------------------------------------------- 4: refusals --------------------------------------------------------
@pytest.mark.parametrize("what", ["chunk length", "zero chunk", "no stream", "stream twice", "stream out of range", "volume 201", "volume -401"])
def test_launcher_refusals_write_nothing(gpu, what):
    x, vols, slots, chunks = three()[:, : 2 * FRAME], [120, 0, -60], [[0, 1, 2]], [2 * FRAME]
    if what == "chunk length":
        chunks = [2 * FRAME - 920]
    elif what == "zero chunk":
        chunks, x = [0], x[:, :0]
    elif what == "no stream":
        x, vols, slots = x[:0], [], [[]]
    elif what == "stream twice":
        slots = [[0, 1, 0]]
    elif what == "stream out of range":
        slots = [[0, 1, 3]]
    elif what == "volume 201":
        vols = [120, 201, -60]
    else:
        vols = [120, 0, -401]
    with pytest.raises(gpu.Q3Error) as ei:
        gpu.op_volume(x, chunks, slots, 3, vols, slack=8, fill=FILL)
    ex = ei.value
    assert "volume: " in str(ex) and len(ex.wholes) == len(vols)
    assert all(np.all(w == FILL) for w in ex.wholes) and all(np.all(t == FILL) for t in ex.twholes) and np.all(ex.n_out == -1)
    h = ex.hist
    assert not h[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].any() and np.all(h[: gpu.GLUE_GUARD] == GUARD) and np.all(h[-gpu.GLUE_GUARD:] == GUARD)
