"""[EXT] the loudness kernel through q3tts_op_loudness (include/q3tts_spec.h "loudness"): rows and final state bit for bit against the
segmented float64 restatement (tests/loudness_ref.py) fed the library's own tables, at every chunk length that takes another path through the
kernel (no block completes, a block ends inside the chunk, the chunk ends on a block edge, more segments than one batch of lanes), on
signals that sit on the segment and block edges; independence of the chunking; streams side by side with an unmetered one between them;
slots of a larger store permuted between chunks; resets; guards; refusals that write nothing."""
import numpy as np
import pytest

import loudness_ref as R

pytestmark = pytest.mark.gpu
F = R.FRAME


@pytest.fixture(scope="module")
def tab(gpu):
    coef, M = gpu.loudness_tables()
    coef.setflags(write=False); M.setflags(write=False)
    return coef, M


def same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(R.bits(a), R.bits(b))


def core(gpu, state, n_streams):
    return state[gpu.GLUE_GUARD: gpu.GLUE_GUARD + n_streams * R.STATE].reshape(n_streams, R.STATE)


def guards_intact(gpu, wholes, want_rows, state, fill=0x5A):
    g = gpu.GLUE_GUARD
    for w, n in zip(wholes, want_rows):
        assert np.all(w[: g * 16] == fill) and np.all(w[(g + n) * 16:] == fill)
    assert np.all(state[:g] == -3e300) and np.all(state[-g:] == -3e300)


SIGNALS = {
    "noise": lambda n: R.noise(n),
    "impulse 95": lambda n: R.impulse(n, 95), "impulse 96": lambda n: R.impulse(n, 96),
    "impulse 2399": lambda n: R.impulse(n, 2399), "impulse 2400": lambda n: R.impulse(n, 2400),
    "impulse 1919": lambda n: R.impulse(n, 1919), "impulse 1920": lambda n: R.impulse(n, 1920),
    "silence": lambda n: np.zeros(n, np.float32), "minus zero": lambda n: np.full(n, -0.0, np.float32),
    "square": lambda n: R.square(n), "dc": lambda n: np.full(n, 0.5, np.float32),
}


@pytest.mark.parametrize("frames", (1, 2, 4, 5, 6))
@pytest.mark.parametrize("name", sorted(SIGNALS))
def test_rows_and_state_are_the_restatement_bit_for_bit(gpu, tab, name, frames):
    """one chunk of 1 (no block completes), 2, 4, 5 (ends on a block edge) and 6 frames"""
    coef, M = tab
    n = frames * F
    if name.startswith("impulse") and int(name.split()[1]) >= n:
        n = 2 * F                                                           # the impulse needs room: two frames, cut as (1, 1) below
    x = SIGNALS[name](n)
    chunks = [n] if n == frames * F else [F, F]
    rows, wholes, n_rows, state = gpu.op_loudness(x[None, :], chunks, [[0]] * len(chunks), 1, [1], slack=3)
    want_rows, want_state = R.segmented(x, coef, M, chunks)
    assert n_rows[0] == want_rows.shape[0] == n // R.BLOCK
    assert same(rows[0], want_rows) and same(core(gpu, state, 1)[0], want_state), name
    guards_intact(gpu, wholes, [want_rows.shape[0]], state)
    assert np.all(wholes[0][(gpu.GLUE_GUARD + n_rows[0]) * 16:] == 0x5A)   # the slack behind the rows too
    if name in ("silence", "minus zero"):
        assert not rows[0].any() and not core(gpu, state, 1).any() and not np.signbit(rows[0]).any()


def test_a_chunk_of_more_segments_than_lanes(gpu, tab):
    """12 frames = 240 segments: two batches of 128 lanes, the walk's state carried between them"""
    coef, M = tab
    x = R.noise(12 * F, 0.3, 21)
    rows, wholes, n_rows, state = gpu.op_loudness(x[None, :], [12 * F], [[0]], 1, [1])
    want_rows, want_state = R.segmented(x, coef, M)
    assert n_rows[0] == 9 and same(rows[0], want_rows) and same(core(gpu, state, 1)[0], want_state)
    seq = R.sequential_rows(x, coef)
    assert np.abs(rows[0][:, 0] - seq[:, 0]).max() / seq[:, 0].min() < 1e-10 and np.array_equal(rows[0][:, 1], seq[:, 1])


@pytest.mark.parametrize("name", ("noise", "dc"))
def test_schedules_of_one_signal_are_bit_identical(gpu, tab, name):
    coef, M = tab
    x = SIGNALS[name](5 * F)
    want_rows, want_state = R.segmented(x, coef, M)
    assert want_rows.shape == (4, 2)
    for sched in ((1, 1, 1, 1, 1), (4, 1), (2, 3), (1, 4), (5,)):
        chunks = [k * F for k in sched]
        rows, _, n_rows, state = gpu.op_loudness(x[None, :], chunks, [[0]] * len(chunks), 1, [1])
        assert n_rows[0] == 4 and same(rows[0], want_rows) and same(core(gpu, state, 1)[0], want_state), sched


@pytest.mark.parametrize("G", (1, 2, 3))
def test_streams_side_by_side_with_an_unmetered_one_between(gpu, tab, G):
    coef, M = tab
    chunks = [2 * F, F, 3 * F]
    x = np.stack([R.noise(6 * F, 0.2 + 0.1 * g, 30 + g) for g in range(G)])
    metered = [1, 0, 1][:G] if G == 3 else [1] * G
    slots = [[g for g in range(G)]] * len(chunks)
    rows, wholes, n_rows, state = gpu.op_loudness(x, chunks, slots, G, metered)
    want_n = []
    for g in range(G):
        if metered[g]:
            want_rows, want_state = R.segmented(x[g], coef, M, chunks)
            assert n_rows[g] == 4 and same(rows[g], want_rows) and same(core(gpu, state, G)[g], want_state), g
            want_n.append(4)
        else:
            assert n_rows[g] == 0 and np.all(wholes[g] == 0x5A) and not core(gpu, state, G)[g].any()   # left unwritten
            want_n.append(0)
    guards_intact(gpu, wholes, want_n, state)


def test_slots_of_a_larger_store_permuted_between_chunks(gpu, tab):
    """three positions walk over slots of a store of seven; a position's rows follow the slot it reads in each chunk"""
    coef, M = tab
    chunks, n_streams = [F, 2 * F, F, 2 * F], 7
    slots = [[5, 0, 3], [0, 3, 5], [3, 5, 0], [5, 0, 3]]
    x = np.stack([R.noise(6 * F, 0.3, 40 + g) for g in range(3)])
    rows, wholes, n_rows, state = gpu.op_loudness(x, chunks, slots, n_streams, [1, 1, 1])
    st = {s: R.fresh_state() for s in range(n_streams)}
    pos = {s: 0 for s in range(n_streams)}
    want = [[np.zeros((0, 2))] for _ in range(3)]
    at = 0
    for c, T in enumerate(chunks):
        for g in range(3):
            s = slots[c][g]
            r, st[s] = R.chunk(x[g, at: at + T], pos[s], st[s], coef, M)
            pos[s] += T
            want[g].append(r)
        at += T
    for g in range(3):
        w = np.concatenate(want[g])
        assert n_rows[g] == w.shape[0] and same(rows[g], w), g
    for s in range(n_streams):
        assert same(core(gpu, state, n_streams)[s], st[s]), s                # the four slots nobody used stay zero
    guards_intact(gpu, wholes, [int(n) for n in n_rows], state)


def test_a_reset_between_utterances_leaves_the_other_slots_alone(gpu, tab):
    coef, M = tab
    chunks = [2 * F, 2 * F]
    x = np.stack([R.noise(4 * F, 0.3, 50), R.noise(4 * F, 0.3, 51)])
    rows, _, n_rows, state = gpu.op_loudness(x, chunks, [[1, 2], [1, 2]], 4, [1, 1], reset_before=[[0, 0], [1, 0]])
    a1, _ = R.segmented(x[0, : 2 * F], coef, M)                            # position 0: two utterances of two frames
    a2, sa = R.segmented(x[0, 2 * F:], coef, M)
    b, sb = R.segmented(x[1], coef, M, chunks)                             # position 1: one of four
    assert n_rows[0] == 2 and n_rows[1] == 3
    assert same(rows[0], np.concatenate([a1, a2])) and same(rows[1], b)
    assert same(core(gpu, state, 4)[1], sa) and same(core(gpu, state, 4)[2], sb) and not core(gpu, state, 4)[[0, 3]].any()


def test_a_store_that_is_not_zero_continues_the_stream(gpu, tab):
    """the state store goes in as well as out: the second half of a stream from the first half's state"""
    coef, M = tab
    x = R.noise(5 * F, 0.3, 60)
    want_rows, want_state = R.segmented(x, coef, M)
    r1, _, _, st = gpu.op_loudness(x[None, : 2 * F], [2 * F], [[0]], 1, [1])
    assert r1[0].shape == (1, 2)
    mid = core(gpu, st, 1)[0].copy()
    r2, s2 = R.chunk(x[2 * F:], 2 * F, mid, coef, M)                        # what the restatement makes of the device's state
    assert same(np.concatenate([r1[0], r2]), want_rows) and same(s2, want_state)


def test_refusals_write_nothing(gpu):
    x = R.noise(2 * F)[None, :]
    two = np.stack([x[0], x[0]])

    def refused(match, *a, **kw):
        with pytest.raises(gpu.Q3Error, match=match) as ei:
            gpu.op_loudness(*a, **kw)
        ex = ei.value
        assert all(np.all(w == 0x5A) for w in ex.wholes) and np.all(ex.n_out == -1)
        g = gpu.GLUE_GUARD
        assert not ex.state[g:-g].any() and np.all(ex.state[:g] == -3e300) and np.all(ex.state[-g:] == -3e300)

    refused("1920", x[:, :2400], [2400], [[0]], 1, [1])
    refused("1920", x[:, :960], [960], [[0]], 1, [1])
    refused("1920", x, [F, 0], [[0], [0]], 1, [1])
    refused("stream out of range", x, [2 * F], [[1]], 1, [1])
    refused("stream out of range", x, [2 * F], [[-1]], 1, [1])
    refused("once", two, [2 * F], [[1, 1]], 2, [1, 1])
    refused("once", two, [F, F], [[0, 1], [1, 1]], 2, [1, 0])              # checked in every chunk before the first launch
    refused("group", np.zeros((0, 2 * F), np.float32), [2 * F], np.zeros((1, 0), np.int32), 1, [])
    L = gpu.lib()
    cs, sl, me, nb, nr = np.array([2 * F], np.int32), np.zeros(1, np.int32), np.ones(1, np.int32), np.array([4096], np.int64), np.full(1, -1, np.int64)
    whole = np.full(4096, 0x5A, np.uint8)
    state = np.zeros(R.STATE + 2 * gpu.GLUE_GUARD)
    ptrs = (gpu.C.c_void_p * 1)(whole.ctypes.data)
    p = gpu._p
    for args in ((None, 1, p(cs), 1, p(sl), 1, p(me), None, ptrs, p(nb), p(nr), p(state)),
                 (p(x), 1, None, 1, p(sl), 1, p(me), None, ptrs, p(nb), p(nr), p(state)),
                 (p(x), 1, p(cs), 1, None, 1, p(me), None, ptrs, p(nb), p(nr), p(state)),
                 (p(x), 1, p(cs), 1, p(sl), 1, None, None, ptrs, p(nb), p(nr), p(state)),
                 (p(x), 1, p(cs), 1, p(sl), 1, p(me), None, None, p(nb), p(nr), p(state)),
                 (p(x), 1, p(cs), 1, p(sl), 1, p(me), None, ptrs, None, p(nr), p(state)),
                 (p(x), 1, p(cs), 1, p(sl), 1, p(me), None, ptrs, p(nb), None, p(state)),
                 (p(x), 1, p(cs), 1, p(sl), 1, p(me), None, ptrs, p(nb), p(nr), None)):
        assert L.q3tts_op_loudness(*args) < 0 and b"null" in L.q3tts_last_error()
        assert np.all(whole == 0x5A) and nr[0] == -1 and not state.any()
    small = np.array([2 * gpu.GLUE_GUARD * 16], np.int64)                   # room for the guards, none for the row
    assert L.q3tts_op_loudness(p(x), 1, p(cs), 1, p(sl), 1, p(me), None, ptrs, p(small), p(nr), p(state)) < 0 and b"too small" in L.q3tts_last_error()
    assert np.all(whole == 0x5A) and nr[0] == -1 and not state.any()
