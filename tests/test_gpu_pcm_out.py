"""[EXT] output formats on the GPU: k_pcm_convert through q3tts_op_pcm_convert, one launch of the engine's launcher per chunk, against the
float64 reference of tests/pcm_out_ref.py.  The reference is fed the library's own f32 table, so only the kernel's arithmetic is judged: an
f32 result must lie within the reference's per-sample running-error bound, an s16 result must be the rounding of the f32 one.  Every output
buffer and the history store come back whole and are checked to the last guard element."""
import functools

import numpy as np
import pytest

import pcm_out_ref as R

pytestmark = pytest.mark.gpu

G, FRAMES, SCHED = 3, 9, (1, 4, 3, 1)
FORMATS = [(r, e) for r in R.RATES for e in (R.F32, R.S16) if R.allowed(r, e)]
FILL = 0x5A
# 22050 Hz s16 gives 3528 bytes a frame, 8 past a multiple of 16: after the 1-frame chunk of SCHED its outputs start off 16 bytes and take the
# kernel's scalar stores; every other format stays on the 16-byte ones
assert (R.n_out(22050, R.FRAME) * 2) % 16 == 8 and all((R.n_out(r, R.FRAME) * (2 if e else 4)) % 16 == 0 for r, e in FORMATS if (r, e) != (22050, R.S16))


@functools.lru_cache(maxsize=None)
def signals():
    """[3][9 frames]: uniform noise in [-1, 1], a 200-sample full-scale square wave (the filter overshoots it and the clamp engages), isolated
    exact +-1.0 samples; stream g differs from the others in all three"""
    rng = np.random.default_rng(20240607)
    x = rng.uniform(-1.0, 1.0, (G, FRAMES * R.FRAME)).astype(np.float32)
    for g in range(G):
        at = 3000 + 5000 * g                                   # inside a chunk of every schedule used here, and across the 1|4 frame cut for g = 0
        x[g, at: at + 100] = 1.0 if g != 1 else -1.0
        x[g, at + 100: at + 200] = -1.0 if g != 1 else 1.0
        x[g, [7, 1919 + g, 1920 * 5 + 11 * g, x.shape[1] - 1 - g]] = [1.0, -1.0, 1.0, -1.0]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def reference(gpu_mod, g, rate, start=0):
    """(y, bound) of stream g from native sample `start` on, by the whole-signal form over the library's table"""
    h32 = gpu_mod.pcm_out_filter(rate) if rate != R.NATIVE else None
    return R.convert(signals()[g, start:], rate, h32)


def run(gpu, x, sched, fmts, slots=None, n_streams=None, **kw):
    """one q3tts_op_pcm_convert; checks what every case must hold: counts, guards, the unwritten slack"""
    slots = np.tile(np.arange(len(fmts), dtype=np.int32), (len(sched), 1)) if slots is None else np.asarray(slots, np.int32)
    n_streams = len(fmts) if n_streams is None else n_streams
    outs, wholes, n_out, hist = gpu.op_pcm_convert(x, [f * R.FRAME for f in sched], slots, n_streams, fmts, slack=8, fill=FILL, **kw)
    n_native = sum(sched) * R.FRAME
    for o, w, n, (rate, enc) in zip(outs, wholes, n_out, fmts):
        assert n == o.size == gpu.pcm_out_samples(rate, n_native) == R.n_out(rate, n_native)
        gb = gpu.GLUE_GUARD * o.dtype.itemsize
        assert np.all(w[:gb] == FILL) and np.all(w[gb + o.nbytes:] == FILL), "a write outside the stream's output"
    assert np.all(hist[: gpu.GLUE_GUARD] == np.float32(-3e38)) and np.all(hist[-gpu.GLUE_GUARD:] == np.float32(-3e38)), "history guards"
    return outs, hist


@functools.lru_cache(maxsize=None)
def single_format(gpu_mod, fmt, sched=SCHED):
    """all three streams in one format"""
    outs, hist = run(gpu_mod, signals(), sched, [fmt] * G)
    for o in outs:
        o.setflags(write=False)
    return outs, hist


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d_%s" % (f[0], "s16" if f[1] else "f32"))
def test_every_format_against_the_reference(gpu, fmt):
    rate, enc = fmt
    outs, _ = single_format(gpu, fmt)
    for g in range(G):
        y, bound = reference(gpu, g, rate)
        o = outs[g]
        assert o.dtype == (np.int16 if enc else np.float32) and o.size == y.size
        if rate == R.NATIVE and enc == R.F32:       # native: the input bits
            assert np.array_equal(o.view(np.uint32), signals()[g].view(np.uint32))
        elif rate == R.NATIVE:                      # the clamp and the rounding alone
            assert np.array_equal(o, R.s16_of(np.clip(signals()[g], -1.0, 1.0)))
        elif enc == R.F32:
            err = np.abs(o.astype(np.float64) - y)
            print("%d f32 stream %d: max err %.3g, max err/bound %.3g" % (rate, g, err.max(), (err / np.maximum(bound, 1e-300)).max()))
            assert np.all(err <= bound)
            assert np.abs(o).max() == 1.0           # the square wave's overshoot met the clamp
        elif rate <= R.NATIVE:                      # the same clamped f32 value, rounded: bit for bit
            assert np.array_equal(o, R.s16_of(single_format(gpu, (rate, R.F32))[0][g]))
        else:                                       # no f32 run to hold it against: the reference's rounding, exact away from ties
            v = y * 32767.0
            r = np.rint(v)
            clear = 0.5 - np.abs(v - r) > bound * 32767.0
            d = o.astype(np.int64) - r.astype(np.int64)
            print("%d s16 stream %d: %d of %d samples within their bound of a tie" % (rate, g, (~clear).sum(), v.size))
            assert np.all(d[clear] == 0) and np.all(np.abs(d) <= 1) and clear.mean() > 0.5
            assert np.abs(o).max() == 32767


@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: "%d_%s" % (f[0], "s16" if f[1] else "f32"))
def test_chunk_schedule_does_not_matter(gpu, fmt):
    """the tail of a chunk is handed over through the history store while other blocks of the same launch still read the old one"""
    want, whist = single_format(gpu, fmt)
    for sched in ((9,), (4, 4, 1), (1,) * 9):
        outs, hist = run(gpu, signals(), sched, [fmt] * G)
        for g in range(G):
            assert np.array_equal(outs[g].view(np.uint8), want[g].view(np.uint8)), (sched, g)
        if fmt[0] != R.NATIVE:   # the live half (chunks converted & 1) holds the signal's last 96 samples
            core = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(G, 2, R.HIST)
            for g in range(G):
                assert np.array_equal(core[g, len(sched) & 1], signals()[g, -R.HIST:])


def test_slots_of_a_larger_store_permuted_between_chunks(gpu):
    fmt = (16000, R.S16)
    want, _ = single_format(gpu, fmt)
    slots = np.array([[5, 0, 2], [2, 5, 0], [0, 2, 5], [5, 2, 0]], np.int32)   # the slot of each position, per chunk
    sig_of = {5: 0, 0: 1, 2: 2}                                                # which signal lives in which slot
    x = np.empty_like(signals())
    edges = np.cumsum((0,) + SCHED) * R.FRAME
    for c in range(len(SCHED)):
        for p in range(G):
            x[p, edges[c]: edges[c + 1]] = signals()[sig_of[slots[c, p]], edges[c]: edges[c + 1]]
    rng = np.random.default_rng(3)
    store = np.zeros((6, 2, R.HIST), np.float32)
    store[[1, 3, 4]] = rng.uniform(-1, 1, (3, 2, R.HIST)).astype(np.float32)   # somebody else's histories
    hist = np.concatenate([np.full(gpu.GLUE_GUARD, -3e38, np.float32), store.reshape(-1), np.full(gpu.GLUE_GUARD, -3e38, np.float32)])
    outs, hist = run(gpu, x, SCHED, [fmt] * G, slots=slots, n_streams=6, hist=hist)
    oe = edges * 2 // 3
    for c in range(len(SCHED)):
        for p in range(G):
            assert np.array_equal(outs[p][oe[c]: oe[c + 1]], want[sig_of[slots[c, p]]][oe[c]: oe[c + 1]]), (c, p)
    after = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(6, 2, R.HIST)
    assert np.array_equal(after[[1, 3, 4]].view(np.uint32), store[[1, 3, 4]].view(np.uint32))
    for slot, g in sig_of.items():   # four chunks: half 0 is live again and holds the last tail, half 1 the one before
        assert np.array_equal(after[slot, 0], signals()[g, -R.HIST:])
        assert np.array_equal(after[slot, 1], signals()[g, edges[3] - R.HIST: edges[3]])


@pytest.mark.parametrize("fmt", [(8000, R.F32), (44100, R.S16)], ids=["8000_f32", "44100_s16"])
def test_reset_makes_a_fresh_stream_and_leaves_the_others(gpu, fmt):
    want, _ = single_format(gpu, fmt)
    reset = np.zeros((len(SCHED), G), np.int32)
    reset[2, 1] = 1                                              # stream 1, ahead of the third chunk (frame 5)
    outs, _ = run(gpu, signals(), SCHED, [fmt] * G, reset_before=reset)
    for g in (0, 2):
        assert np.array_equal(outs[g], want[g])
    cut, ocut = 5 * R.FRAME, R.n_out(fmt[0], 5 * R.FRAME)
    assert np.array_equal(outs[1][:ocut], want[1][:ocut])
    fresh, _ = run(gpu, signals()[:, cut:], (3, 1), [fmt] * G)
    assert np.array_equal(outs[1][ocut:], fresh[1])
    assert not np.array_equal(outs[1][ocut: ocut + 8], want[1][ocut: ocut + 8])   # and that differs from the stream that went on
    y, bound = reference(gpu, 1, fmt[0], cut)
    if fmt[1] == R.F32:
        assert np.all(np.abs(fresh[1].astype(np.float64) - y) <= bound)
    else:
        assert np.all(np.abs(fresh[1].astype(np.int64) - np.rint(y * 32767.0).astype(np.int64)) <= 1)


def test_mixed_formats_in_one_launch(gpu):
    fmts = [(R.NATIVE, R.F32), (8000, R.S16), (48000, R.S16)]
    outs, hist = run(gpu, signals(), SCHED, fmts)
    assert np.array_equal(outs[0].view(np.uint32), signals()[0].view(np.uint32))   # the native stream: the input bits
    assert np.array_equal(outs[1], single_format(gpu, fmts[1])[0][1])
    assert np.array_equal(outs[2], single_format(gpu, fmts[2])[0][2])
    core = hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].reshape(G, 2, R.HIST)
    assert not core[0].any()                                     # a native stream keeps no history


@pytest.mark.parametrize("what", ["chunk length", "no stream", "stream twice", "48000 f32"])
def test_launcher_refusals_write_nothing(gpu, what):
    x, fmts, slots, chunks = signals()[:, : 2 * R.FRAME], [(16000, R.S16)] * G, [[0, 1, 2]], [2 * R.FRAME]
    if what == "chunk length":
        chunks = [2 * R.FRAME - 920]
    elif what == "no stream":
        x, fmts, slots = x[:0], [], [[]]
    elif what == "stream twice":
        slots = [[0, 1, 0]]
    else:
        fmts = [(16000, R.S16), (48000, R.F32), (16000, R.S16)]
    with pytest.raises(gpu.Q3Error) as ei:
        gpu.op_pcm_convert(x, chunks, slots, 3, fmts, slack=8, fill=FILL)
    ex = ei.value
    assert "pcm convert" in str(ex) and len(ex.wholes) == len(fmts)
    assert all(np.all(w == FILL) for w in ex.wholes) and np.all(ex.n_out == -1)
    assert not ex.hist[gpu.GLUE_GUARD: -gpu.GLUE_GUARD].any() and np.all(ex.hist[: gpu.GLUE_GUARD] == np.float32(-3e38))
