"""Named cases shared by tests/test_frame_glue_ref_cpu.py and tests/test_gpu_frame_glue.py.  TEST INFRASTRUCTURE ONLY.

Every case is built from a seed, and each stands for one plausible kernel bug:

  projection   (n_in, n_out, ntok, x gap, out pad): one, two and four 512-input chunks (no prefetch / one prefetch / the engine's depth) with
               every token tail around the 16-row tile (1, 15, 16, 17, 33); an x gap of 3e38 that a fetch with the wrong stride reads; an out
               pad that a store with the wrong stride hits.  The CPU test holds that an fma chain differs from the mul-then-add chain on
               the inputs of every case, so a contracted kernel cannot pass
  table        rows around the 4-row workgroup (1, 3, 4, 5, 9), n_out 272 = a partial second 256-column block, n_in 64 and 2048
  codes        per table: 0, the last row, exactly rows[q] (first zero row: `<` against `<=`), far past it, negative (row 0, never an index)
  trail        f < n_trail, f == n_trail - 1 (last id), f == n_trail (first pad), n_trail == 0; ids inside the table, exactly text_rows,
               -1 (64-bit wrap), Q3_TEXT_EOS, 986800 (id*17 + i crosses 2^24 at i = 1616: the float stops being exact), INT32_MAX
  slots        finished; n_frames == max_frames; n_frames == max_frames - 1 (the last history row); code_0 either EOS id; ordinary
  gate         all 16 combinations of (finished, f < max, open, f >= n_trail) and one ordinary slot
"""
import functools
import itertools

import numpy as np

import frame_glue_ref as R

PROJECTION_CASES = (   # (n_in, n_out, ntok, x gap, out pad): every (n_in, ntok) pair, every n_out, gap and pad under every n_in
    (512, 16, 1, 0, 0), (512, 48, 15, 4, 3), (512, 1024, 16, 0, 3), (512, 16, 17, 4, 0), (512, 48, 33, 0, 0),
    (1024, 48, 1, 4, 3), (1024, 16, 15, 0, 0), (1024, 48, 16, 4, 0), (1024, 1024, 17, 0, 3), (1024, 16, 33, 4, 3),
    (2048, 1024, 1, 0, 0), (2048, 48, 15, 4, 3), (2048, 16, 16, 0, 3), (2048, 48, 17, 4, 0), (2048, 1024, 33, 4, 3),
)
TABLE_CASES = (        # (rows, n_out, n_in)
    (1, 16, 64), (3, 256, 2048), (4, 272, 64), (5, 1024, 2048), (9, 272, 2048), (9, 16, 64), (4, 256, 2048), (5, 272, 64), (1, 1024, 64),
)
CODEC_ROWS = (40,) + (24,) * 15      # unequal small tables
TEXT_ROWS = 32
IDS_STRIDE = 8
INT32_MAX = 2 ** 31 - 1
TRAIL_IDS = (5, 0, TEXT_ROWS - 1, TEXT_ROWS, -1, R.TEXT_EOS, 986800, INT32_MAX)
TRAIL_SHAPES = ((1, 4), (2, 3), (3, 3), (0, 0), (2, 0), (0, 1), (7, 8), (8, 8))   # (n_frames, n_trail): f <, f == n - 1, f ==, n == 0, ...
HI_WORDS = (0x007FFFFF, 0x80000000, 0xBFC00000, 0x3F800000, 0xFFFFFFFF, 0x00000000, 0x12345678)   # 0x007FFFFF = the armed key's
I32 = np.int32(0x5A5A5A5A)           # sentinels of the guarded buffers
U64 = np.uint64(0xA5C3F00D5A3C0FF1)
U32 = np.uint32(0xDEADBEEF)
F32 = np.float32(-7777.25)


def _rng(*key):
    return np.random.default_rng([0xF6A3E, *key])


@functools.lru_cache(maxsize=None)
def projection_inputs(n_in, n_out, seed=0):
    """x [33][n_in], W [n_out][n_in], b [n_out]: shared by every token count of the shape"""
    g = _rng(1, n_in, n_out, seed)
    x = (g.standard_normal((33, n_in)) * 1.7).astype(np.float32)
    W = (g.standard_normal((n_out, n_in)) * 0.9).astype(np.float32)
    b = g.standard_normal(n_out).astype(np.float32)
    for a in (x, W, b):
        a.setflags(write=False)
    return x, W, b


@functools.lru_cache(maxsize=None)
def projection_ref(n_in, n_out, seed=0):
    """(f32 chain, fma chain, float64 sum, magnitude) of all 33 rows, computed once"""
    x, W, b = projection_inputs(n_in, n_out, seed)
    out = R.project(x, W, b), R.project_fma(x, W, b), *R.project64(x, W, b)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def codec_tables(rows=CODEC_ROWS, row_len=2048, seed=0):
    g = _rng(2, row_len, seed)
    tabs = tuple((g.standard_normal((r, row_len)) * (1 + q % 3)).astype(np.float32) for q, r in enumerate(rows))
    for t in tabs:
        t.setflags(write=False)
    return tabs


@functools.lru_cache(maxsize=None)
def text_table():
    t = _rng(3).standard_normal((TEXT_ROWS, 2048)).astype(np.float32)
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def tts_pad():
    t = _rng(4).standard_normal(2048).astype(np.float32)
    t.setflags(write=False)
    return t


def code_edges(rows):
    return (0, rows - 1, rows, rows + 1, 100000, INT32_MAX, -1, -5, -2 ** 31)


def feedback_codes(ntok, rows=CODEC_ROWS):
    """[ntok][16]: token t < 9 holds edge t of every table; later tokens are inside the tables with one or two edges planted.  With ntok < 9
    the edges go on a diagonal instead, so that even one token meets every one of them"""
    g = _rng(5, ntok)
    c = np.stack([g.integers(0, r, ntok) for r in rows], axis=1).astype(np.int64)
    if ntok >= 9:
        for t in range(9):
            c[t] = [code_edges(r)[t] for r in rows]
        for t in range(9, ntok):
            q = t % 16
            c[t, q] = code_edges(rows[q])[(t // 16 + t) % 9]
    else:
        for t in range(ntok):
            for q in range(16):
                c[t, q] = code_edges(rows[q])[(q + 3 * t) % 9]
    return c.astype(np.int32)


def keys_of(codes, key_stride):
    """[ntok][key_stride] uint64: slot q < 16 = raw_key(some value word, code); the armed key wherever a code is 0 and the word cycle says so;
    slots from 16 on hold the sentinel"""
    codes = np.asarray(codes).reshape(codes.shape[0], -1)
    k = np.full((codes.shape[0], key_stride), U64, np.uint64)
    for t, q in itertools.product(range(codes.shape[0]), range(codes.shape[1])):
        k[t, q] = R.raw_key(HI_WORDS[(t * 5 + q) % len(HI_WORDS)], codes[t, q])
    return k


def trail_case(ntok):
    """n_frames, n_trail [ntok], ids [ntok][IDS_STRIDE]: token t takes shape t % 8 and, where it reads an id, id (t // 8 + t) % 8 of TRAIL_IDS
    at column n_frames; the other columns hold other in-table ids, so a cursor off by one reads a different row"""
    shapes = [TRAIL_SHAPES[(t + (1 if ntok == 1 else 0)) % len(TRAIL_SHAPES)] for t in range(ntok)]
    n_frames = np.array([s[0] for s in shapes], np.int32)
    n_trail = np.array([s[1] for s in shapes], np.int32)
    ids = np.zeros((ntok, IDS_STRIDE), np.int32)
    for t in range(ntok):
        ids[t] = [(7 * t + 3 * j + 1) % TEXT_ROWS for j in range(IDS_STRIDE)]
        if n_frames[t] < n_trail[t]:
            ids[t, n_frames[t]] = TRAIL_IDS[(t // 8 + t) % len(TRAIL_IDS)]
    return n_frames, n_trail, ids


# ------------------------------------------------------------ slot states ------------------------------------------------------------
MAX_FRAMES = 6
HIST_STRIDE = MAX_FRAMES * 16 + 8
SLOT_KINDS = ("ordinary", "finished", "at_max", "last_row", "codec_eos", "text_eos")


def fresh_keys(state, step, eos=()):
    """what a frame leaves behind before the advance: 16 new keys per slot (code_0 stays what the previous advance handed over, except at step 0)
    and the talker's next pick in next_key0; eos = {slot: id} plants an EOS id as the slot's current code_0"""
    g = _rng(6, len(state["finished"]), step)
    B = len(state["finished"])
    for b in range(B):
        for q in range(16):
            if q > 0 or step == 0:
                state["keys"][b, q] = R.raw_key(HI_WORDS[(b + q + step) % len(HI_WORDS)], int(g.integers(0, 2048)))
        if b in eos:
            state["keys"][b, 0] = R.raw_key(0x80000000, eos[b])
        state["next_key0"][b] = R.raw_key(HI_WORDS[(b + step) % len(HI_WORDS)], int(g.integers(0, 2048)))


def slot_state(B, kind0=0):
    """B slots, slot b of kind SLOT_KINDS[(b + kind0) % 6]; history rows not yet written and the 8 ints behind max_frames*16 hold the sentinel"""
    s = dict(finished=np.zeros(B, np.int32), n_frames=np.zeros(B, np.int32), max_frames=np.full(B, MAX_FRAMES, np.int32),
             t_slot=np.zeros(B, np.int32), t_pos=np.zeros((B, 4), np.int32), keys=np.full((B, 16), R.ARMED, np.uint64),
             next_key0=np.full(B, R.ARMED, np.uint64), hist=np.full((B, HIST_STRIDE), I32, np.int32))
    eos = {}
    for b in range(B):
        kind = SLOT_KINDS[(b + kind0) % 6]
        f = {"ordinary": b % 4, "finished": 2, "at_max": MAX_FRAMES, "last_row": MAX_FRAMES - 1, "codec_eos": 1, "text_eos": 3}[kind]
        s["n_frames"][b] = f
        s["finished"][b] = kind == "finished"
        s["t_slot"][b] = 10 + f + b
        s["t_pos"][b] = [20 + f, 30 + f, 40 + f, 50 + b]
        s["hist"][b, : f * 16] = np.arange(f * 16) + 1000 * (b + 1)
        if kind.endswith("_eos"):
            eos[b] = R.CODEC_EOS if kind == "codec_eos" else R.TEXT_EOS
    return s, eos


def gate_state():
    """17 slots: the 16 combinations of (finished, f < max, open, f >= n_trail) and an ordinary closed slot; only slot 0b0111 waits"""
    B = 17
    s, _ = slot_state(B)
    g = _rng(7)
    for b in range(16):
        fin, below, opn, past = b >> 3 & 1, b >> 2 & 1, b >> 1 & 1, b & 1
        f = 2 if below else MAX_FRAMES
        s["finished"][b], s["n_frames"][b] = fin, f
        s["hist"][b] = I32
        s["hist"][b, : f * 16] = np.arange(f * 16) + 1000 * (b + 1)
    s["finished"][16], s["n_frames"][16] = 0, 1
    s["open"] = np.array([b >> 1 & 1 for b in range(16)] + [0], np.int32)
    s["n_trail"] = np.array([s["n_frames"][b] - (b & 1) + (1 - (b & 1)) * 1 for b in range(16)] + [0], np.int32)   # past: n_trail <= f, else f + 1
    s["hidden"] = g.standard_normal((B, 2048)).astype(np.float32)
    s["save_hidden"] = g.standard_normal((B, 2048)).astype(np.float32)          # stale contents of earlier stalls
    s["draws"] = g.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
    s["pdraws"] = g.integers(0, 2 ** 32, B, dtype=np.uint64).astype(np.uint32)
    s["save_draws"] = g.integers(0, 2 ** 32, (B, 2), dtype=np.uint64).astype(np.uint32)
    fresh_keys(s, 0)
    return s
