"""Plain numpy / Python restatements of the glue kernels between the GEMMs of a decode frame, the yardstick of tests/test_gpu_frame_glue.py.
TEST INFRASTRUCTURE ONLY.  Nothing here shares code with the kernels; the only thing taken from the package is argmax_key, and only to
build input keys (tests/test_frame_glue_ref_cpu.py holds the bit layout written out below against it).

  project        out[t][o] = b[o] + sum_i x[t][i] * W[o][i]: the product rounded to f32, then added in f32, i ascending (the reference's
                 assets_manager.rs:383-399; never an fma).  project64 is the same sum in float64 with its magnitude |b| + sum |x w|
  feedback       (sum_q E_q[code_q], q = 0..15 in order from 0) + last, f32 left to right (q3tts_spec.h "resume: prefill").  A negative
                 code reads row 0, a code >= rows[q] the zero row.  last = text(ids[f]) while f = n_frames < n_trail, tts_pad otherwise
  text_row       a table row, or HostAssets::text_embedding's row for any other id: fmod((float)((u64)id * 17 + i), 2) - 1
  gather         one table, the same two rules for a code outside it
  advance        kernels.h AdvanceKeysArgs: a slot is live when !finished && n_frames < max_frames.  A live slot whose code_0 is Q3_CODEC_EOS
                 or Q3_TEXT_EOS becomes finished and nothing else; any other live slot appends its 16 codes at history row n_frames, then
                 n_frames and t_slot step by one and so do position streams 0..2 (stream 3 stays).  Every slot, live or not, then takes
                 keys[0] = next_key0 and gets next_key0 and keys 1..15 re-armed
  waits          q3tts_spec.h "live text append": !finished && n_frames < max_frames && open && n_frames >= n_trail
  stall_save     a waiting slot's hidden row and (draws, pdraws) go to the save area; nothing else changes
  advance_gated  a waiting slot gets them back, keeps keys[0], has keys 1..15 and next_key0 re-armed and nothing else touched; every other
                 slot takes the plain advance

A state is a dict of plain numpy arrays over B slots: finished, n_frames, max_frames, t_slot [B], t_pos [B][4], keys [B][16] uint64,
next_key0 [B] uint64, hist [B][hist_stride]; the gated forms add open, n_trail [B], hidden, save_hidden [B][2048], draws, pdraws [B],
save_draws [B][2].  The functions return a changed deep copy.
"""
import copy
import math

import numpy as np

CODEC_EOS, TEXT_EOS = 2150, 151673           # include/q3tts_spec.h Q3_CODEC_EOS, Q3_TEXT_EOS
ARMED = 0x007FFFFFFFFFFFFF                   # pack_key(-inf, 0): value word ~0xFF800000, index word ~0
U = 2.0 ** -24                               # unit roundoff of f32


def key_code(k):
    """the code of an argmax key: the complement of its low word, as a signed 32-bit integer"""
    c = ~int(k) & 0xFFFFFFFF
    return c - (1 << 32) if c & 0x80000000 else c


def make_key(v, code):
    """the key the library packs for logit v at index code"""
    import q3tts
    return q3tts.argmax_key(float(v), int(code))


def pack_key(v, idx):
    """kdev.h pack_key written out: the value word orders floats as unsigned integers (-0.0 first folded onto +0.0; a negative value
    complemented, any other with the sign bit set), the index word is ~idx"""
    b = int(np.array([v], np.float32).view(np.uint32)[0])
    if b == 0x80000000:
        b = 0
    hi = (~b & 0xFFFFFFFF) if b & 0x80000000 else (b | 0x80000000)
    return (hi << 32) | (~int(idx) & 0xFFFFFFFF)


def raw_key(hi, code):
    """a key with any value word: the kernels here must read nothing but the low word"""
    return ((int(hi) & 0xFFFFFFFF) << 32) | (~int(code) & 0xFFFFFFFF)


def gamma(m):
    """the recursive-summation constant: m u / (1 - m u)"""
    return m * U / (1.0 - m * U)


# ------------------------------------------------------------ projection ------------------------------------------------------------
def project(x, W, b):
    x, W, b = np.asarray(x, np.float32), np.asarray(W, np.float32), np.asarray(b, np.float32)
    s = np.tile(b, (x.shape[0], 1))
    for i in range(W.shape[1]):
        t = x[:, i, None] * W[None, :, i]     # f32 * f32 -> f32: one rounding
        s = s + t                             # f32 + f32 -> f32: one rounding
    assert s.dtype == np.float32
    return s


def project_fma(x, W, b):
    """what a contracted kernel would compute: s = round_f32(s + x w) with the product exact (it is exact in float64: 24 + 24 bits)"""
    x, W = np.asarray(x, np.float32).astype(np.float64), np.asarray(W, np.float32).astype(np.float64)
    s = np.tile(np.asarray(b, np.float32), (x.shape[0], 1))
    for i in range(W.shape[1]):
        s = (s.astype(np.float64) + x[:, i, None] * W[None, :, i]).astype(np.float32)
    return s


def project64(x, W, b):
    """(float64 result, magnitude |b| + sum |x_i w_i|)"""
    x, W, b = (np.asarray(a, np.float32).astype(np.float64) for a in (x, W, b))
    return b[None, :] + x @ W.T, np.abs(b)[None, :] + np.abs(x) @ np.abs(W).T


# ------------------------------------------------------------ code consumers ------------------------------------------------------------
def _u64_to_f32(v):
    """(float)v for 0 <= v < 2^64, round to nearest even, as an exact Python float"""
    n = v.bit_length()
    if n <= 24:
        return float(v)
    sh = n - 24
    q, r = divmod(v, 1 << sh)
    half = 1 << (sh - 1)
    if r > half or (r == half and q & 1):
        q += 1
    return math.ldexp(float(q), sh)


def fallback_row(tok, n=2048):
    """HostAssets::text_embedding for an id outside the table (csrc/host_logic.cpp): the id goes to int64, then to u64, times 17 plus i with
    64-bit wrap, to float, fmod 2, minus 1"""
    base = int(tok) % (1 << 64)
    return np.array([math.fmod(_u64_to_f32((base * 17 + i) % (1 << 64)), 2.0) - 1.0 for i in range(n)], np.float32)


def text_row(text_table, tok):
    return np.asarray(text_table[int(tok)], np.float32) if 0 <= int(tok) < len(text_table) else fallback_row(tok)


def code_row(table, rows, code, row_len):
    c = max(int(code), 0)
    return np.asarray(table[c], np.float32)[:row_len] if c < rows else np.zeros(row_len, np.float32)


def last_rows(pad, ntok, n_frames=None, n_trail=None, ids=None, text_table=None):
    """the last addend of every token: tts_pad, or with a trail text(ids[t][f]) while f = n_frames[t] < n_trail[t]"""
    out = []
    for t in range(ntok):
        if n_frames is not None and int(n_frames[t]) < int(n_trail[t]):
            out.append(text_row(text_table, ids[t][int(n_frames[t])]))
        else:
            out.append(np.asarray(pad, np.float32))
    return out


def feedback(tables, rows, codes, pad, last=None):
    """rows [ntok][2048] in f32; also (float64 sum, magnitude sum |addend|).  last = last_rows(...) or None for tts_pad everywhere"""
    codes = np.asarray(codes).reshape(-1, 16)
    last = last if last is not None else last_rows(pad, codes.shape[0])
    out = np.zeros((codes.shape[0], 2048), np.float32)
    d = np.zeros((codes.shape[0], 2048), np.float64)
    mag = np.zeros((codes.shape[0], 2048), np.float64)
    for t in range(codes.shape[0]):
        acc = np.zeros(2048, np.float32)
        for q in range(16):
            v = code_row(tables[q], rows[q], codes[t, q], 2048)
            acc = acc + v
            d[t] += v
            mag[t] += np.abs(v)
        acc = acc + last[t]
        assert acc.dtype == np.float32
        out[t] = acc
        d[t] += last[t]
        mag[t] += np.abs(last[t])
    return out, d, mag


def gather(table, rows, codes, row_len):
    return np.stack([code_row(table, rows, c, row_len) for c in codes])


# ------------------------------------------------------------ slot state machine ------------------------------------------------------------
def _advance_slot(s, b):
    live = (not s["finished"][b]) and s["n_frames"][b] < s["max_frames"][b]
    if live:
        codes = [key_code(k) for k in s["keys"][b]]
        if codes[0] in (CODEC_EOS, TEXT_EOS):
            s["finished"][b] = 1
        else:
            f = int(s["n_frames"][b])
            s["hist"][b, f * 16: f * 16 + 16] = codes
            s["n_frames"][b] += 1
            s["t_slot"][b] += 1
            s["t_pos"][b, :3] += 1
    s["keys"][b, 0] = s["next_key0"][b]
    s["next_key0"][b] = ARMED
    s["keys"][b, 1:] = ARMED


def advance(state):
    s = copy.deepcopy(state)
    for b in range(len(s["finished"])):
        _advance_slot(s, b)
    return s


def waits(s, b):
    f = s["n_frames"][b]
    return bool((not s["finished"][b]) and f < s["max_frames"][b] and s["open"][b] and f >= s["n_trail"][b])


def stall_save(state):
    s = copy.deepcopy(state)
    for b in range(len(s["finished"])):
        if waits(s, b):
            s["save_hidden"][b] = s["hidden"][b]
            s["save_draws"][b] = (s["draws"][b], s["pdraws"][b])
    return s


def advance_gated(state):
    s = copy.deepcopy(state)
    for b in range(len(s["finished"])):
        if waits(s, b):
            s["hidden"][b] = s["save_hidden"][b]
            s["draws"][b], s["pdraws"][b] = s["save_draws"][b]
            s["next_key0"][b] = ARMED
            s["keys"][b, 1:] = ARMED
        else:
            _advance_slot(s, b)
    return s
