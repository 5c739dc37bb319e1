"""The glue kernels between the GEMMs of a decode frame -- k_project_mt, k_project_table, k_feedback_keys<false/true>, k_gather_rows_keys,
k_advance_keys, k_stall_save, k_advance_keys_gated -- through q3tts_op_frame_glue: one launch per call through the launcher the engine
uses, every output and every piece of state in a guarded buffer that comes back whole.

Every comparison with tests/frame_glue_ref.py is bit-exact and covers the WHOLE buffer: guards, stride padding, rows past ntok and the
state of slot B hold their sentinel afterwards, so a stray write fails the same assertion as a wrong value.  The projection and feedback
results are also held against float64 within the recursive-summation bound gamma_m (|b| + sum |x_i w_i|), m = n_in + 1 and 17: derived, not
measured.  The cases and what each is for are listed in tests/frame_glue_cases.py; tests/test_frame_glue_ref_cpu.py checks the reference
and holds that every projection case tells mul-then-add from fma."""
import os

import numpy as np
import pytest

import frame_glue_cases as K
import frame_glue_ref as R

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what=""):
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not np.array_equal(_bits(got), _bits(want)):
        bad = np.flatnonzero(_bits(got).ravel() != _bits(want).ravel())
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %r, want %r"
                             % (what, bad.size, got.size, bad[0], got.ravel()[bad[0]], want.ravel()[bad[0]]))


# ------------------------------------------------------------ projection ------------------------------------------------------------
def _project_mt(gpu, x, W, b, ntok, gap=0, pad=0, x_off=0, out=None):
    """rows x[:ntok] at stride n_in + gap (gap columns 3e38) -> the whole guarded out buffer, 16 * ceil(ntok / 16) + 1 rows of n_out + pad"""
    n_out, n_in = W.shape
    xs = np.full((ntok, n_in + gap), 3e38, np.float32)
    xs[:, :n_in] = x[:ntok]
    rows = (ntok + 15) // 16 * 16 + 1
    out = out if out is not None else gpu.glue_guarded(np.full((rows, n_out + pad), K.F32), K.F32)
    gpu.op_frame_glue(gpu.GLUE_PROJECT_MT, ntok=ntok, n_in=n_in, n_out=n_out, x_stride=n_in + gap, x_off=x_off, out_stride=n_out + pad,
                      x=xs, w=W, b=b, out=out)
    return out


def _project_want(gpu, ref, ntok, n_out, pad):
    rows = (ntok + 15) // 16 * 16 + 1
    core = np.full((rows, n_out + pad), K.F32)
    core[:ntok, :n_out] = ref[:ntok]
    return gpu.glue_guarded(core, K.F32)


@pytest.mark.parametrize("case", K.PROJECTION_CASES, ids=lambda c: "in%d_out%d_tok%d_gap%d_pad%d" % c)
def test_project_mt(gpu, case):
    n_in, n_out, ntok, gap, pad = case
    x, W, b = K.projection_inputs(n_in, n_out)
    ref, _, d, mag = K.projection_ref(n_in, n_out)
    got = _project_mt(gpu, x, W, b, ntok, gap, pad)
    _same(got, _project_want(gpu, ref, ntok, n_out, pad), "k_project_mt %r" % (case,))
    core = gpu.glue_core(got, (-1, n_out + pad))[:ntok, :n_out]
    assert np.all(np.abs(core.astype(np.float64) - d[:ntok]) <= R.gamma(n_in + 1) * mag[:ntok])


def test_project_mt_at_an_aligned_offset_and_one_row_at_a_time(gpu):
    n_in, n_out = 1024, 48
    x, W, b = K.projection_inputs(n_in, n_out)
    ref = K.projection_ref(n_in, n_out)[0]
    _same(_project_mt(gpu, x, W, b, 17, gap=4, pad=3, x_off=4), _project_want(gpu, ref, 17, n_out, 3), "x_off = 4")
    for t in (0, 16, 32):     # a row's result does not depend on the rows that share its tile
        _same(_project_mt(gpu, x[t:t + 1], W, b, 1), _project_want(gpu, ref[t:t + 1], 1, n_out, 0), "row %d alone" % t)


@pytest.mark.parametrize("why, kw", [("n_in % 512", dict(n_in=768)), ("n_in % 512", dict(n_in=256)), ("x_stride % 4", dict(gap=2)),
                                     ("x_stride % 4", dict(gap=1)), ("misaligned x", dict(x_off=1)), ("misaligned x", dict(x_off=2)),
                                     ("misaligned x", dict(x_off=3)), ("n_out % 16", dict(n_out=24)), ("n_out % 16", dict(n_out=8))])
def test_project_mt_refusals_leave_the_outputs_alone(gpu, why, kw):
    n_in, n_out = kw.get("n_in", 512), kw.get("n_out", 16)
    g = np.random.default_rng(3)
    x, W, b = (g.standard_normal(s).astype(np.float32) for s in ((3, n_in), (n_out, n_in), (n_out,)))
    out = gpu.glue_guarded(np.full((17, n_out), K.F32), K.F32)
    with pytest.raises(gpu.Q3Error, match="k_project_mt"):
        _project_mt(gpu, x, W, b, 3, gap=kw.get("gap", 0), x_off=kw.get("x_off", 0), out=out)
    assert np.all(out == K.F32), why
    if n_in % 512 == 0 and n_out % 16 == 0:   # the same buffers with the offending stride / offset put right: accepted
        _same(_project_mt(gpu, x, W, b, 3, out=out), _project_want(gpu, R.project(x, W, b), 3, n_out, 0), why)


@pytest.mark.parametrize("n_in, n_out", [(2048, 24), (768, 16), (2048, 8), (256, 48)])
def test_op_project_refuses_what_k_project_mt_cannot_run(gpu, n_in, n_out):
    """q3tts_op_project runs k_project_mt: a width that is no multiple of 16 (whose blocked weight would not fill its last block) or an input
    length that is no multiple of 512 is refused by the launcher, and y stays as it was"""
    g = np.random.default_rng([5, n_in, n_out])
    x, W, b = (g.standard_normal(s).astype(np.float32) for s in ((n_in,), (n_out, n_in), (n_out,)))
    y = np.full(n_out, K.F32)
    with pytest.raises(gpu.Q3Error, match="k_project_mt"):
        gpu._chk(gpu.lib().q3tts_op_project(gpu._p(x), gpu._p(W), gpu._p(b), n_in, n_out, gpu._p(y)))
    assert np.all(y == K.F32)
    ok_in, ok_out = (n_in + 511) // 512 * 512, (n_out + 15) // 16 * 16       # the nearest shape it can run: accepted, and the chain's bits
    x, W, b = (g.standard_normal(s).astype(np.float32) for s in ((ok_in,), (ok_out, ok_in), (ok_out,)))
    _same(gpu.op_project(x, W, b), R.project(x[None], W, b)[0], "op_project %d -> %d" % (ok_in, ok_out))


@pytest.mark.parametrize("case", K.TABLE_CASES, ids=lambda c: "rows%d_out%d_in%d" % c)
def test_project_table(gpu, case):
    rows, n_out, n_in = case
    g = np.random.default_rng([21, *case])
    x, W, b = (g.standard_normal(s).astype(np.float32) for s in ((rows, n_in), (n_out, n_in), (n_out,)))
    out = gpu.glue_guarded(np.full((rows + 4, n_out), K.F32), K.F32)      # room for the whole last workgroup of 4 rows
    gpu.op_frame_glue(gpu.GLUE_PROJECT_TABLE, ntok=rows, n_in=n_in, n_out=n_out, x=x, w=W, b=b, out=out)
    ref = R.project(x, W, b)
    core = np.full((rows + 4, n_out), K.F32)
    core[:rows] = ref
    _same(out, gpu.glue_guarded(core, K.F32), "k_project_table %r" % (case,))
    d, mag = R.project64(x, W, b)
    assert np.all(np.abs(gpu.glue_core(out, (-1, n_out))[:rows].astype(np.float64) - d) <= R.gamma(n_in + 1) * mag)
    if n_in % 512 == 0:   # the engine relies on P_q[c] == project(E_q[c]): the load-time kernel and the per-frame kernel agree bit for bit
        mt = gpu.glue_core(_project_mt(gpu, x, W, b, rows), (-1, n_out))[:rows]
        _same(mt, gpu.glue_core(out, (-1, n_out))[:rows], "k_project_mt against k_project_table %r" % (case,))


# ------------------------------------------------------------ code consumers ------------------------------------------------------------
def _feedback(gpu, tables, codes, key_stride, pad, trail=None, text=None):
    """-> (whole out buffer [ntok + 1][2048], whole keys buffer, whole n_frames buffer or None)"""
    ntok = codes.shape[0]
    keys = gpu.glue_guarded(np.concatenate([K.keys_of(codes, key_stride), np.full((1, key_stride), K.U64)]), K.U64)
    out = gpu.glue_guarded(np.full((ntok + 1, 2048), K.F32), K.F32)
    kw, nf = {}, None
    if trail is not None:
        n_frames, n_trail, ids = trail
        nf = gpu.glue_guarded(np.concatenate([n_frames, [K.I32]]).astype(np.int32), K.I32)
        kw = dict(trail=1, n_frames=nf, n_trail=n_trail, trail_ids=ids, ids_stride=ids.shape[1], text_table=text)
    gpu.op_frame_glue(gpu.GLUE_FEEDBACK_KEYS, tables=tables, ntok=ntok, key_stride=key_stride, tts_pad=pad, keys=keys, out=out, **kw)
    return out, keys, nf


@pytest.mark.parametrize("trail", [False, True], ids=["pad", "trail"])
@pytest.mark.parametrize("key_stride", [16, 17])
@pytest.mark.parametrize("ntok", [1, 3, 65])
def test_feedback_keys(gpu, ntok, key_stride, trail):
    tables, pad, text = K.codec_tables(), K.tts_pad(), K.text_table()
    codes = K.feedback_codes(ntok)
    tr = K.trail_case(ntok) if trail else None
    last = R.last_rows(pad, ntok, tr[0], tr[1], tr[2], text) if trail else None
    ref, d, mag = R.feedback(tables, K.CODEC_ROWS, codes, pad, last)
    out, keys, nf = _feedback(gpu, tables, codes, key_stride, pad, tr, text)
    core = np.full((ntok + 1, 2048), K.F32)
    core[:ntok] = ref
    _same(out, gpu.glue_guarded(core, K.F32), "k_feedback_keys")
    assert np.all(np.abs(gpu.glue_core(out, (-1, 2048))[:ntok].astype(np.float64) - d) <= R.gamma(17) * mag)
    # the inputs the kernel shares with the rest of the frame are read only
    _same(keys, gpu.glue_guarded(np.concatenate([K.keys_of(codes, key_stride), np.full((1, key_stride), K.U64)]), K.U64), "keys")
    if trail:
        _same(nf, gpu.glue_guarded(np.concatenate([tr[0], [K.I32]]).astype(np.int32), K.I32), "n_frames")
        assert not np.array_equal(ref, R.feedback(tables, K.CODEC_ROWS, codes, pad)[0])


def test_feedback_keys_ignores_the_value_word(gpu):
    tables, pad = K.codec_tables(), K.tts_pad()
    codes = K.feedback_codes(3)
    want = _feedback(gpu, tables, codes, 16, pad)[0]
    keys = np.array([[R.raw_key(K.HI_WORDS[(t + 2 * q + 3) % len(K.HI_WORDS)], codes[t, q]) for q in range(16)] for t in range(3)], np.uint64)
    assert not np.array_equal(keys, K.keys_of(codes, 16))
    kb = gpu.glue_guarded(keys, K.U64)
    out = gpu.glue_guarded(np.full((4, 2048), K.F32), K.F32)
    gpu.op_frame_glue(gpu.GLUE_FEEDBACK_KEYS, tables=tables, ntok=3, key_stride=16, tts_pad=pad, keys=kb, out=out)
    _same(out, want, "other value words, same codes")


def test_feedback_keys_equals_feedback_rows_on_the_tiny_model(gpu, tiny_model):
    """ties the per-frame kernel to its tested resume twin (k_feedback_codes, test_feedback_rows_bit_exact) on the real tables"""
    import ggml_ref as G
    path = os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf")
    _, t = G.read_gguf(path)
    ten = lambda n: np.array(t[n][2]).view(np.float32).reshape(-1, 2048)
    tables = [ten("codec_embd.%d" % q) for q in range(16)]
    a = gpu.Assets(path)
    try:
        pad = a.tts_pad()
        rng = np.random.default_rng(31)
        n = 5
        codes = rng.integers(0, 2048, (n, 16)).astype(np.int32)
        codes[0, 15], codes[1, 0], codes[2, 7], codes[2, 9], codes[3, 0] = 2047, 2159, 2048, -3, tables[0].shape[0]
        _same(gpu.glue_core(_feedback(gpu, tables, codes, 16, pad)[0], (-1, 2048))[:n], gpu.op_feedback_rows(a, codes), "no trail")
        trail = np.array([7, R.TEXT_EOS, 4095, 4096], np.int32)          # row 4 is past the trail: tts_pad
        ids = np.zeros((n, 6), np.int32)
        ids[:, :4] = trail
        tr = (np.arange(n, dtype=np.int32), np.full(n, 4, np.int32), ids)  # slot f stands at frame f of the same trail
        got = _feedback(gpu, tables, codes, 16, pad, tr, ten("text_embd"))[0]
        _same(gpu.glue_core(got, (-1, 2048))[:n], gpu.op_feedback_rows(a, codes, trail), "trail")
    finally:
        a.close()


def _gather(gpu, table, codes, row_len):
    ntok = len(codes)
    keys = gpu.glue_guarded(np.concatenate([K.keys_of(np.asarray(codes).reshape(-1, 1), 16), np.full((1, 16), K.U64)]), K.U64)
    out = gpu.glue_guarded(np.full((ntok + 1, row_len), K.F32), K.F32)
    gpu.op_frame_glue(gpu.GLUE_GATHER_ROWS_KEYS, tables=[table], ntok=ntok, key_stride=16, row_len=row_len, keys=keys, out=out)
    core = np.full((ntok + 1, row_len), K.F32)
    core[:ntok] = R.gather(table, table.shape[0], codes, row_len)
    _same(out, gpu.glue_guarded(core, K.F32), "k_gather_rows_keys row_len %d ntok %d" % (row_len, ntok))


@pytest.mark.parametrize("ntok", [1, 65])
@pytest.mark.parametrize("row_len", [16, 256, 260, 1024])
def test_gather_rows_keys(gpu, row_len, ntok):
    table = K.codec_tables((24,), row_len)[0]
    edges = K.code_edges(24)
    for first in range(len(edges) if ntok == 1 else 1):     # one token: every edge in turn
        _gather(gpu, table, [edges[(first + t) % len(edges)] if t < 18 else (7 * t) % 24 for t in range(ntok)], row_len)


def test_gather_rows_keys_minus_one(gpu):
    """-1 alone: the smallest negative code, one row in front of the table when the clamp is missing"""
    table = K.codec_tables((24,), 260)[0]
    _gather(gpu, table, [3, -1, 23, -1, 0], 260)


# ------------------------------------------------------------ slot state machine ------------------------------------------------------------
_STATE = (("keys", K.U64), ("next_key0", K.U64), ("finished", K.I32), ("n_frames", K.I32), ("t_slot", K.I32), ("t_pos", K.I32), ("hist", K.I32))
_GATE = (("hidden", K.F32), ("save_hidden", K.F32), ("draws", K.U32), ("pdraws", K.U32), ("save_draws", K.U32))


def _pack(gpu, s):
    """the guarded buffers of a state: B slots and the sentinel state of slot B"""
    ext = lambda a, sent: gpu.glue_guarded(np.concatenate([a, np.full((1,) + a.shape[1:], sent, a.dtype)]), sent)
    return {k: ext(s[k], sent) for k, sent in _STATE + (_GATE if "hidden" in s else ())}


def _unpack(gpu, s, bufs):
    out = {k: np.array(v, copy=True) for k, v in s.items()}
    for k, v in bufs.items():
        out[k] = np.array(gpu.glue_core(v).reshape((-1,) + s[k].shape[1:])[: len(s["finished"])], copy=True)
    return out


def _run(gpu, kernel, s):
    """one launch on state s -> (the state after it, the whole buffers)"""
    bufs = _pack(gpu, s)
    kw = dict(open=s["open"], n_trail=s["n_trail"]) if "hidden" in s else {}
    gpu.op_frame_glue(kernel, ntok=len(s["finished"]), max_frames=s["max_frames"], hist_stride=s["hist"].shape[1], **kw, **bufs)
    return _unpack(gpu, s, bufs), bufs


def _same_state(gpu, bufs, want, what):
    for k, v in _pack(gpu, want).items():
        _same(bufs[k], v, "%s: %s" % (what, k))


def _advance_steps(gpu, B, kind0=0):
    s, eos = K.slot_state(B, kind0)
    for step in range(5):
        late = {b: R.CODEC_EOS if b % 2 else R.TEXT_EOS for b in range(B) if b % 6 == 0 and b % 5 == step}   # ordinary slots that end later
        K.fresh_keys(s, step, eos if step == 0 else late)
        got, bufs = _run(gpu, gpu.GLUE_ADVANCE_KEYS, s)
        _same_state(gpu, bufs, R.advance(s), "k_advance_keys B %d kind0 %d step %d" % (B, kind0, step))
        s = got
    return s


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
def test_advance_keys(gpu, B):
    for kind0 in range(6 if B == 1 else 1):      # the single slot is of every kind in turn
        s = _advance_steps(gpu, B, kind0)
    if B >= 6:
        assert np.any(s["n_frames"] == K.MAX_FRAMES) and np.any(s["finished"] == 1) and np.all(s["n_frames"] <= K.MAX_FRAMES)
        assert np.all(s["hist"][:, K.MAX_FRAMES * 16:] == K.I32) and np.all(s["t_pos"][:, 3] == 50 + np.arange(B))


def test_stall_save_and_gated_advance(gpu):
    s0 = K.gate_state()
    B = len(s0["finished"])
    waiting = [b for b in range(B) if R.waits(s0, b)]
    assert waiting == [7]
    s1, bufs = _run(gpu, gpu.GLUE_STALL_SAVE, s0)
    _same_state(gpu, bufs, R.stall_save(s0), "k_stall_save")
    for b in range(B):        # the save area of waiting slots only; nothing else at all
        assert np.array_equal(s1["save_hidden"][b], s0["hidden"][b] if b in waiting else s0["save_hidden"][b])
    # the discarded frame: hidden rows, draw counters and keys are overwritten for every slot
    g = np.random.default_rng(41)
    s1["hidden"] = g.standard_normal((B, 2048)).astype(np.float32)
    s1["draws"] = s1["draws"] + np.uint32(1)
    s1["pdraws"] = s1["pdraws"] + np.uint32(15)
    K.fresh_keys(s1, 1)
    s2, bufs = _run(gpu, gpu.GLUE_ADVANCE_KEYS_GATED, s1)
    _same_state(gpu, bufs, R.advance_gated(s1), "k_advance_keys_gated")
    plain, _ = _run(gpu, gpu.GLUE_ADVANCE_KEYS, {k: v for k, v in s1.items() if k not in dict(_GATE) and k not in ("open", "n_trail")})
    for b in range(B):
        if b in waiting:
            assert np.array_equal(s2["hidden"][b], s0["hidden"][b]) and s2["draws"][b] == s0["draws"][b] and s2["pdraws"][b] == s0["pdraws"][b]
            assert s2["keys"][b, 0] == s1["keys"][b, 0] and np.all(s2["keys"][b, 1:] == R.ARMED) and s2["next_key0"][b] == R.ARMED
            for k in ("n_frames", "finished", "hist", "t_slot", "t_pos"):
                assert np.array_equal(s2[k][b], s1[k][b]), k
        else:                 # exactly the plain advance, and the overwritten hidden / draws stay: the stale save area is not copied
            for k, _ in _STATE:
                assert np.array_equal(s2[k][b], plain[k][b]), (k, b)
            assert np.array_equal(s2["hidden"][b], s1["hidden"][b]) and s2["draws"][b] == s1["draws"][b] and s2["pdraws"][b] == s1["pdraws"][b]
    # the slot stays stalled for a second frame (nothing moved), then its id arrives and it runs
    s3, bufs = _run(gpu, gpu.GLUE_STALL_SAVE, s2)
    _same_state(gpu, bufs, R.stall_save(s2), "k_stall_save, second frame")
    s3["n_trail"][7] = s3["n_frames"][7] + 1
    assert not R.waits(s3, 7)
    K.fresh_keys(s3, 2)
    s4, bufs = _run(gpu, gpu.GLUE_ADVANCE_KEYS_GATED, s3)
    _same_state(gpu, bufs, R.advance_gated(s3), "k_advance_keys_gated, after the append")
    assert s4["n_frames"][7] == s3["n_frames"][7] + 1
