"""Every non-GEMM codec kernel (csrc/codec.hip), launched through q3tts_op_codec_kernel exactly as decode_group_async launches it, against a
float64 reference element by element (tests/codec_ops_ref.py): tiny and full decoder widths, groups of 1 / 5 / 16 streams with mixed cache
lengths and positions, RoPE positions up to the per-stream frame limit, stores outside the logical output.  Then two decoder-level checks:
a stream imported just below RoPE position 8192 decoded across it against the oracle, and staggered group joins past window saturation.  (-m gpu)"""
import os

import numpy as np
import pytest

import codec_ops_ref as R

pytestmark = pytest.mark.gpu

SENT = 0x7FA5A5A5   # a NaN bit pattern no kernel computes
LIMIT = 65536       # Q3TTS_CODEC_MAX_FRAMES


def _sent(n):
    return np.full(n, SENT, np.uint32).view(np.float32)


def _untouched(buf, written):
    """no float outside the `written` indices changed from the sentinel"""
    keep = np.ones(buf.size, bool)
    keep[np.asarray(written).ravel()] = False
    bad = np.flatnonzero(keep & (buf.view(np.uint32) != SENT))
    assert bad.size == 0, "%d floats written outside the logical output, first at %s" % (bad.size, bad[:8])


def _rows_idx(rows, C):
    return (np.asarray(rows)[:, None] * C + np.arange(C)[None, :]).ravel()


def _check(got, ref, bar, what):
    got = np.asarray(got, np.float64)
    err = np.abs(got - ref)
    assert np.isfinite(got).all(), what + ": non-finite output"
    i = np.unravel_index(np.argmax(err / bar), err.shape)
    assert np.all(err <= bar), "%s at %s: |err| %.3g > bar %.3g (got %r ref %r)" % (what, i, err[i], bar[i], got[i], ref[i])
    print("%s: max |err| / bar %.3g, max |err| %.3g" % (what, (err / bar).max(), err.max()))


def _meta(G, slots=None, kv=None, seen=None):
    m = np.zeros(3 * G, np.int64)
    m[:G] = np.arange(G) if slots is None else slots
    if kv is not None:
        m[G:2 * G] = kv
    if seen is not None:
        m[2 * G:] = seen
    return m


# ---------------- RVQ sum ----------------
@pytest.mark.parametrize("G,T,C,cb_size", [(1, 1, 32, 2048), (5, 4, 32, 2048), (16, 4, 512, 64), (3, 7, 512, 2048)])
def test_rvq_sum(gpu, G, T, C, cb_size):
    rng = np.random.default_rng(G * 100 + T + C)
    n_q, H = 16, 2
    cb = rng.standard_normal((n_q, cb_size, C)).astype(np.float32)
    codes = rng.integers(0, cb_size, (G * T, n_q))
    edge = np.array([-1, -7, cb_size, cb_size + 5, 2 ** 40, -2 ** 40, 0, cb_size - 1])
    codes.ravel()[: min(codes.size, 3 * len(edge))] = np.resize(edge, min(codes.size, 3 * len(edge)))
    out, = gpu.op_codec_kernel("RVQ_SUM", G, T, C, H, ins=[cb], outs=[_sent(G * (H + T) * C)], codes=codes, n_q=n_q, cb_size=cb_size)
    rows = R.ext_rows(G, T, H)
    _untouched(out, _rows_idx(rows, C))
    got = out.reshape(-1, C)[rows]
    ref, mag = R.rvq_sum(codes, cb)
    _check(got, ref, R.rvq_bar(n_q, mag), "RVQ_SUM")
    # the kernel adds the 16 rows in codebook order in f32: equal to that sum bit for bit
    c = np.clip(codes, 0, cb_size - 1)
    acc = np.zeros((G * T, C), np.float32)
    for q in range(n_q):
        acc = acc + cb[q][c[:, q]]
    assert np.array_equal(got, acc)


# ---------------- norms ----------------
def _norm_rows(rng, Rn, C):
    x = rng.standard_normal((Rn, C)) * np.exp2(rng.integers(-12, 12, Rn))[:, None]
    x[0] = 1e3 + rng.standard_normal(C) * 1e-2            # large mean, small spread
    x[-1] = -7.5e2 + rng.uniform(-1, 1, C) * 3e-3
    return x.astype(np.float32)


@pytest.mark.parametrize("G,T,C", [(1, 1, 64), (5, 4, 64), (16, 8, 1024), (3, 5, 1000)])
def test_rmsnorm_rows(gpu, G, T, C):
    rng = np.random.default_rng(C + G)
    x = _norm_rows(rng, G * T, C)
    g = rng.uniform(-2, 2, C).astype(np.float32)
    n = G * T * C
    out, = gpu.op_codec_kernel("RMSNORM_ROWS", G, T, C, ins=[x], outs=[_sent(n + 16)], p0=g, eps=1e-5)
    _untouched(out, np.arange(n))
    _check(out[:n].reshape(-1, C), R.rmsnorm(x, g, 1e-5), R.rmsnorm_bar(x, g, 1e-5), "RMSNORM_ROWS")


@pytest.mark.parametrize("G,T,C", [(1, 1, 64), (5, 4, 64), (4, 16, 1024), (3, 5, 1000)])
def test_layernorm_rows(gpu, G, T, C):
    rng = np.random.default_rng(C * 3 + G)
    x = _norm_rows(rng, G * T, C)
    w = rng.uniform(-2, 2, C).astype(np.float32)
    b = rng.uniform(-1, 1, C).astype(np.float32)
    n = G * T * C
    out, = gpu.op_codec_kernel("LAYERNORM_ROWS", G, T, C, ins=[x], outs=[_sent(n + 16)], p0=w, p1=b, eps=1e-6)
    _untouched(out, np.arange(n))
    _check(out[:n].reshape(-1, C), R.layernorm(x, w, b, 1e-6), R.layernorm_bar(x, w, b, 1e-6), "LAYERNORM_ROWS")
    # in place (the decoder's use): in = NULL, x uploaded as the output buffer; the same values bit for bit
    buf = np.concatenate([x.ravel(), _sent(16)])
    ip, = gpu.op_codec_kernel("LAYERNORM_ROWS", G, T, C, ins=[None], outs=[buf], p0=w, p1=b, eps=1e-6)
    assert np.array_equal(ip.view(np.uint32), out.view(np.uint32))


# ---------------- RoPE + K / V append ----------------
ROPE_CASES = [  # (n_heads, hd, W, G, T, frames seen per stream)
    (2, 32, 8, 1, 1, [0]),
    (2, 32, 8, 5, 4, [0, 8188, 8189, 8191, LIMIT - 4]),
    (16, 64, 72, 1, 4, [8190]),
    (16, 64, 72, 16, 4, [0, 1, 7, 8188, 8189, 8190, 8191, 8192, 12345, 30000, 40000, 50001, 65000, LIMIT - 6, LIMIT - 5, LIMIT - 4]),
    (3, 30, 12, 3, 2, [5, 8191, LIMIT - 2]),
]


@pytest.mark.parametrize("case", ROPE_CASES, ids=lambda c: "h%d-hd%d-G%d-T%d" % (c[0], c[1], c[3], c[4]))
def test_rope_append(gpu, case):
    nh, hd, W, G, T, seen = case
    C, H = nh * hd, W - 1
    rng = np.random.default_rng(hd * 7 + G)
    qkv = (rng.standard_normal((G * T, 3 * C)) * 2).astype(np.float32)
    ext = G * (H + T) * C
    meta = _meta(G, kv=rng.integers(0, W, G), seen=seen)
    q_out, k_ext, v_ext = gpu.op_codec_kernel("ROPE_APPEND", G, T, C, H, outs=[qkv, _sent(ext), _sent(ext)], meta=meta, n_heads=nh,
                                              head_dim=hd, window=W, rope_base=10000.0)
    pos = np.repeat(np.asarray(seen, np.int64), T) + np.tile(np.arange(T), G)
    assert pos.max() == max(seen) + T - 1
    q_out = q_out.reshape(G * T, 3 * C)
    for part, name in ((0, "q"), (1, "k")):
        ref, mag = R.rope(qkv[:, part * C:(part + 1) * C], pos, nh, hd, 10000.0)
        _check(q_out[:, part * C:(part + 1) * C], ref, R.rope_bar(ref, mag), "ROPE " + name)
    assert np.array_equal(q_out[:, 2 * C:].view(np.uint32), qkv[:, 2 * C:].view(np.uint32))      # V untouched in qkv
    rows = R.ext_rows(G, T, H)
    for buf in (k_ext, v_ext):
        _untouched(buf, _rows_idx(rows, C))
    assert np.array_equal(k_ext.reshape(-1, C)[rows].view(np.uint32), q_out[:, C:2 * C].view(np.uint32))
    assert np.array_equal(v_ext.reshape(-1, C)[rows].view(np.uint32), qkv[:, 2 * C:].view(np.uint32))


def test_rope_refuses_positions_past_the_limit(gpu):
    nh, hd, W, G, T = 2, 32, 8, 3, 4
    C, H = nh * hd, W - 1
    qkv = np.ones((G * T, 3 * C), np.float32)
    ext = G * (H + T) * C
    kw = dict(n_heads=nh, head_dim=hd, window=W)
    gpu.op_codec_kernel("ROPE_APPEND", G, T, C, H, outs=[qkv, _sent(ext), _sent(ext)], meta=_meta(G, seen=[0, 9, LIMIT - T]), **kw)
    for bad in ([0, LIMIT - T + 1, 0], [0, 0, LIMIT], [-1, 0, 0]):
        with pytest.raises(gpu.Q3Error, match="Q3TTS_CODEC_MAX_FRAMES"):
            gpu.op_codec_kernel("ROPE_APPEND", G, T, C, H, outs=[qkv, _sent(ext), _sent(ext)], meta=_meta(G, seen=bad), **kw)


# ---------------- sliding-window attention ----------------
ATTN_CASES = [  # (n_heads, hd, W, G, T, kv_len per stream)
    (2, 32, 8, 1, 1, [0]),
    (2, 32, 8, 1, 4, [7]),
    (2, 32, 8, 5, 4, [0, 1, 3, 7, 5]),
    (2, 32, 8, 5, 1, [7, 0, 7, 1, 6]),
    (2, 32, 8, 3, 11, [2, 7, 0]),                       # T0 > W: the window slides inside the call
    (16, 64, 72, 1, 4, [71]),
    (16, 64, 72, 16, 4, [0, 1, 2, 13, 35, 36, 60, 67, 68, 69, 70, 71, 71, 0, 71, 40]),
    (16, 64, 72, 5, 1, [71, 0, 1, 70, 33]),
    (3, 30, 12, 5, 3, [0, 11, 4, 10, 1]),               # hd % 4 != 0: the scalar K loads
    (1, 128, 128, 2, 2, [127, 3]),                      # the LDS limits
]


def _attn_problem(rng, nh, hd, W, G, T, kv):
    C, H = nh * hd, W - 1
    qkv = rng.standard_normal((G * T, 3 * C)).astype(np.float32)
    qkv[:, :C] *= 2.0
    Kx = rng.standard_normal((G, H + T, C)).astype(np.float32)
    Vx = rng.standard_normal((G, H + T, C)).astype(np.float32)
    for g in range(G):                                  # history rows before the valid ones hold NaN: reading one shows
        Kx[g, :H - kv[g]] = np.nan
        Vx[g, :H - kv[g]] = np.nan
    Kx[:, H:] = qkv[:, C:2 * C].reshape(G, T, C)         # the new rows are the call's own keys / values (as ROPE_APPEND leaves them)
    Vx[:, H:] = qkv[:, 2 * C:].reshape(G, T, C)
    return qkv, Kx, Vx


@pytest.mark.parametrize("case", ATTN_CASES, ids=lambda c: "h%d-hd%d-W%d-G%d-T%d" % c[:5])
def test_window_attention(gpu, case):
    nh, hd, W, G, T, kv = case
    C, H = nh * hd, W - 1
    rng = np.random.default_rng(hd + W * 3 + G * 5 + T)
    qkv, Kx, Vx = _attn_problem(rng, nh, hd, W, G, T, kv)
    n = G * T * C
    out, = gpu.op_codec_kernel("WINDOW_ATTN", G, T, C, H, ins=[qkv, Kx, Vx], outs=[_sent(n + 8)], meta=_meta(G, kv=kv), n_heads=nh,
                               head_dim=hd, window=W)
    _untouched(out, np.arange(n))
    ref, pv, info = R.window_attn(qkv[:, :C], Kx, Vx, kv, G, T, W, nh, hd)
    _check(out[:n].reshape(-1, C), ref, R.attn_bar(info, hd, T, pv), "WINDOW_ATTN")


def test_window_attention_refusals(gpu):
    rng = np.random.default_rng(3)
    for nh, hd, W, kv, what in ((1, 130, 8, [0], "head_dim"), (1, 32, 129, [0], "window"), (2, 32, 8, [8], "kv_len"), (2, 32, 8, [-1], "kv_len")):
        C, H = nh * hd, W - 1
        qkv = rng.standard_normal((1, 3 * C)).astype(np.float32)
        ext = np.zeros((H + 1) * C, np.float32)
        with pytest.raises(gpu.Q3Error, match=what):
            gpu.op_codec_kernel("WINDOW_ATTN", 1, 1, C, H, ins=[qkv, ext, ext], outs=[_sent(C)], meta=_meta(1, kv=kv), n_heads=nh, head_dim=hd, window=W)


# ---------------- SwiGLU, depthwise conv ----------------
@pytest.mark.parametrize("G,T,ff", [(1, 1, 128), (5, 4, 128), (16, 4, 3072)])
def test_swiglu_rows(gpu, G, T, ff):
    rng = np.random.default_rng(ff + G)
    gu = (rng.standard_normal((G * T, 2 * ff)) * 3).astype(np.float32)
    gu[0, :4] = [-100.0, 100.0, -20.0, 0.0]
    n = G * T * ff
    out, = gpu.op_codec_kernel("SWIGLU_ROWS", G, T, ff, ins=[gu], outs=[_sent(n + 8)])
    _untouched(out, np.arange(n))
    ref = R.swiglu(gu, ff)
    _check(out[:n].reshape(-1, ff), ref, R.swiglu_bar(ref), "SWIGLU_ROWS")


@pytest.mark.parametrize("G,T,C", [(1, 1, 64), (5, 4, 64), (16, 8, 1024), (3, 16, 1000)])
def test_dwconv7(gpu, G, T, C):
    rng = np.random.default_rng(C + T)
    xe = rng.standard_normal((G, 6 + T, C)).astype(np.float32)
    w = rng.standard_normal((C, 7)).astype(np.float32)
    b = rng.standard_normal(C).astype(np.float32)
    n = G * T * C
    out, = gpu.op_codec_kernel("DWCONV7", G, T, C, 6, ins=[xe], outs=[_sent(n + 8)], p0=w, p1=b)
    _untouched(out, np.arange(n))
    ref, mag = R.dwconv7(xe, w, b, G, T)
    _check(out[:n].reshape(-1, C), ref, R.dwconv_bar(mag), "DWCONV7")


# ---------------- SnakeBeta ----------------
@pytest.mark.parametrize("G,T,C,H", [(1, 1, 16, 6), (5, 4, 96, 1), (16, 40, 1536, 1), (3, 64, 96, 54)])
def test_snake_and_split(gpu, G, T, C, H):
    rng = np.random.default_rng(C * 5 + G)
    x = (rng.standard_normal((G * T, C)) * 3).astype(np.float32)
    ea = rng.uniform(0.5, 2.0, C).astype(np.float32)
    ib = rng.uniform(0.2, 1.5, C).astype(np.float32)
    big = rng.random((G * T, C)) < 0.3                    # |x * a| up to 1e5 (the range snake_sin's accuracy claim covers)
    x[big] = (rng.uniform(-1e5, 1e5, big.sum()) / ea[np.nonzero(big)[1]]).astype(np.float32)
    ext = G * (H + T) * C
    rows = R.ext_rows(G, T, H)
    out, = gpu.op_codec_kernel("SNAKE", G, T, C, H, ins=[x], outs=[_sent(ext)], p0=ea, p1=ib)
    _untouched(out, _rows_idx(rows, C))
    y = out.reshape(-1, C)[rows]
    ref, s = R.snake(x, ea, ib)
    _check(y, ref, R.snake_bar(ref, s, ib), "SNAKE")
    sp, = gpu.op_codec_kernel("SNAKE_SPLIT", G, T, C, H, ins=[x], outs=[_sent(ext)], p0=ea, p1=ib)
    _untouched(sp, _rows_idx(rows, C))
    h = np.ascontiguousarray(sp.reshape(-1, C)[rows]).view(np.float16)
    hi, lo = h[:, :C], h[:, C:]
    # the split planes are f16(y) and f16(y - f16(y)) of the very value SNAKE stores
    assert np.array_equal(hi.view(np.uint16), y.astype(np.float16).view(np.uint16))
    assert np.array_equal(lo.view(np.uint16), (y - hi.astype(np.float32)).astype(np.float16).view(np.uint16))
    # hi + lo carries ~22 bits wherever f16 can hold hi (|y| < 65520; the large-argument rows go past it and are compared as bits above)
    fin = np.isfinite(hi)
    assert fin.mean() > 0.6
    whole = hi.astype(np.float64) + lo.astype(np.float64)
    lo_step = np.spacing(np.abs(lo).astype(np.float16)).astype(np.float64) / 2 + 2.0 ** -25
    _check(whole[fin], ref[fin], (R.snake_bar(ref, s, ib) + lo_step)[fin], "SNAKE_SPLIT reassembled")


# ---------------- output conv ----------------
@pytest.mark.parametrize("G,T,C", [(1, 1, 16), (5, 7, 16), (1, 128, 96), (3, 256, 96), (16, 128, 96), (2, 100, 96)])
def test_conv_out(gpu, G, T, C):
    rng = np.random.default_rng(C + G * 11 + T)
    xe = rng.standard_normal((G, 6 + T, C)).astype(np.float32)
    w = (rng.standard_normal((7, C)) / np.sqrt(7 * C) * 2.5).astype(np.float32)   # |pcm| > 1 in a good share of samples
    bias = 0.125
    n = G * T
    wave, = gpu.op_codec_kernel("CONV_OUT_WAVE", G, T, C, 6, ins=[xe], outs=[_sent(n + 8)], p0=w, bias=bias)
    _untouched(wave, np.arange(n))
    ref, mag = R.conv_out(xe, w, bias, G, T)
    raw, _ = R.conv_out(xe, w, bias, G, T, clamp=False)
    bar = R.conv_out_bar(C, mag)
    _check(wave[:n], ref, bar, "CONV_OUT_WAVE")
    over = np.abs(raw) > 1 + bar
    assert n < 20 or over.sum() > n // 20
    assert np.array_equal(wave[:n][over], np.sign(raw[over]).astype(np.float32))                  # clamped to exactly +-1
    if C == 96 and T % 128 == 0:
        win, = gpu.op_codec_kernel("CONV_OUT_WIN", G, T, C, 6, ins=[xe], outs=[_sent(n + 8)], p0=w, bias=bias)
        _untouched(win, np.arange(n))
        assert np.array_equal(win.view(np.uint32), wave.view(np.uint32))    # same lane split, same order of adds
    else:
        with pytest.raises(gpu.Q3Error, match="CONV_OUT_WIN"):
            gpu.op_codec_kernel("CONV_OUT_WIN", G, T, C, 6, ins=[xe], outs=[_sent(n + 8)], p0=w, bias=bias)


# ---------------- histories ----------------
@pytest.mark.parametrize("G,T,H,C", [(1, 4, 2, 32), (3, 4, 6, 16), (3, 2, 6, 16), (5, 4, 71, 64), (16, 8, 1, 96)])
def test_history_load_save_zero(gpu, G, T, H, C):
    rng = np.random.default_rng(G * 7 + H)
    n_streams = G + 4
    slots = rng.permutation(n_streams)[:G]              # non-contiguous, unordered slots
    meta = _meta(G, slots=slots)
    store = rng.standard_normal(n_streams * H * C).astype(np.float32)
    work = rng.standard_normal(G * (H + T) * C).astype(np.float32)
    got, = gpu.op_codec_kernel("HIST_LOAD", G, T, C, H, ins=[store], outs=[work], meta=meta, n_streams=n_streams)
    assert np.array_equal(got.view(np.uint32), R.hist_load(store, work, slots, G, T, H, C).view(np.uint32))
    got, = gpu.op_codec_kernel("HIST_SAVE", G, T, C, H, ins=[work], outs=[store], meta=meta, n_streams=n_streams)
    assert np.array_equal(got.view(np.uint32), R.hist_save(work, store, slots, G, T, H, C).view(np.uint32))
    s = int(slots[-1])
    got, = gpu.op_codec_kernel("HIST_ZERO", G, T, C, H, outs=[store], n_streams=n_streams, stream=s)
    want = store.reshape(n_streams, H, C).copy()
    want[s] = 0
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))
    with pytest.raises(gpu.Q3Error, match="slot"):
        gpu.op_codec_kernel("HIST_LOAD", G, T, C, H, ins=[store], outs=[work], meta=_meta(G, slots=np.full(G, n_streams)), n_streams=n_streams)


# ---------------- decoder level ----------------
def _codec_path(model):
    return os.path.join(model, "onnx", "q3tts_codec.gguf")


def _pcm_close(got, ref, what):
    rms = float(np.sqrt(np.mean((got - ref) ** 2)))
    mx = float(np.abs(got - ref).max())
    print("%s: rms %.3g max %.3g" % (what, rms, mx))
    assert got.shape == ref.shape and rms < 1e-4 and mx < 1e-4, "%s: rms %.3g max %.3g" % (what, rms, mx)


def test_decoder_positions_across_8192_and_the_limit(gpu, oracle, tiny_model):
    """a stream imported with frames_seen = 8190 decodes 4-frame chunks across RoPE position 8192 like the oracle given the same counter;
    a call that would pass Q3TTS_CODEC_MAX_FRAMES is refused and leaves the state as it was; so is importing a larger counter"""
    path = _codec_path(tiny_model)
    gd = gpu.Decoder(path, n_streams=2, max_frames=4, max_group=2)
    oc = oracle.Codec(path)
    gd.reset(0)
    blob = gd.state_export(0)
    assert blob[-2] == 0 and blob[-1] == 0
    blob[-1] = 8190
    gd.state_import(blob, 0)
    oc.reset()
    oc.set_frames_seen(8190)
    codes = np.random.default_rng(81).integers(0, 2048, (12, 16))
    for o in (0, 4, 8):                                 # positions 8190..8193, 8194..8197, 8198..8201
        _pcm_close(gd.decode(codes[o:o + 4], False, 0), oc.decode(codes[o:o + 4]).copy(), "frames %d.." % (8190 + o))
    assert gd.state_export(0)[-1] == 8202
    # just below the limit: 4 frames fit exactly, one more is refused before anything runs
    blob[-1] = LIMIT - 4
    gd.state_import(blob, 0)
    oc.reset()
    oc.set_frames_seen(LIMIT - 4)
    _pcm_close(gd.decode(codes[:4], False, 0), oc.decode(codes[:4]).copy(), "frames %d.." % (LIMIT - 4))
    before = gd.state_export(0)
    assert before[-1] == LIMIT
    with pytest.raises(gpu.Q3Error, match="Q3TTS_CODEC_MAX_FRAMES"):
        gd.decode(codes[:1], False, 0)
    gd.reset(1)
    with pytest.raises(gpu.Q3Error, match="Q3TTS_CODEC_MAX_FRAMES"):
        gd.decode_group([1, 0], np.stack([codes[:1], codes[:1]]))    # the whole group is refused, stream 1 included
    assert np.array_equal(gd.state_export(0).view(np.uint32), before.view(np.uint32))
    assert gd.state_export(1)[-1] == 0
    blob[-1] = LIMIT + 1
    with pytest.raises(gpu.Q3Error, match="frame counter"):
        gd.state_import(blob, 0)
    assert np.array_equal(gd.state_export(0).view(np.uint32), before.view(np.uint32))
    oc.close(); gd.close()


def _staggered(gpu, oracle, path, n_streams, max_group, joins, n_chunks, check, seed):
    """streams join the group at the chunks in `joins` and decode 4-frame chunks until n_chunks; each stream's PCM vs the oracle's.
    Returns every stream's codes and PCM (test_gpu_codec_pcm_f64.py holds them to float64 per frame)"""
    gd = gpu.Decoder(path, n_streams=n_streams, max_frames=4, max_group=max_group)
    rng = np.random.default_rng(seed)
    G = len(joins)
    slots = [(3 * i + 1) % n_streams for i in range(G)]
    assert len(set(slots)) == G
    codes = [rng.integers(0, 2048, ((n_chunks - j) * 4, 16)) for j in joins]
    pcm = [[] for _ in range(G)]
    for c in range(n_chunks):
        live = [i for i in range(G) if joins[i] <= c]
        for i in live:
            if joins[i] == c:
                gd.reset(slots[i])
        o = [(c - joins[i]) * 4 for i in live]
        wav = gd.decode_group([slots[i] for i in live], np.stack([codes[i][a:a + 4] for i, a in zip(live, o)]))
        for k, i in enumerate(live):
            pcm[i].append(wav[k])
    oc = oracle.Codec(path)
    for i in check:
        oc.reset()
        _pcm_close(np.concatenate(pcm[i]), oc.decode(codes[i]).copy(), "stream %d (joined at chunk %d)" % (i, joins[i]))
    oc.close(); gd.close()
    return codes, [np.concatenate(p) for p in pcm]


def test_decoder_staggered_group_joins(gpu, oracle, tiny_model):
    """tiny codec (W = 8): five streams join at chunks 0, 0, 1, 3 and 6 and decode to chunk 10, so every pass mixes cache lengths 0, 4 and
    7 (saturated) and different positions; every stream against the oracle"""
    _staggered(gpu, oracle, _codec_path(tiny_model), 8, 5, [0, 0, 1, 3, 6], 10, range(5), 31)


@pytest.fixture(scope="module")
def full_model(synth_tool):
    import synth_models
    return synth_models.full("q8_0")


def test_fullsize_decoder_staggered_group_joins(gpu, oracle, full_model):
    """full codec (W = 72): four streams join at chunks 0, 1, 2 and 5 and decode 20 chunks (80 frames), past window saturation; the first
    and the last stream against the oracle"""
    _staggered(gpu, oracle, _codec_path(full_model), 7, 4, [0, 1, 2, 5], 20, (0, 3), 41)
