"""Host-only checks of tests/codec_ops_ref.py, the float64 references and bounds the codec kernel tests rely on: the windowed attention
against brute-force masked attention, float32 computations of each operation inside its bound, each bound failing on a plausible mistake
(window start off by one, left-aligned history, clamped or mispaired RoPE, unclamped codes, sin for sin^2, single-pass variance), and
snake_sin's accuracy claim on a float32 model of its instruction sequence."""
import numpy as np
import pytest

import codec_ops_ref as R

F = np.float32
R_LIMIT = 65536     # Q3TTS_CODEC_MAX_FRAMES


def _within(got, ref, bar):
    return bool(np.all(np.abs(np.asarray(got, np.float64) - ref) <= bar))


def _attn_inputs(rng, nh, hd, W, G, T, kv):
    C, H = nh * hd, W - 1
    q = rng.standard_normal((G * T, C)).astype(F) * 2
    Kx = rng.standard_normal((G, H + T, C)).astype(F)
    Vx = rng.standard_normal((G, H + T, C)).astype(F)
    for g in range(G):
        Kx[g, :H - kv[g]] = np.nan
        Vx[g, :H - kv[g]] = np.nan
    return q, Kx, Vx


@pytest.mark.parametrize("W,T,kv", [(8, 1, [0, 1, 7]), (8, 4, [7, 3, 0]), (8, 11, [2, 7, 0]), (72, 4, [71, 35, 1]), (12, 3, [11, 0, 5])])
def test_window_attention_equals_masked_full_attention(W, T, kv):
    rng = np.random.default_rng(W + T)
    nh, hd, G = 2, 16, len(kv)
    H = W - 1
    q, Kx, Vx = _attn_inputs(rng, nh, hd, W, G, T, kv)
    out, pv, info = R.window_attn(q, Kx, Vx, kv, G, T, W, nh, hd)
    assert np.isfinite(out).all() and len(info) == G * T
    for g in range(G):
        seq_k, seq_v = Kx[g, H - kv[g]:], Vx[g, H - kv[g]:]   # the stream's visible positions: valid history, then the new rows
        ref = R.masked_full_attn(q[g * T:(g + 1) * T], seq_k, seq_v, nh, hd, W)
        assert np.allclose(out[g * T:(g + 1) * T], ref, rtol=1e-12, atol=1e-12)
        for t in range(T):
            assert info[g * T + t][1] == min(W, kv[g] + t + 1)


def _attn_f32(q, Kx, Vx, kv, G, T, W, nh, hd):
    """the kernel's arithmetic in float32 (scores, max-subtracted exp, PV sum, one division)"""
    H = W - 1
    out = np.zeros((G * T, nh, hd), F)
    for g in range(G):
        rows = np.concatenate([np.arange(H - kv[g], H), H + np.arange(T)])
        for t in range(T):
            j0, j1 = R.window_keys(kv[g], t, W)
            K = Kx[g, rows[j0:j1 + 1]].reshape(-1, nh, hd)
            V = Vx[g, rows[j0:j1 + 1]].reshape(-1, nh, hd)
            s = np.einsum("nhd,hd->hn", K, q[g * T + t].reshape(nh, hd)).astype(F) * F(1 / np.sqrt(hd))
            e = np.exp(s - s.max(1, keepdims=True)).astype(F)
            out[g * T + t] = np.einsum("hn,nhd->hd", e, V).astype(F) / e.sum(1, keepdims=True, dtype=F)
    return out.reshape(G * T, -1)


def test_attention_bound_holds_for_f32_and_fails_on_window_mistakes():
    rng = np.random.default_rng(5)
    nh, hd, W, T = 2, 32, 8, 4
    kv = [7, 3, 0, 7]
    G = len(kv)
    q, Kx, Vx = _attn_inputs(rng, nh, hd, W, G, T, kv)
    ref, pv, info = R.window_attn(q, Kx, Vx, kv, G, T, W, nh, hd)
    bar = R.attn_bar(info, hd, T, pv)
    assert _within(_attn_f32(q, Kx, Vx, kv, G, T, W, nh, hd), ref, bar)
    for mistake in (dict(start_off=1), dict(start_off=-1)):
        kx = np.nan_to_num(Kx)          # an extra key reaches into the invalid rows: give them values to show the bound, not a NaN
        vx = np.nan_to_num(Vx)
        wrong, _, _ = R.window_attn(q, kx, vx, kv, G, T, W, nh, hd, **mistake)
        assert not _within(wrong, ref, bar), mistake
    kx = rng.standard_normal(Kx.shape).astype(F)
    vx = rng.standard_normal(Vx.shape).astype(F)
    kx[:, W - 1:], vx[:, W - 1:] = Kx[:, W - 1:], Vx[:, W - 1:]
    for g in range(G):                  # left-aligned: the valid rows where a right-aligned reader does not look (kv = 3 here)
        kx[g, :kv[g]], vx[g, :kv[g]] = Kx[g, W - 1 - kv[g]:W - 1], Vx[g, W - 1 - kv[g]:W - 1]
    wrong, _, _ = R.window_attn(q, kx, vx, kv, G, T, W, nh, hd, left_aligned=True)
    assert np.allclose(wrong, ref)      # the same data read the left-aligned way is the same attention ...
    wrong, _, _ = R.window_attn(q, kx, vx, kv, G, T, W, nh, hd)
    assert not _within(wrong, ref, bar)  # ... and a right-aligned kernel over left-aligned rows is caught


def _rope_f32(x, pos, nh, hd, base):
    ang = R.rope_angles(pos, hd, base)
    c, s = np.cos(ang).astype(F)[:, None, :], np.sin(ang).astype(F)[:, None, :]
    x = np.asarray(x, F).reshape(len(pos), nh, hd)
    a, b = x[..., :hd // 2], x[..., hd // 2:]
    return np.concatenate([a * c - b * s, b * c + a * s], -1).reshape(len(pos), -1)


def test_rope_bound_holds_for_f32_tables_and_fails_on_clamp_and_pairing():
    rng = np.random.default_rng(6)
    nh, hd = 4, 64
    pos = np.array([0, 1, 8190, 8191, 8192, 8193, 20000, R_LIMIT - 1])
    x = rng.standard_normal((len(pos), nh * hd)).astype(F)
    ref, mag = R.rope(x, pos, nh, hd, 10000.0)
    bar = R.rope_bar(ref, mag)
    assert _within(_rope_f32(x, pos, nh, hd, 10000.0), ref, bar)
    clamped, _ = R.rope(x, pos, nh, hd, 10000.0, clamp_at=8192)
    over = pos >= 8192
    assert _within(clamped[~over], ref[~over], bar[~over])
    assert all(not _within(clamped[i], ref[i], bar[i]) for i in np.flatnonzero(over))
    adj, _ = R.rope(x, pos, nh, hd, 10000.0, adjacent=True)
    assert not _within(adj[1:], ref[1:], bar[1:])


def test_rvq_bound_fails_on_unclamped_codes():
    rng = np.random.default_rng(7)
    cb = rng.standard_normal((16, 64, 32)).astype(F)
    codes = rng.integers(0, 64, (6, 16))
    codes[0, 3], codes[2, 0], codes[4, 15] = -1, 64, 70
    ref, mag = R.rvq_sum(codes, cb)
    bar = R.rvq_bar(16, mag)
    c = np.clip(codes, 0, 63)
    acc = np.zeros((6, 32), F)
    for q in range(16):
        acc = acc + cb[q][c[:, q]]
    assert _within(acc, ref, bar)
    wrapped, _ = R.rvq_sum(codes, cb, clamp=False)
    for r in (0, 2, 4):
        assert not _within(wrapped[r], ref[r], bar[r])


def test_norm_bounds_hold_for_f32_and_fail_on_single_pass_variance():
    rng = np.random.default_rng(8)
    C = 1024
    x = rng.standard_normal((4, C)) * np.array([1.0, 1e-3, 1e3, 1.0])[:, None]
    x[3] = 1e3 + rng.standard_normal(C) * 1e-2
    x = x.astype(F)
    w = rng.uniform(-2, 2, C).astype(F)
    b = rng.uniform(-1, 1, C).astype(F)
    ref = R.layernorm(x, w, b, 1e-6)
    bar = R.layernorm_bar(x, w, b, 1e-6)
    mu = x.mean(1, keepdims=True, dtype=F)
    d = x - mu
    var = (d * d).mean(1, keepdims=True, dtype=F)
    two = d * (F(1) / np.sqrt(var + F(1e-6))) * w + b
    assert _within(two, ref, bar)
    one = R.layernorm_f32_single_pass(x, w, b, 1e-6)
    assert not _within(one[3], ref[3], bar[3])
    g = rng.uniform(-2, 2, C).astype(F)
    rms = x * (F(1) / np.sqrt((x * x).mean(1, keepdims=True, dtype=F) + F(1e-5))) * g
    assert _within(rms, R.rmsnorm(x, g, 1e-5), R.rmsnorm_bar(x, g, 1e-5))


def _fma(a, b, c):
    """fmaf modelled as the f32 rounding of the f64 value (the product is exact in f64; the sum's rounding is below the f32 one)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def snake_sin_model(x):
    """codec.hip snake_sin, instruction by instruction in float32"""
    x = np.asarray(x, F)
    n = np.rint(x * F(0.63661977236758134))
    r = _fma(n, F(-1.57079637050628662), x)
    r = _fma(n, F(4.37113900018624283e-8), r)
    q = n.astype(np.int64)
    r2 = r * r
    sp = _fma(_fma(_fma(F(-1.9515295891e-4), r2, F(8.3321608736e-3)), r2, F(-1.6666654611e-1)), r2 * r, r)
    cp = _fma(_fma(_fma(F(2.443315711809948e-5), r2, F(-1.388731625493765e-3)), r2, F(4.166664568298827e-2)), r2 * r2, _fma(F(-0.5), r2, F(1.0)))
    v = np.where(q & 1, cp, sp)
    return np.where(q & 2, -v, v)


def test_snake_sin_accuracy_claim():
    """|snake_sin(x) - sin(x)| < 1e-7 for f32 x up to |x| = 1e5: random points over every scale plus the neighbourhoods of k * pi/4"""
    rng = np.random.default_rng(9)
    xs = [rng.uniform(-1e5, 1e5, 2_000_000), rng.uniform(-50, 50, 1_000_000),
          np.exp(rng.uniform(np.log(1e-6), np.log(1e5), 1_000_000)) * rng.choice([-1, 1], 1_000_000)]
    k = rng.integers(-127_000, 127_000, 200_000)
    edge = (k * (np.pi / 4))[:, None] + np.arange(-8, 9)[None, :] * np.spacing(np.abs(k * (np.pi / 4)).astype(F)).astype(np.float64)[:, None]
    xs.append(edge.ravel())
    x = np.concatenate(xs).astype(F)
    x = x[np.abs(x) <= 1e5]
    err = np.abs(snake_sin_model(x).astype(np.float64) - np.sin(x.astype(np.float64)))
    assert x.size > 7_000_000
    assert err.max() < R.SNAKE_SIN_ERR, "max |err| %.3g at x = %r" % (err.max(), x[np.argmax(err)])


def test_snake_bound_holds_for_the_model_and_fails_on_sin_for_sin_squared():
    rng = np.random.default_rng(10)
    C = 96
    x = (rng.standard_normal((64, C)) * 3).astype(F)
    ea = rng.uniform(0.5, 2.0, C).astype(F)
    ib = rng.uniform(0.2, 1.5, C).astype(F)
    x[::4] = (rng.uniform(-1e5, 1e5, (16, C)) / ea).astype(F)
    ref, s = R.snake(x, ea, ib)
    bar = R.snake_bar(ref, s, ib)
    sn = snake_sin_model(x * ea)
    assert _within(x + ib * (sn * sn), ref, bar)
    wrong, _ = R.snake(x, ea, ib, square=False)
    assert not _within(wrong, ref, bar)


def test_dwconv_and_conv_out_references():
    rng = np.random.default_rng(11)
    G, T, C = 3, 5, 16
    xe = rng.standard_normal((G, 6 + T, C)).astype(F)
    w = rng.standard_normal((C, 7)).astype(F)
    b = rng.standard_normal(C).astype(F)
    ref, mag = R.dwconv7(xe, w, b, G, T)
    for g in range(G):                 # causal: output t of a stream reads its rows t .. t+6, tap 6 = the current (new) row
        for t in range(T):
            assert np.allclose(ref[g * T + t], b + (w.T.astype(float) * xe[g, t:t + 7]).sum(0), rtol=1e-12, atol=1e-12)
    wo = rng.standard_normal((7, C)).astype(F)
    pcm, m2 = R.conv_out(xe, wo, 0.5, G, T)
    raw, _ = R.conv_out(xe, wo, 0.5, G, T, clamp=False)
    assert np.array_equal(pcm, np.clip(raw, -1, 1)) and (np.abs(raw) > 1).any()
    assert np.allclose(raw[T + 2], 0.5 + (wo.astype(float) * xe[1, 2:9]).sum(), rtol=1e-12)


def test_history_moves():
    rng = np.random.default_rng(12)
    G, T, H, C, n = 3, 2, 6, 4, 7
    slots = [5, 0, 3]
    store = rng.standard_normal(n * H * C)
    work = rng.standard_normal(G * (H + T) * C)
    loaded = R.hist_load(store, work, slots, G, T, H, C).reshape(G, H + T, C)
    assert np.array_equal(loaded[1, :H], store.reshape(n, H, C)[0]) and np.array_equal(loaded[:, H:], work.reshape(G, H + T, C)[:, H:])
    saved = R.hist_save(work, store, slots, G, T, H, C).reshape(n, H, C)
    assert np.array_equal(saved[3], work.reshape(G, H + T, C)[2, T:])       # T < H: old history rows T.. then the T new rows
    assert np.array_equal(saved[1], store.reshape(n, H, C)[1])
