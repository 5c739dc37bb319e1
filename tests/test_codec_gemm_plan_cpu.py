"""Host-only checks of the codec GEMM dispatch (q3tts_codec_gemm_plan = the decoder's plan_gemm, csrc/codec.hip) and of the float64 reference
helpers the GPU GEMM tests (tests/test_gpu_codec_gemm.py) rely on.  No GPU needed."""
import re
import os

import numpy as np
import pytest

import codec_gemm_ref as R
from q3tts import GEMM_FORMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T0 = 4   # frames per decode call


def _full_codec_dims():
    """the full-size synthetic codec's dims, read from tools/q3synth.c (ccfg "full")"""
    src = open(os.path.join(ROOT, "tools", "q3synth.c")).read()
    m = re.search(r'if \(!strcmp\(preset, "full"\)\).*?codec = \(ccfg\)\{([^;]*)\};', src, re.S)
    nums = [int(x) for x in re.findall(r"-?\d+", m.group(1))]
    keys = ["hidden", "cb_dim", "n_layers", "n_heads", "head_dim", "ffn", "window", "dec_dim", "n_up", "n_dec"]
    d = dict(zip(keys, nums[:10]))
    d["up"] = nums[10:10 + d["n_up"]]
    d["rates"] = nums[10 + d["n_up"]:10 + d["n_up"] + d["n_dec"]]
    return d


def decoder_gemms(G):
    """every GEMM one grouped pass of the full-size decoder runs (G streams x T0 frames), with the row layouts CodecDecoder uses:
    name -> plan_gemm arguments"""
    c = _full_codec_dims()
    H, ffn, dec = c["hidden"], c["ffn"], c["dec_dim"]
    # split-K workspace of a lane: 2 x the largest activation of a pass (max_frames = T0, max_group = G), at least 2^20 floats
    tlat = T0
    for f in c["up"]:
        tlat *= f
    max_act, T, ch = max(tlat * 4 * H, tlat * dec), tlat, dec
    for r in c["rates"]:
        T *= r
        ch //= 2
        max_act = max(max_act, T * ch)
    ws = max(2 * max_act * G, 1 << 20)
    g = {}

    def add(name, M, N, cin, taps=1, dil=1, ldo=None, o_segT=0, o_skip=0, a_segT=0, a_skip=0, epi=R.EPI_NONE, ldr=0, r_segT=0, r_skip=0):
        g[name] = dict(M=M, N=N, cin=cin, taps=taps, dil=dil, ldo=N if ldo is None else ldo, o_segT=o_segT, o_skip=o_skip, a_segT=a_segT,
                       a_skip=a_skip, epi=epi, ldr=ldr, r_segT=r_segT, r_skip=r_skip, ws_floats=ws)

    R0 = G * T0
    add("pre_conv", R0, H, c["cb_dim"], 3, 1, a_segT=T0, a_skip=2)
    add("qkv", R0, 3 * H, H)
    add("wo", R0, H, H, epi=R.EPI_RES_SCALE, ldr=H)
    add("gate_up", R0, 2 * ffn, H)
    add("down", R0, H, ffn, epi=R.EPI_RES_SCALE, ldr=H)
    T = T0
    for i, f in enumerate(c["up"]):
        add("up%d.convT" % i, G * T, f * H, H, ldo=f * H, o_segT=T, o_skip=6 * H)
        T *= f
        add("up%d.pw1" % i, G * T, 4 * H, H, epi=R.EPI_GELU)
        add("up%d.pw2" % i, G * T, H, 4 * H, epi=R.EPI_RES_SCALE, ldr=H, r_segT=T, r_skip=6 * H)
    add("conv_in", G * T, dec, H, 7, 1, a_segT=T, a_skip=6)
    ch = dec
    for b, r in enumerate(c["rates"]):
        co = ch // 2
        add("dec%d.convT" % b, G * T, r * co, ch, 2, 1, a_segT=T, a_skip=1)
        T *= r
        for u, d in enumerate((1, 3, 9)):
            add("dec%d.ru%d.conv1" % (b, u), G * T, co, co, 7, d, a_segT=T, a_skip=6 * d, epi=R.EPI_SNAKE)
        add("dec%d.ru.conv2" % b, G * T, co, co, epi=R.EPI_RES, ldr=co)
        ch = co
    return g


# (form, ksplit, reducer) the dispatcher picks for the full-size decoder at T0 = 4 frames per stream
PLANS = {
    1: {
        "pre_conv": ("SKINNY4", 1, -1), "qkv": ("SKINNY4", 1, -1), "wo": ("SKINNY4", 1, -1), "gate_up": ("SKINNY4", 1, -1),
        "down": ("SKINNY4", 1, -1), "up0.convT": ("SKINNY4", 1, -1), "up0.pw1": ("SKINNY8", 1, -1), "up0.pw2": ("SKINNY8", 1, -1),
        "up1.convT": ("SKINNY8", 1, -1), "up1.pw1": ("SKINNY16", 1, -1), "up1.pw2": ("SKINNY16", 1, -1), "conv_in": ("SKINNY16", 1, -1),
        "dec0.convT": ("SKINNY16", 1, -1), "dec0.ru0.conv1": ("H1_EPL", 8, 1), "dec0.ru1.conv1": ("H1_EPL", 8, 1), "dec0.ru2.conv1": ("H1_EPL", 8, 1),
        "dec0.ru.conv2": ("H1_EPL", 4, 1), "dec1.convT": ("H1_EPL", 4, 1), "dec1.ru0.conv1": ("H1_EPL", 4, 1), "dec1.ru1.conv1": ("H1_EPL", 4, 1),
        "dec1.ru2.conv1": ("H1_EPL", 4, 1), "dec1.ru.conv2": ("H1_EPL", 2, 1), "dec2.convT": ("H1_EPL", 2, 1), "dec2.ru0.conv1": ("H1_EPL", 2, 1),
        "dec2.ru1.conv1": ("H1_EPL", 2, 1), "dec2.ru2.conv1": ("H1_EPL", 2, 1), "dec2.ru.conv2": ("H1_EPL", 1, -1), "dec3.convT": ("H1_EPL", 2, 1),
        "dec3.ru0.conv1": ("H1_EPL", 1, -1), "dec3.ru1.conv1": ("H1_EPL", 1, -1), "dec3.ru2.conv1": ("H1_EPL", 1, -1),
        "dec3.ru.conv2": ("H1_EPL", 1, -1),
    },
    4: {
        "pre_conv": ("SKINNY16", 1, -1), "qkv": ("SKINNY16", 1, -1), "wo": ("SKINNY16", 1, -1), "gate_up": ("SKINNY16", 1, -1),
        "down": ("SKINNY16", 1, -1), "up0.convT": ("SKINNY16", 1, -1), "up0.pw1": ("F32_1", 8, 0), "up0.pw2": ("F32_1", 16, 0),
        "up1.convT": ("F32_1", 8, 0), "up1.pw1": ("H1_EPL", 4, 1), "up1.pw2": ("H1_EPL", 16, 1), "conv_in": ("H1_EPL", 16, 1),
        "dec0.convT": ("H1_EPL", 4, 1), "dec0.ru0.conv1": ("H1_EPL", 4, 1), "dec0.ru1.conv1": ("H1_EPL", 4, 1), "dec0.ru2.conv1": ("H1_EPL", 4, 1),
        "dec0.ru.conv2": ("H1_EPL", 4, 1), "dec1.convT": ("H1_EPL", 2, 1), "dec1.ru0.conv1": ("H1_EPL", 2, 1), "dec1.ru1.conv1": ("H1_EPL", 2, 1),
        "dec1.ru2.conv1": ("H1_EPL", 2, 1), "dec1.ru.conv2": ("H1_EPL", 2, 1), "dec2.convT": ("H3_EPL", 1, -1), "dec2.ru0.conv1": ("H3_EPL", 1, -1),
        "dec2.ru1.conv1": ("H3_EPL", 1, -1), "dec2.ru2.conv1": ("H3_EPL", 1, -1), "dec2.ru.conv2": ("H3_EPL", 1, -1), "dec3.convT": ("H3_EPL", 1, -1),
        "dec3.ru0.conv1": ("H3_EPL", 1, -1), "dec3.ru1.conv1": ("H3_EPL", 1, -1), "dec3.ru2.conv1": ("H3_EPL", 1, -1),
        "dec3.ru.conv2": ("H3_EPL", 1, -1),
    },
    16: {
        "pre_conv": ("H1_EPL", 8, 1), "qkv": ("H1_EPL", 8, 1), "wo": ("H1_EPL", 8, 1), "gate_up": ("H1_EPL", 4, 1), "down": ("H1_EPL", 16, 1),
        "up0.convT": ("H1_EPL", 8, 1), "up0.pw1": ("H1_EPL", 2, 1), "up0.pw2": ("H1_EPL", 8, 1), "up1.convT": ("H1_EPL", 4, 1),
        "up1.pw1": ("H1_EPL", 1, -1), "up1.pw2": ("H1_EPL", 4, 1), "conv_in": ("H1_EPL", 4, 1), "dec0.convT": ("H3_EPL", 1, -1),
        "dec0.ru0.conv1": ("H3_EPL", 1, -1), "dec0.ru1.conv1": ("H3_EPL", 1, -1), "dec0.ru2.conv1": ("H3_EPL", 1, -1),
        "dec0.ru.conv2": ("H3_EPL", 1, -1), "dec1.convT": ("H3_EPL", 1, -1), "dec1.ru0.conv1": ("H3_EPL", 1, -1), "dec1.ru1.conv1": ("H3_EPL", 1, -1),
        "dec1.ru2.conv1": ("H3_EPL", 1, -1), "dec1.ru.conv2": ("H3_EPL", 1, -1), "dec2.convT": ("H3_EPL", 1, -1), "dec2.ru0.conv1": ("H3_EPL", 1, -1),
        "dec2.ru1.conv1": ("H3_EPL", 1, -1), "dec2.ru2.conv1": ("H3_EPL", 1, -1), "dec2.ru.conv2": ("H3_EPL", 1, -1), "dec3.convT": ("H3_EPL", 1, -1),
        "dec3.ru0.conv1": ("H3_EPL", 1, -1), "dec3.ru1.conv1": ("H3_EPL", 1, -1), "dec3.ru2.conv1": ("H3_EPL", 1, -1),
        "dec3.ru.conv2": ("H3_EPL", 1, -1),
    },
}


@pytest.mark.parametrize("G", (1, 4, 16))
def test_full_decoder_dispatch_is_pinned(q3, G):
    got = {n: q3.codec_gemm_plan(**a) for n, a in decoder_gemms(G).items()}
    assert got == PLANS[G]


def test_gpu_cases_cover_every_form_the_decoder_uses():
    covered = {(c[0], c[8] > 1, c[9]) for c in R.FORCED_CASES}
    for G, plans in PLANS.items():
        for name, (form, ks, red) in plans.items():
            assert (form, ks > 1, red) in covered, (G, name, form, ks, red)
    # and every form at all: ks = 1, and for the tiled forms ks > 1 with both reducers
    forms = {c[0] for c in R.FORCED_CASES}
    assert forms == set(GEMM_FORMS) - {"AUTO"}
    for f in forms - {"SKINNY4", "SKINNY8", "SKINNY16"}:
        assert {(f, False, -1), (f, True, 0), (f, True, 1)} <= covered, f


def test_plan_rejects_a_bad_descriptor(q3):
    with pytest.raises(q3.Q3Error):
        q3.codec_gemm_plan(0, 64, 64)


def test_plan_follows_alignment_and_workspace(q3):
    # the 16-byte epilogue needs an aligned output and N % 4 == 0; split-K needs workspace for its slabs
    assert q3.codec_gemm_plan(128, 768, 768, 7) == ("H1_EPL", 8, 1)
    assert q3.codec_gemm_plan(128, 768, 768, 7, out_off=1) == ("H1", 8, 0)
    assert q3.codec_gemm_plan(128, 766, 768, 7) == ("H1", 8, 0)
    assert q3.codec_gemm_plan(128, 768, 768, 7, ws_floats=128 * 768) == ("H1_EPL", 1, -1)
    assert q3.codec_gemm_plan(2048, 768, 768, 7) == ("H3_EPL", 1, -1)
    assert q3.codec_gemm_plan(2048, 768, 768, 7, out_off=2) == ("H3", 1, -1)
    assert q3.codec_gemm_plan(2048, 704, 64, 2) == ("H2_EPL", 1, -1)   # tall tile: N >= 512, 1024+ rows, 176 tiles


# ---- the reference helpers themselves (a wrong reference must not pass silently) ----
def test_im2col_dilation_and_segments():
    rng = np.random.default_rng(0)
    cin, taps, dil, T, H, G = 3, 3, 2, 4, 5, 3
    A = rng.standard_normal((G * (H + T) + 8, cin + 1))
    M = G * T
    X = R.im2col(A, M, cin, taps, dil, T, H)
    for m in range(M):
        g, t = divmod(m, T)
        for j in range(taps):
            for ci in range(cin):
                assert X[m, j * cin + ci] == A[g * (H + T) + t + j * dil, ci]
    assert np.array_equal(R.im2col(A, 5, cin, 1, 1), A[:5, :cin])
    assert list(R.seg_rows(np.arange(7), 3, 10)) == [0, 1, 2, 13, 14, 15, 26]
    assert list(R.seg_rows(np.arange(3), 0, 10)) == [0, 1, 2]
    idx = R.out_index(4, 2, 5, 7, 2, 3)
    assert idx.tolist() == [[7, 8], [12, 13], [20, 21], [25, 26]]


def test_gemm_ref_against_a_loop():
    rng = np.random.default_rng(1)
    A = rng.standard_normal((20, 4))
    W = rng.standard_normal((3, 8))
    acc, absb = R.gemm_ref(A, W, 6, 4, 2, 3, 3, 2)
    for m in range(6):
        row = m + (m // 3) * 2
        x = np.concatenate([A[row, :4], A[row + 3, :4]])
        assert np.allclose(acc[m], W @ x, rtol=1e-14) and np.allclose(absb[m], np.abs(W) @ np.abs(x), rtol=1e-14)


def test_f16_split_emulation():
    x = np.float32([1.0, 1.0 + 2.0 ** -20, 0.1, -3.3e4, 2.0 ** -20, 1e-3, 0.0])
    hi, lo = R.f16_split(x)
    assert hi.dtype == np.float16 and lo.dtype == np.float16
    v = hi.astype(np.float64) + lo.astype(np.float64)
    big = np.abs(x) >= 0.125
    assert np.all(np.abs(v - x)[big] <= 2.0 ** -22 * np.abs(x[big]))
    assert np.all(np.abs(v - x)[~big] <= 2.0 ** -25)
    assert hi[0] == 1.0 and lo[0] == 0.0 and hi[1] == 1.0 and float(lo[1]) == 2.0 ** -20
    rows = np.float32([[0.1, -2.5, 3e-3, 7.0]])
    w = R.split_rows(rows)
    assert w.shape == (1, 4) and w.dtype == np.uint32
    h2, l2, val = R.unsplit_rows(w, 4)
    assert np.array_equal(h2, R.f16_split(rows)[0]) and np.array_equal(l2, R.f16_split(rows)[1])
    assert np.all(np.abs(val - rows) <= 2.0 ** -22 * np.abs(rows) + 2.0 ** -25)


def test_weight_prescale_keeps_22_bits_at_any_scale():
    rng = np.random.default_rng(2)
    for e in (-20, -10, -3, 0, 12):
        W = (rng.standard_normal((4, 512)) * 2.0 ** e).astype(np.float32)
        _, _, scaled = R.split_weights_emul(W, prescale=True)
        rel = np.abs(scaled - W) / np.abs(W).max(axis=1, keepdims=True)
        assert rel.max() <= 2.0 ** -22, e
        _, _, plain = R.split_weights_emul(W, prescale=False)
        rel0 = np.abs(plain - W) / np.abs(W).max(axis=1, keepdims=True)
        if e <= -10:   # the unscaled split loses bits below 2^-3 (lo is an f16 subnormal)
            assert rel0.max() > 2.0 ** -18, e
    hi, lo, _ = R.split_weights_emul(np.float32([[3.0, -1.0]]))
    assert float(hi[0, 0]) == 3.0 * 2 ** 12   # max 3 in [2, 4): scaled by 2^12 into [2^13, 2^14)


def test_epilogue_reference():
    v = np.array([[0.0, 1.0, -1.0, 10.0]])
    assert np.allclose(R.epilogue(v, R.EPI_GELU), [[0.0, 0.8413447460685429, -0.15865525393145707, 10.0]], rtol=1e-15, atol=1e-300)
    assert np.allclose(R.epilogue(v, R.EPI_RES_SCALE, bias=[1, 1, 1, 1], res=v, scale=[2, 2, 2, 2]), [[2.0, 5.0, -1.0, 32.0]])
    assert np.allclose(R.epilogue(v, R.EPI_RES, res=v), 2 * v)
    ea, ib = np.array([1.0, 2.0, 0.5, 1.0]), np.array([1.0, 0.5, 2.0, 0.0])
    assert np.allclose(R.epilogue(v, R.EPI_SNAKE, ea=ea, ib=ib), v + ib * np.sin(v * ea) ** 2)
    assert np.array_equal(R.epilogue(v, R.EPI_NONE, bias=[1, 2, 3, 4]), v + [1, 2, 3, 4])
