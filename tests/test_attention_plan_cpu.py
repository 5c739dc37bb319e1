"""Host-only checks of the attention dispatch (q3tts_attention_plan = plan_attention, csrc/transformer.cpp), of the float64 reference the GPU
attention tests rely on (tests/attention_ref.py), and of the bound they hold the kernels to: the oracle's arithmetic meets it on every case
of tests/test_gpu_attention.py, and plausible wrong answers on the same cases do not.  No GPU needed."""
import math

import numpy as np
import pytest

import attention_cases as AC
import attention_ref as R
from q3tts import attention_plan

CASES = AC.all_cases()


# ---------------- dispatch ----------------
def test_plan_talker():
    """talker (16 q / 8 kv heads, no short form): decode steps of 1..8 tokens run k_attention_fused, wider steps and prefill the unfused pair"""
    for n in range(1, 9):
        assert attention_plan(n) == "FUSED"
    for n in (9, 64, 256):
        assert attention_plan(n) == "UNFUSED"
    for n in (1, 2, 8, 100):
        assert attention_plan(n, same_seq=True) == "UNFUSED"
    assert attention_plan(4, fused=False) == "UNFUSED"         # Q3_UNFUSED=1


def test_plan_predictor():
    """code predictor (short form from 8 tokens): < 8 -> FUSED, 8..128 -> SHORT1, >= 129 -> SHORT2; its prefill stays unfused"""
    for n in range(1, 8):
        assert attention_plan(n, short_attn_min=8) == "FUSED"
    for n in (8, 9, 64, 128):
        assert attention_plan(n, short_attn_min=8) == "SHORT1"
    for n in (129, 132, 256, 512):
        assert attention_plan(n, short_attn_min=8, fused_max_tok=8) == "SHORT2"
    assert attention_plan(16, short_attn_min=8, same_seq=True) == "UNFUSED"
    assert attention_plan(4, n_head=2, n_kv=1, short_attn_min=8) == "FUSED"
    assert attention_plan(132, n_head=2, n_kv=1, short_attn_min=8) == "SHORT2"
    assert attention_plan(64, n_head=16, n_kv=4, short_attn_min=8) == "UNFUSED"  # the short forms need n_head == 2 n_kv
    assert attention_plan(8, n_head=16, n_kv=4, short_attn_min=8) == "FUSED"
    assert attention_plan(16, short_attn_min=8, fused=False) == "SHORT1"         # Q3_UNFUSED=1 keeps the short form
    assert attention_plan(16, short_attn_min=8, hpw1_max=8) == "SHORT2"          # Q3_SHORT_ATTN_HPW1_MAX
    assert attention_plan(16, short_attn_min=0) == "UNFUSED"                     # Q3_SHORT_ATTN_MIN=0


def test_plan_modes():
    for n in (1, 8, 9, 200):
        assert attention_plan(n, float_mode=True) == "UNFUSED"
        assert attention_plan(n, ggml_mode=True) == "GGML"
        assert attention_plan(n, ggml_mode=True, short_attn_min=1) == "GGML"
    assert attention_plan(8, float_mode=True, short_attn_min=8) == "SHORT1"
    assert attention_plan(7, float_mode=True, short_attn_min=8) == "UNFUSED"


# ---------------- the float64 reference ----------------
def test_pack_roundtrip():
    rng = np.random.default_rng(1)
    Kc, Vc = R.new_caches(9, 3, 2, R.NAN16)
    pages = [7, 2, 5]
    K = R.f16_bits(rng.standard_normal((150, 2, 128)))
    V = R.f16_bits(rng.standard_normal((150, 2, 128)))
    R.write_rows(Kc, Vc, pages, 1, np.arange(150), K, V)
    K2, V2 = R.read_rows(Kc, Vc, pages, 1, np.arange(150))
    assert np.array_equal(K, K2) and np.array_equal(V, V2)
    # element (pos, kvh, d) of K sits at [page][layer][kvh][d / 8][pos % 64][d % 8], V at [page][layer][kvh][pos % 64][d]
    assert Kc[5, 1, 1, 100 // 8, 130 % 64, 100 % 8] == K[130, 1, 100]
    assert Vc[2, 1, 0, 70 % 64, 33] == V[70, 0, 33]
    written = np.zeros(Kc.shape, bool)
    written[[7, 2, 5], 1] = True
    written[5, 1, :, :, 150 - 128:, :] = False
    assert np.all(Kc[~written] == R.NAN16) and np.all(Kc[written] != R.NAN16)


def test_attention_trivial():
    rng = np.random.default_rng(2)
    v = rng.standard_normal((1, 128))
    y, w, _ = R.attention(rng.standard_normal(128), rng.standard_normal((1, 128)), v)
    assert np.array_equal(y, v[0]) and np.array_equal(w, np.abs(v[0]))
    V = rng.standard_normal((37, 128))
    y, _, _ = R.attention(np.zeros(128), rng.standard_normal((37, 128)), V)
    assert np.allclose(y, V.mean(0), rtol=0, atol=1e-15)


def test_mrope_sections():
    real = (24, 20, 20, 0)
    assert [R.mrope_stream(i, real) for i in (0, 23, 24, 43, 44, 63)] == [0, 0, 1, 1, 2, 2]
    wrap = (7, 5, 3, 2)                     # 17 pairs per period: pair 17 is stream 0 again
    assert [R.mrope_stream(i, wrap) for i in (0, 6, 7, 11, 12, 14, 15, 16, 17, 24, 63)] == [0, 0, 1, 1, 2, 2, 3, 3, 0, 1, 2]
    assert all(R.mrope_stream(i, (0, 0, 0, 0)) == 0 for i in range(64))
    assert [R.mrope_stream(i, (0, 0, 0, 8)) for i in (0, 9)] == [3, 3]
    # pair i rotates by p_stream * base^(-i/64)
    ang = R.rope_angles([10, 20, 30, 40], (1, 1, 1, 1), 1e6, 4096)
    assert np.allclose(ang[[0, 5, 63]], [10, 20 * 1e6 ** (-5 / 64), 40 * 1e6 ** (-63 / 64)], rtol=1e-15, atol=0)
    clamped = R.rope_angles([9000, -4, 0, 0], (1, 1, 0, 0), 1e6, 4096)   # positions clamp to [0, n_ctx - 1]
    assert clamped[0] == 4095 and clamped[1] == 0


def test_quant_blocks(oracle):
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(256) * np.repeat([1e-3, 1, 7, 0, 1e4, 0.3, 2, 5], 32)).astype(np.float32)
    q, d = R.quant_blocks(x)
    q2, d2 = oracle.quant_act(x)
    assert np.array_equal(q, q2) and np.array_equal(d, d2)


# ---------------- the bound ----------------
@pytest.mark.parametrize("P", CASES, ids=[P.name for P in CASES])
def test_oracle_meets_bound(oracle, P):
    """the oracle restates the kernels' arithmetic (the GPU tests hold them bit-equal): it must meet the float64 bound on every case"""
    for ggml in (False, True):
        Kc, Vc = P.caches(True)
        e = AC.expect(oracle, P, ggml, Kc.reshape(P.n_pages, -1), Vc.reshape(P.n_pages, -1))
        AC.check_f64(P, "GGML" if ggml else "UNFUSED", e)


def _wrong_answers(P):
    """f64 outputs of the launch under plausible mistakes -> {mistake: (y, y64, w, tol)} over every token and head"""
    nh, nkv, grp = P.n_head, P.n_kv, P.n_head // P.n_kv
    rng = np.random.default_rng(5)
    out = {}

    def rot(t, h, which, stream_shift=0, swap=False, flip=False):
        x = P.qkv[t, h * R.HD:(h + 1) * R.HD]
        y = R.head_norm(x, P.q_norm if which == "q" else P.k_norm, P.eps)
        sec = P.sec
        i = np.arange(64)
        stream = np.array([(R.mrope_stream(k, sec) + stream_shift) % 4 for k in i])
        p = np.clip(P.pos[t][stream], 0, P.n_ctx - 1).astype(np.float64)
        ang = p * np.power(float(np.float32(P.base)), -i / 64.0)
        if flip:
            ang = -ang
        if swap:
            y = np.concatenate([y[64:], y[:64]])
        return R.rope(y, ang)

    def ctx(t, kvh, **mut):
        s = int(P.seq[t])
        K0, V0 = P.ctx[s]
        K = R.h2f(K0[:, kvh])
        V = R.h2f(V0[:, kvh])
        rows = [(int(P.slot[u]), u) for u in range(P.ntok) if int(P.seq[u]) == s and P.slot[u] <= P.slot[t]]
        n = int(P.slot[t]) + 1
        Kf = np.zeros((n, 128)); Vf = np.zeros((n, 128))
        Kf[:K.shape[0]], Vf[:V.shape[0]] = K[:n], V[:n]
        for sl, u in rows:
            Kf[sl] = R.h2f(R.f16_bits(rot(u, nh + kvh, "k", **mut)))
            Vf[sl] = R.h2f(R.f16_bits(P.v_row(u, kvh)))
        return Kf, Vf

    def merge_without_rescale(q, K, V):
        s = K @ q / math.sqrt(128)
        num, den = 0, 0
        for c0 in range(0, len(s), 256):
            e = np.exp(s[c0:c0 + 256] - s[c0:c0 + 256].max())
            num, den = num + e @ V[c0:c0 + 256], den + e.sum()
        return num / den

    muts = {"ctx+1": {}, "ctx-1": {}, "kv_head+1": {}, "stream+1": dict(stream_shift=1), "rope_swap": dict(swap=True),
            "rope_sign": dict(flip=True), "merge_no_rescale": {}}
    for name, mut in muts.items():
        if name == "ctx-1" and int(P.slot.min()) == 0 or name == "kv_head+1" and nkv == 1:
            continue
        if name == "merge_no_rescale" and int(P.slot.max()) < 256:
            continue
        res = []
        for t in range(P.ntok):
            for h in range(nh):
                kvh = h // grp
                q, qmag = P.q64(t, h)
                K, V = ctx(t, kvh)
                y64, w, _ = R.attention(q, K, V)
                tol = max(R.attention_tol(f, q, qmag, K) for f in ("UNFUSED", "GGML"))
                if name in ("stream+1", "rope_swap", "rope_sign"):
                    Kw, Vw = ctx(t, kvh, **mut)
                    yw = R.attention(rot(t, h, "q", **mut), Kw, Vw)[0]
                elif name == "ctx+1":
                    yw = R.attention(q, np.vstack([K, rng.standard_normal(128)]), np.vstack([V, rng.standard_normal(128)]))[0]
                elif name == "ctx-1":
                    if K.shape[0] < 2:
                        continue
                    yw = R.attention(q, K[:-1], V[:-1])[0]
                elif name == "kv_head+1":
                    yw = R.attention(q, *ctx(t, (kvh + 1) % nkv))[0]
                else:
                    if K.shape[0] <= 256:
                        continue
                    yw = merge_without_rescale(q, K, V)
                res.append((np.abs(yw - y64), w, tol))
        out[name] = res
    return out


MATERIAL = 1e-4   # a mistake moves some output by more than this fraction of sum_j p_j |v_j|: far above f32 rounding (the bound is ~1e-5)
_wrong_cache = {}


def _worst(P):
    """{mistake: (largest change / sum p|v|, largest change / bound)} on case P"""
    if P.name not in _wrong_cache:
        out = {}
        for name, res in _wrong_answers(P).items():
            if res:
                out[name] = (max(float(np.max(d / np.maximum(w, 1e-300))) for d, w, _ in res),
                             max(float(np.max(d / np.maximum(tol * w, 1e-300))) for d, w, tol in res))
        _wrong_cache[P.name] = out
    return _wrong_cache[P.name]


@pytest.mark.parametrize("P", CASES, ids=[P.name for P in CASES])
def test_bound_has_teeth(P):
    """every plausible wrong answer that moves the case's output materially exceeds the bound somewhere in the launch (a mistake can be
    immaterial on a case: a dropped position of negligible weight, a stream shift between equal positions, a rescale between equal maxima)"""
    for name, (change, over) in _worst(P).items():
        if name == "stream+1" and not P.distinct_streams:
            continue
        if change > MATERIAL:
            assert over > 1.0, (P.name, name, change, over)


def test_every_mistake_is_caught():
    """each mistake is caught on some case of the list"""
    caught = {}
    for P in CASES:
        for name, (_, over) in _worst(P).items():
            caught[name] = max(caught.get(name, 0.0), over)
    assert sorted(caught) == sorted(["ctx+1", "ctx-1", "kv_head+1", "stream+1", "rope_swap", "rope_sign", "merge_no_rescale"])
    assert all(v > 1.0 for v in caught.values()), caught
