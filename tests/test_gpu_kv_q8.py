"""[EXT] KV cache type Q8_0: k_qk_rope_append_q8 + k_attention_q8kv through q3tts_op_attention_q8kv on synthetic problems
(tests/attention_cases.py, no model weights).  Append: every written quant and scale equals a numpy f32 restatement of q3_quant_block32
(attention_ref.quant_blocks) of the oracle's q3o_head_rope rows (K), the raw v (V) and, via qrot, the q rows; every other cache byte is
unchanged.  Attention: against the spec's quantised arithmetic in float64 over the device-stored cache, within a bound derived as
attention_ref.attention_tol derives UNFUSED's; with the scales of every position the launch must not read set to f16 NaN and their quants
to 0x80.  Refusals leave every buffer untouched.  (-m gpu)"""
import math

import numpy as np
import pytest

import attention_cases as AC
import attention_ref as R

pytestmark = pytest.mark.gpu


def _blocks(P):
    """edge "kblocks": cached keys with an all-zero block (d = 0) and a block whose amax sits in one element"""
    for s, (K, V) in enumerate(P.ctx):
        Kf = R.h2f(K)
        Kf[0::3, :, 32:64] = 0.0
        Kf[1::3, :, 64:96] = 0.0
        Kf[1::3, :, 70] = 3.0
        P.ctx[s] = (R.f16_bits(Kf), V)
    return P


def _case(name, seed, seqs, grp, edge=None, **kw):
    return AC.Problem(name, seed, seqs, n_head=2 * grp, n_kv=2, edge=edge, pos="distinct", **kw)


CASES = [_case("ctx%d_g%d" % (n, g), 300 + n, [(n - 1, 1)], g, layer=n % 3)
         for n, g in ((1, 2), (63, 1), (64, 4), (65, 2), (255, 4), (256, 1), (257, 2), (513, 2))]
CASES += [_case("gqa%d" % g, 320 + g, [(70, 1), (300, 1)], g) for g in (1, 4)]
CASES += [_case("decode3", 330, [(63, 1), (256, 1), (512, 1)], 2, layer=2),
          _case("prefill", 331, [(0, 70), (250, 10)], 2, layer=1),
          _case("big", 332, [(40, 1), (300, 1)], 2, edge="big"),            # score spreads far beyond the expf flush at -87
          _case("equal", 333, [(40, 1), (300, 1)], 2, edge="equal"),        # q = 0: every score equal, the query's d = 0
          _case("zero_v", 334, [(40, 1), (300, 1)], 2, edge="zero_v"),
          _blocks(_case("kblocks", 335, [(40, 1), (300, 1)], 2))]


def caches(P, poison):
    """kq [page][layer][kvh][4][64][32], ks [..][4][64], vq [..][64][128], vs [..][64][4] holding every sequence's context at the tested layer;
    everything else f16 NaN scales and 0x80 quants (poison) or random"""
    rng = np.random.default_rng(len(P.name))
    U = (P.n_pages, P.n_layer, P.n_kv)
    if poison:
        kq, vq = np.full(U + (4, R.PAGE, 32), -128, np.int8), np.full(U + (R.PAGE, R.HD), -128, np.int8)
        ks, vs = np.full(U + (4, R.PAGE), R.NAN16, np.uint16), np.full(U + (R.PAGE, 4), R.NAN16, np.uint16)
    else:
        kq, vq = (rng.integers(-127, 128, U + sh).astype(np.int8) for sh in ((4, R.PAGE, 32), (R.PAGE, R.HD)))
        ks, vs = (R.f16_bits(rng.uniform(0.01, 0.1, U + sh)) for sh in ((4, R.PAGE), (R.PAGE, 4)))
    for s, (K, V) in enumerate(P.ctx):
        if K.shape[0]:
            put(P, (kq, ks, vq, vs), s, np.arange(K.shape[0]), R.h2f(K), R.h2f(V))
    return kq, ks, vq, vs


def put(P, C, s, positions, K, V):
    """quantise (S2, numpy f32) logical rows K, V [len][n_kv][128] of sequence s and write them at `positions`"""
    kq, ks, vq, vs = C
    pg, pp = R._where(P.pages[s], positions)
    n = pg.size
    q, d = R.quant_blocks(K)
    kq[pg, P.layer, :, :, pp, :] = q.reshape(n, P.n_kv, 4, 32)
    ks[pg, P.layer, :, :, pp] = d.reshape(n, P.n_kv, 4)
    q, d = R.quant_blocks(V)
    vq[pg, P.layer, :, pp, :] = q.reshape(n, P.n_kv, R.HD)
    vs[pg, P.layer, :, pp, :] = d.reshape(n, P.n_kv, 4)


def run(q3, P, poison, **kw):
    C = caches(P, poison)
    r = q3.op_attention_q8kv(P.qkv, P.q_norm, P.k_norm, *C, P.n_head, P.n_kv, P.n_layer, P.layer, P.seq, P.slot, P.pos, eps=P.eps,
                             rope_base=P.base, n_ctx=P.n_ctx, mrope_sec=P.sec, page_table=P.table, **kw)
    return r, C


FLUSH = math.exp(-86.0)


def tol_q8(n, s, S):
    """tol of |y - y64| <= tol * sum_j p_j |v_j|, as attention_ref.attention_tol's UNFUSED branch with two changes.  The inputs are the
    quantised q and the stored cache themselves, so no norm / rotation term; the score is four fma terms of exact integers, the scale
    product and the scale: E_j = (4 + 3) u S_j, S_j = scale * sum_b |I_b e_b dk_b|.  The PV order is S7's with one more rounding per term
    (w = p_j * dv, rounded once, not accumulated): gamma = (chain + 1 + 8 + chunks * (8 + R)) u.
    The issue's bound, tol * w, holds every element but one kind: q3_expf returns 0 below -87 where float64 keeps e^x, so where quantised
    V is exactly 0 at every position the device does not flush, the device's element is 0 and w itself is a sum of flushed terms only
    (1e-45 in the spread case).  There, and only there, the caller allows FLUSH * sum_j |v_j| instead: p_j below e^-86 (one unit of
    margin for the score errors, far below 1 here) against L >= 1."""
    E = 7 * R.U * S
    spread = float(s.max() - s.min() + 2 * E.max())
    delta = 2 * float(E.max()) + R.U * spread + 3 * R.U
    chunks, chain = -(-n // R.CHUNK), -(-min(n, R.CHUNK) // 16)
    gamma = (chain + 1 + 8 + chunks * (8 + spread)) * R.U
    return 2 * delta + 2 * gamma + R.U


@pytest.mark.parametrize("P", CASES, ids=[P.name for P in CASES])
def test_q8kv(gpu, oracle, P):
    r, C = run(gpu, P, poison=True)
    tb = oracle.rope_tables(P.base, P.n_ctx)
    nh, nkv, grp = P.n_head, P.n_kv, P.n_head // P.n_kv
    # ---- append: the written rows are S2 of the oracle's rows; everything else is the input, bit for bit ----
    exp = tuple(a.copy() for a in C)
    for t in range(P.ntok):
        x = P.qkv[t]
        for h in range(nh):
            q = oracle.head_rope(x[h * R.HD:(h + 1) * R.HD], P.q_norm, P.eps, P.pos[t], P.sec, tb)
            assert np.array_equal(r["qrot"][t, h * R.HD:(h + 1) * R.HD].view(np.uint32), q.view(np.uint32)), (P.name, t, h, "qrot")
        k = np.stack([oracle.head_rope(x[(nh + j) * R.HD:(nh + j + 1) * R.HD], P.k_norm, P.eps, P.pos[t], P.sec, tb) for j in range(nkv)])
        v = x[(nh + nkv) * R.HD:(nh + 2 * nkv) * R.HD].reshape(nkv, R.HD)
        put(P, exp, int(P.seq[t]), [int(P.slot[t])], k[None], v[None])
    for name, e in zip(("kq", "ks", "vq", "vs"), exp):
        assert np.array_equal(r[name].reshape(e.shape), e), (P.name, name, "appended rows or untouched bytes differ")
    # ---- poison: nothing the launch must not read was read ----
    c, _ = run(gpu, P, poison=False)
    for key in ("att", "aq", "ad"):
        assert np.all(np.isfinite(r[key])) and np.array_equal(r[key], c[key]), (P.name, key, "differs from the clean-cache run")
    # ---- attention: the spec's quantised arithmetic in float64 over the stored cache ----
    worst = 0.0
    for t in range(P.ntok):
        n = int(P.slot[t]) + 1
        pg, pp = R._where(P.pages[int(P.seq[t])], np.arange(n))
        for j in range(nkv):
            Kq = exp[0][pg, P.layer, j, :, pp, :].astype(np.int64)                                    # [n][4][32]
            dk = R.h2f(exp[1][pg, P.layer, j, :, pp])                                                 # [n][4]
            V = exp[2][pg, P.layer, j, pp, :].astype(np.float64) * np.repeat(R.h2f(exp[3][pg, P.layer, j, pp, :]), 32, axis=1)
            for h in range(j * grp, (j + 1) * grp):
                qq, qe = R.quant_blocks(r["qrot"][t, h * R.HD:(h + 1) * R.HD])
                terms = np.einsum("nbi,bi->nb", Kq, qq.reshape(4, 32).astype(np.int64)) * (R.h2f(qe)[None, :] * dk) / math.sqrt(R.HD)
                s = terms.sum(1)
                e = np.exp(s - s.max())
                p = e / e.sum()
                y64, w = p @ V, p @ np.abs(V)
                tol = tol_q8(n, s, np.abs(terms).sum(1))
                y = r["att"][t, h * R.HD:(h + 1) * R.HD].astype(np.float64)
                err = np.abs(y - y64)
                kept = (s - s.max() >= -86.0).astype(np.float64) @ np.abs(V)          # > 0 where a position the device keeps has v != 0
                bound = np.where(kept > 0, tol * w, FLUSH * np.abs(V).sum(0))
                if (bound > 0).any():
                    worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
                assert np.all(err <= bound), (P.name, t, h, float(np.max(err - bound)), tol)
                aq, ad = R.quant_blocks(r["att"][t, h * R.HD:(h + 1) * R.HD])                         # S2 of the output row
                assert np.array_equal(r["aq"][t, h * R.HD:(h + 1) * R.HD], aq) and np.array_equal(r["ad"][t, h * 4:(h + 1) * 4], ad)
    print("F64 Q8KV %-12s max |y-y64| / bound = %.3f" % (P.name, worst))


REFUSED = [("grp3", dict(n_head=6)), ("grp16", dict(n_head=32)), ("slot", dict(slot=[64 * 6])), ("dup", dict(seq=[0, 0], slot=[5, 5]))]


@pytest.mark.parametrize("name,bad", REFUSED, ids=[n for n, _ in REFUSED])
def test_q8kv_refusals(gpu, name, bad):
    """grp outside {1, 2, 4, 8}, a slot beyond the paging, two tokens writing one (sequence, slot): an error, and every buffer as it was"""
    n_head, n_kv = bad.get("n_head", 4), 2
    seq, slot = np.array(bad.get("seq", [0]), np.int32), np.array(bad.get("slot", [5]), np.int32)
    nt = seq.size
    rng = np.random.default_rng(1)
    qkv = rng.standard_normal((nt, (n_head + 2 * n_kv) * R.HD)).astype(np.float32)
    U = (8, 1, n_kv)
    C = [rng.integers(-127, 128, U + (8192,)).astype(np.int8), R.f16_bits(rng.uniform(0.01, 0.1, U + (256,))),
         rng.integers(-127, 128, U + (8192,)).astype(np.int8), R.f16_bits(rng.uniform(0.01, 0.1, U + (256,)))]
    before = [a.copy() for a in C]
    table = np.arange(12, dtype=np.int32).reshape(2, 6) % 8
    with pytest.raises(gpu.Q3Error):
        gpu.op_attention_q8kv(qkv, np.ones(R.HD, np.float32), np.ones(R.HD, np.float32), *C, n_head, n_kv, 1, 0, seq, slot,
                              np.zeros((nt, 4), np.int32), page_table=table, copy=False)
    for a, b in zip(C, before):
        assert np.array_equal(a, b)
