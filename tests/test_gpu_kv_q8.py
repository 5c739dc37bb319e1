"""[EXT] KV cache type Q8_0: k_qk_rope_append_q8 + k_attention_q8kv through q3tts_op_attention_q8kv on synthetic problems
(tests/attention_cases.py, no model weights).  Append: every written quant and scale equals a numpy f32 restatement of q3_quant_block32
(attention_ref.quant_blocks) of the oracle's q3o_head_rope rows (K), the raw v (V) and, via qrot, the q rows; every other cache byte is
unchanged.  Attention: against the spec's quantised arithmetic in float64 over the device-stored cache, within a bound derived as
attention_ref.attention_tol derives UNFUSED's (attention_ref.attention_q8), and bit for bit against the oracle's q3o_attn_head_q8 over the
same bytes -- which tests/test_kv_q8_oracle_cpu.py holds to the same float64 bound on these very problems; with the scales of every
position the launch must not read set to f16 NaN and their quants to 0x80.  The problems reach every instance (1, 2, 4 and 8 query heads
per kv head), 1, 2, 3 and 8 kv heads, the talker's geometry at its last layer, and the launch without a page table, which the operator
accepts for contexts of one page (slot < 64).  Refusals leave every buffer untouched.  (-m gpu)"""
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


def _case(name, seed, seqs, grp, edge=None, n_kv=2, **kw):
    return AC.Problem(name, seed, seqs, n_head=n_kv * grp, n_kv=n_kv, edge=edge, pos="distinct", **kw)


CASES = [_case("ctx%d_g%d" % (n, g), 300 + n, [(n - 1, 1)], g, layer=n % 3)
         for n, g in ((1, 2), (63, 1), (64, 4), (65, 2), (255, 4), (256, 1), (257, 2), (513, 2))]
# k_attention_q8kv<8>: the one instance whose waves merge two heads (w and w + 4) and hold four q registers per thread
CASES += [_case("ctx%d_g8" % n, 340 + n, [(n - 1, 1)], 8, layer=n % 3) for n in (1, 65, 257)]
CASES += [_case("kv1_g%d" % g, 350 + g, [(70, 1), (130, 1)], g, n_kv=1, layer=1) for g in (8, 1)]
CASES += [_case("kv3_g2", 353, [(70, 1), (130, 1)], 2, n_kv=3, layer=2),
          _case("decode3_g8", 354, [(63, 1), (256, 1), (200, 1)], 8, layer=1),
          # the talker's own geometry, last layer: the largest unit offsets the product reaches
          _case("talker", 355, [(69, 1), (129, 1)], 2, n_kv=8, n_layer=28, layer=27),
          # no page table: sequence s owns page s (kv.page_table == nullptr in both kernels), a prefill and a decode beside it
          _case("identity", 356, [(0, 12), (40, 1)], 2, paging="identity", layer=2),
          _case("identity_g8", 357, [(63, 1), (5, 3)], 8, paging="identity")]
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


def appended(oracle, P, C):
    """the oracle's side of the append: (qrot [ntok][n_head * 128] = its q3o_head_rope rows, the caches C with S2 of its K rows and of the
    raw v written at every token's (sequence, slot))"""
    tb = oracle.rope_tables(P.base, P.n_ctx)
    nh, nkv = P.n_head, P.n_kv
    exp = tuple(a.copy() for a in C)
    qrot = np.zeros((P.ntok, nh * R.HD), np.float32)
    for t in range(P.ntok):
        x = P.qkv[t]
        for h in range(nh):
            qrot[t, h * R.HD:(h + 1) * R.HD] = oracle.head_rope(x[h * R.HD:(h + 1) * R.HD], P.q_norm, P.eps, P.pos[t], P.sec, tb)
        k = np.stack([oracle.head_rope(x[(nh + j) * R.HD:(nh + j + 1) * R.HD], P.k_norm, P.eps, P.pos[t], P.sec, tb) for j in range(nkv)])
        v = x[(nh + nkv) * R.HD:(nh + 2 * nkv) * R.HD].reshape(nkv, R.HD)
        put(P, exp, int(P.seq[t]), [int(P.slot[t])], k[None], v[None])
    return qrot, exp


def stored(P, C, t, j):
    """what token t attends to in kv head j, in logical order: Kq [n][4][32] int8, ks [n][4], Vq [n][128] int8, vs [n][4] (f16 bits)"""
    pg, pp = R._where(P.pages[int(P.seq[t])], np.arange(int(P.slot[t]) + 1))
    return C[0][pg, P.layer, j, :, pp, :], C[1][pg, P.layer, j, :, pp], C[2][pg, P.layer, j, pp, :], C[3][pg, P.layer, j, pp, :]


def check_heads(P, C, qrot, att, oracle=None):
    """every (token, head) of att [ntok][n_head * 128] against the spec's quantised arithmetic in float64 over the caches C (R.attention_q8)
    and, given the oracle, against q3o_attn_head_q8 over the same bytes bit for bit.  Returns the largest |y - y64| / bound"""
    grp, worst = P.n_head // P.n_kv, 0.0
    for t in range(P.ntok):
        for j in range(P.n_kv):
            Kq, ks, Vq, vs = stored(P, C, t, j)
            V = Vq.astype(np.float64) * np.repeat(R.h2f(vs), 32, axis=1)
            for h in range(j * grp, (j + 1) * grp):
                qq, qe = R.quant_blocks(qrot[t, h * R.HD:(h + 1) * R.HD])
                y64, bound, tol = R.attention_q8(qq, qe, Kq.astype(np.int64), R.h2f(ks), V)
                y = att[t, h * R.HD:(h + 1) * R.HD]
                err = np.abs(y.astype(np.float64) - y64)
                if (bound > 0).any():
                    worst = max(worst, float(np.max(err[bound > 0] / bound[bound > 0])))
                assert np.all(err <= bound), (P.name, t, h, float(np.max(err - bound)), tol)
                if oracle is not None:
                    yo = oracle.attn_head_q8(qrot[t, h * R.HD:(h + 1) * R.HD], Kq.reshape(-1, R.HD), ks, Vq, vs)
                    assert np.array_equal(y.view(np.uint32), yo.view(np.uint32)), (P.name, t, h, "att differs from q3o_attn_head_q8")
    return worst


@pytest.mark.parametrize("P", CASES, ids=[P.name for P in CASES])
def test_q8kv(gpu, oracle, P):
    r, C = run(gpu, P, poison=True)
    # ---- append: the written rows are S2 of the oracle's rows; everything else is the input, bit for bit ----
    qrot, exp = appended(oracle, P, C)
    assert np.array_equal(r["qrot"].view(np.uint32), qrot.view(np.uint32)), (P.name, "qrot")
    for name, e in zip(("kq", "ks", "vq", "vs"), exp):
        assert np.array_equal(r[name].reshape(e.shape), e), (P.name, name, "appended rows or untouched bytes differ")
    # ---- poison: nothing the launch must not read was read ----
    c, _ = run(gpu, P, poison=False)
    for key in ("att", "aq", "ad"):
        assert np.all(np.isfinite(r[key])) and np.array_equal(r[key], c[key]), (P.name, key, "differs from the clean-cache run")
    # ---- attention: within the float64 bound of the spec's quantised arithmetic over the stored cache, and the oracle's bits ----
    worst = check_heads(P, exp, r["qrot"], r["att"], oracle)
    aq, ad = R.quant_blocks(r["att"])                                                                 # S2 of the output rows
    assert np.array_equal(r["aq"].reshape(-1), aq) and np.array_equal(r["ad"].reshape(-1), ad)
    print("F64 Q8KV %-12s max |y-y64| / bound = %.3f" % (P.name, worst))


REFUSED = [("grp3", dict(n_head=6)), ("grp16", dict(n_head=32)), ("slot", dict(slot=[64 * 6])), ("slot_g8", dict(n_head=16, slot=[64 * 6])),
           ("dup", dict(seq=[0, 0], slot=[5, 5]))]


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
