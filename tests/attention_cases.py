"""Synthetic attention problems for q3tts_op_attention (tests/test_gpu_attention.py) and the host-side checks of their float64 bound
(tests/test_attention_plan_cpu.py).  No model: every shape and value is generated here from a seed."""
import zlib

import numpy as np

import attention_ref as R

REAL_SEC = (24, 20, 20, 0)   # the talker's M-RoPE sections (rope.dimension_sections)


class Problem:
    """One launch: `seqs` = [(cached positions, new tokens)] per sequence; the new tokens of a sequence sit at consecutive slots, and the
    launch interleaves the sequences' tokens (ragged prefill when a sequence has several).
    paging: "perm" = a random permutation of physical pages, sequences' pages interleaved, spare pages; "identity" = no table (page s);
    uniform_pos >= 0: the predictor's form (token t = sequence t = page t at slot uniform_pos, every stream = uniform_pos).
    pos: "same" = [p, p, p, 0] for slot p (the talker's text positions), "distinct" = four different streams, or a callable (tok, slot) -> [4].
    edge: None, "big" (large q / k norm weights: score spreads far beyond 87), "equal" (q = 0), "dominant" (one cached key aligned with q),
    "chunks" (cached keys shifted along q per 256-chunk: the chunk maxima rise, then fall), "zero_v" (kv head 0 has V = 0)."""

    def __init__(self, name, seed, seqs, n_head=16, n_kv=8, n_layer=3, layer=0, n_ctx=4096, sec=REAL_SEC, paging="perm", uniform_pos=-1,
                 pos="same", edge=None, eps=1e-6, base=1e6):
        rng = np.random.default_rng(seed)
        self.name, self.n_head, self.n_kv, self.n_layer, self.layer, self.n_ctx = name, n_head, n_kv, n_layer, layer, n_ctx
        self.sec, self.eps, self.base, self.uniform_pos, self.edge = tuple(sec), eps, base, uniform_pos, edge
        if uniform_pos >= 0:
            seqs = [(uniform_pos, 1)] * len(seqs)
            paging = "identity"
        self.seqs = list(seqs)
        # tokens: round-robin over the sequences' new tokens
        toks, k = [], 0
        while any(k < nn for _, nn in seqs):
            toks += [(s, c + k) for s, (c, nn) in enumerate(seqs) if k < nn]
            k += 1
        self.seq = np.array([t[0] for t in toks], np.int32)
        self.slot = np.array([t[1] for t in toks], np.int32)
        self.ntok = len(toks)
        self.distinct_streams = uniform_pos < 0 and pos != "same"
        if uniform_pos >= 0:
            self.pos = np.full((self.ntok, 4), uniform_pos, np.int32)
        elif callable(pos):
            self.pos = np.array([pos(t, int(self.slot[t])) for t in range(self.ntok)], np.int32)
        elif pos == "distinct":
            self.pos = np.stack([self.slot, self.slot // 2 + 3, np.maximum(self.slot - 5, 0) * 3 % n_ctx, (self.slot * 7 + 1) % n_ctx], 1).astype(np.int32)
        else:
            self.pos = np.stack([self.slot, self.slot, self.slot, 0 * self.slot], 1).astype(np.int32)
        # pages
        need = [(c + nn - 1) // R.PAGE + 1 for c, nn in seqs]
        if paging == "identity":
            assert max(c + nn for c, nn in seqs) <= R.PAGE
            self.table, self.n_pages = None, len(seqs) + 1
            self.pages = [[s] for s in range(len(seqs))]
        else:
            max_pages = max(need) + 1
            total = sum(need) + 3
            perm = rng.permutation(total)
            self.pages, it = [[] for _ in seqs], iter(perm)
            for lp in range(max(need)):                       # logical page lp of every sequence in turn: interleaved
                for s in range(len(seqs)):
                    if lp < need[s]:
                        self.pages[s].append(int(next(it)))
            spare = [int(p) for p in it]
            self.table = np.array([pg + [spare[(s + j) % len(spare)] for j in range(max_pages - len(pg))] for s, pg in enumerate(self.pages)],
                                  np.int32)
            self.n_pages = total
        # inputs
        d = (n_head + 2 * n_kv) * R.HD
        self.qkv_stride = d + 8
        self.qkv = (rng.standard_normal((self.ntok, self.qkv_stride)) * 1.5).astype(np.float32)
        self.q_norm = rng.uniform(0.5, 1.5, R.HD).astype(np.float32)
        self.k_norm = rng.uniform(0.5, 1.5, R.HD).astype(np.float32)
        kscale = 1.0
        if edge == "big":
            self.q_norm *= np.float32(12.0)
            self.k_norm *= np.float32(12.0)
            kscale = 12.0
        if edge == "equal":
            self.q_norm[:] = 0.0
        if edge == "zero_v":
            self.qkv[:, (n_head + n_kv) * R.HD:(n_head + n_kv + 1) * R.HD] = 0.0
        # the cached context of the tested layer: logical rows [seq] -> K, V [c][n_kv][128] (f16 bits)
        self.ctx = []
        for s, (c, nn) in enumerate(seqs):
            K = rng.standard_normal((c, n_kv, R.HD)) * kscale
            V = rng.standard_normal((c, n_kv, R.HD))
            if edge == "zero_v":
                V[:, 0] = 0.0
            if edge in ("dominant", "chunks") and c > 0:
                for kvh in range(n_kv):                       # along the f64 query of the group's first head (the sequence's first token)
                    t0 = int(np.nonzero(self.seq == s)[0][0])
                    q = self.q64(t0, kvh * (n_head // n_kv))[0]
                    qh = q / np.linalg.norm(q)
                    if edge == "dominant":
                        K[rng.integers(0, c), kvh] = 40.0 * qh      # its score exceeds the others' by ~40
                    else:
                        beta = np.array([0.0, 2.5, 5.0, 1.0, 3.0])[np.minimum(np.arange(c) // R.CHUNK, 4)]
                        K[:, kvh] += beta[:, None] * qh * 3.0
            self.ctx.append((R.f16_bits(K), R.f16_bits(V)))

    # ---- f64 of the inputs ----
    def q64(self, t, h):
        x = self.qkv[t, h * R.HD:(h + 1) * R.HD]
        return R.head_rope(x, self.q_norm, self.eps, self.pos[t], self.sec, self.base, self.n_ctx)

    def k64(self, t, kvh):
        x = self.qkv[t, (self.n_head + kvh) * R.HD:(self.n_head + kvh + 1) * R.HD]
        return R.head_rope(x, self.k_norm, self.eps, self.pos[t], self.sec, self.base, self.n_ctx)

    def v_row(self, t, kvh):
        o = (self.n_head + self.n_kv + kvh) * R.HD
        return self.qkv[t, o:o + R.HD]

    # ---- caches ----
    def caches(self, poison):
        """the launch's input caches: the cached context of every sequence at the tested layer; everything else NaN (poison) or random"""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        Kc, Vc = R.new_caches(self.n_pages, self.n_layer, self.n_kv, R.NAN16)
        if not poison:   # finite values, different in every page, layer and head
            Kc[...] = R.f16_bits(rng.standard_normal((self.n_pages, self.n_layer, self.n_kv, 1, 1, 8)) + rng.standard_normal((16, R.PAGE, 8)))
            Vc[...] = R.f16_bits(rng.standard_normal((self.n_pages, self.n_layer, self.n_kv, 1, 1)) + rng.standard_normal((R.PAGE, R.HD)))
        for s, (K, V) in enumerate(self.ctx):
            if K.shape[0]:
                R.write_rows(Kc, Vc, self.pages[s], self.layer, np.arange(K.shape[0]), K, V)
        return Kc, Vc

    def op_args(self, poison):
        Kc, Vc = self.caches(poison)
        kw = dict(n_head=self.n_head, n_kv=self.n_kv, n_layer=self.n_layer, layer=self.layer, eps=self.eps, rope_base=self.base,
                  n_ctx=self.n_ctx, mrope_sec=self.sec, page_table=self.table)
        if self.uniform_pos >= 0:
            kw["uniform_pos"] = self.uniform_pos
        else:
            kw.update(seq=self.seq, slot=self.slot, pos=self.pos)
        return (self.qkv, self.q_norm, self.k_norm, Kc.reshape(self.n_pages, -1), Vc.reshape(self.n_pages, -1)), kw

    def one_per_seq(self):
        return len(set(self.seq.tolist())) == self.ntok

    def logical(self, Kc, Vc, t):
        """the K / V rows [n][n_kv][128] token t attends to, read from (written-back) caches"""
        Kc = Kc.reshape(self.n_pages, self.n_layer, self.n_kv, 16, R.PAGE, 8)
        Vc = Vc.reshape(self.n_pages, self.n_layer, self.n_kv, R.PAGE, R.HD)
        return R.read_rows(Kc, Vc, self.pages[int(self.seq[t])], self.layer, np.arange(int(self.slot[t]) + 1))

    def appended(self, Kc, Vc, t):
        K, V = self.logical(Kc, Vc, t)
        return K[-1], V[-1]


_tables = {}


def _rope_tables(O, P):
    key = (P.base, P.n_ctx)
    if key not in _tables:
        _tables[key] = O.rope_tables(P.base, P.n_ctx)
    return _tables[key]


def expect(O, P, ggml, Kin, Vin):
    """the oracle's result of the launch: att [ntok][n_head*128], aq, ad, and the written caches"""
    tb = _rope_tables(O, P)
    Kc = Kin.copy().reshape(P.n_pages, P.n_layer, P.n_kv, 16, R.PAGE, 8)
    Vc = Vin.copy().reshape(P.n_pages, P.n_layer, P.n_kv, R.PAGE, R.HD)
    nh, nkv, grp = P.n_head, P.n_kv, P.n_head // P.n_kv
    q = np.zeros((P.ntok, nh, R.HD), np.float32)
    for t in range(P.ntok):
        x = P.qkv[t]
        for h in range(nh):
            q[t, h] = O.head_rope(x[h * R.HD:(h + 1) * R.HD], P.q_norm, P.eps, P.pos[t], P.sec, tb, ggml)
        k = np.stack([O.head_rope(x[(nh + j) * R.HD:(nh + j + 1) * R.HD], P.k_norm, P.eps, P.pos[t], P.sec, tb, ggml) for j in range(nkv)])
        v = x[(nh + nkv) * R.HD:(nh + 2 * nkv) * R.HD].reshape(nkv, R.HD)
        R.write_rows(Kc, Vc, P.pages[int(P.seq[t])], P.layer, [int(P.slot[t])], R.f16_bits(k)[None], R.f16_bits(v)[None])
    att = np.zeros((P.ntok, nh * R.HD), np.float32)
    aq = np.zeros((P.ntok, nh * R.HD), np.int8)
    ad = np.zeros((P.ntok, nh * 4), np.uint16)
    for t in range(P.ntok):
        K, V = P.logical(Kc, Vc, t)
        for h in range(nh):
            att[t, h * R.HD:(h + 1) * R.HD] = O.attn_head(q[t, h], K[:, h // grp], V[:, h // grp], ggml)
        aq[t], ad[t] = O.quant_act(att[t])
    return dict(att=att, aq=aq, ad=ad, k_cache=Kc.reshape(P.n_pages, -1), v_cache=Vc.reshape(P.n_pages, -1))


def check_f64(P, form, r):
    """float64 contract of one run: returns the largest |y - y64| / sum_j p_j |v_j| and its ratio to the bound"""
    nh, nkv, grp = P.n_head, P.n_kv, P.n_head // P.n_kv
    worst, worst_rel = 0.0, 0.0
    for t in range(P.ntok):
        K, V = P.logical(r["k_cache"], r["v_cache"], t)   # what the device stored
        Kf, Vf = R.h2f(K), R.h2f(V)
        for j in range(nkv):
            k64, kmag = P.k64(t, j)
            e = 16 * R.U * kmag                             # f32 error of the normed, rotated k (the same derivation as q's)
            lo, hi = R.f16_bracket(k64 - e, k64 + e)
            assert np.all((Kf[-1, j] >= lo) & (Kf[-1, j] <= hi)), (P.name, form, t, j, "appended K is not a rounding of k64")
            assert np.array_equal(V[-1, j], R.f16_bits(P.v_row(t, j))), (P.name, form, t, j, "appended V is not f16(v)")
        for h in range(nh):
            q64, qmag = P.q64(t, h)
            y64, w, _ = R.attention(q64, Kf[:, h // grp], Vf[:, h // grp])
            tol = R.attention_tol(form, q64, qmag, Kf[:, h // grp])
            if r["att"] is not None:
                y = r["att"][t, h * R.HD:(h + 1) * R.HD].astype(np.float64)
                bound = tol * w
            else:   # FUSED: only the quantised row; add the S2 step (half a quantum, the f16 rounding of the scale)
                d = R.h2f(r["ad"][t, h * 4:(h + 1) * 4])
                y = r["aq"][t, h * R.HD:(h + 1) * R.HD].astype(np.float64) * np.repeat(d, 32)
                bound = tol * w + np.repeat(d, 32) * (0.5 + 128 * 2.0 ** -11)
            err = np.abs(y - y64)
            assert np.all(err <= bound), (P.name, form, t, h, float(np.max(err - bound)), tol)
            nz = w > 0
            if nz.any() and r["att"] is not None:
                worst = max(worst, float(np.max(err[nz] / w[nz])))
                worst_rel = max(worst_rel, float(np.max(err[nz] / (tol * w[nz]))))
    return worst, worst_rel


def context_cases():
    """n = slot + 1 across page, chunk and n_ctx edges, one sequence each (UNFUSED / FUSED / GGML), plus all of them mixed in one launch"""
    ns = [1, 2, 16, 17, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1500, 4096]
    out = [Problem("ctx%d" % n, 100 + n, [(n - 1, 1)], layer=2 if n % 2 else 0) for n in ns]
    out.append(Problem("ctx_mixed", 7, [(n - 1, 1) for n in ns[:-1]], layer=2, pos="distinct"))
    return out


def short_cases():
    """contexts the short forms serve (n <= 64), per-token metadata on a permuted table and the predictor's uniform form"""
    ns = [1, 2, 16, 17, 33, 63, 64]
    out = [Problem("short_mixed", 21, [(n - 1, 1) for n in ns], pos="distinct")]
    out += [Problem("short_uniform%d" % n, 30 + n, [(0, 1)] * 5, uniform_pos=n - 1, layer=2) for n in (1, 17, 64)]
    return out


def gqa_cases():
    """n_head / n_kv = 1, 2, 4, 8 and the real 16 / 8"""
    return [Problem("gqa%d_%d" % (h, k), 40 + h * 8 + k, [(70, 1), (3, 1), (300, 1)], n_head=h, n_kv=k, layer=(h + k) % 2 * 2)
            for h, k in ((4, 4), (4, 2), (8, 2), (16, 2), (16, 8), (2, 1))]


def ntok_cases():
    """token counts around the fused limit (8) and the short forms' switch (128): per-token metadata, permuted pages"""
    return [Problem("ntok%d" % n, 60 + n, [(int(i * 7 % 60), 1) for i in range(n)], pos="distinct", layer=0 if n % 2 else 2)
            for n in (1, 7, 8, 9, 64, 129, 300)]


def prefill_cases():
    """several tokens of one sequence at consecutive slots in one launch, ragged across sequences (UNFUSED / GGML)"""
    return [Problem("prefill", 80, [(0, 5), (61, 7), (250, 9), (3, 1)], pos="distinct"),
            Problem("prefill_identity", 81, [(0, 12), (40, 20)], paging="identity", layer=2)]


def mrope_cases():
    """four distinct streams per token: the real sections, all zero, and sections summing below 64 (the mapping wraps);
    positions 0 and n_ctx - 1; one case beyond [0, n_ctx) (the kernels clamp to the table: see test_mrope_clamp)"""
    last = lambda t, s: [4095, 0, 4095 - t, t]
    far = lambda t, s: [5000 + t, -3, 4095, 4096]
    return [Problem("mrope_real", 90, [(5, 1), (200, 1), (64, 1)], pos="distinct"),
            Problem("mrope_zero", 91, [(5, 1), (200, 1), (64, 1)], pos="distinct", sec=(0, 0, 0, 0)),
            Problem("mrope_wrap", 92, [(5, 1), (200, 1), (64, 1)], pos="distinct", sec=(7, 5, 3, 2)),
            Problem("mrope_last", 93, [(10, 1), (33, 1)], pos=last, sec=(16, 8, 8, 0)),
            Problem("mrope_clamp", 94, [(10, 1), (33, 1)], pos=far, sec=(16, 8, 8, 0))]


def edge_cases():
    return [Problem("edge_big", 95, [(40, 1), (700, 1)], edge="big"),
            Problem("edge_equal", 96, [(40, 1), (700, 1)], edge="equal"),
            Problem("edge_dominant", 97, [(40, 1), (700, 1)], edge="dominant"),
            Problem("edge_chunks", 98, [(1100, 1), (600, 1)], edge="chunks"),
            Problem("edge_zero_v", 99, [(40, 1), (300, 1)], edge="zero_v")]


def forms_for(P):
    """the forced forms whose preconditions the problem meets"""
    forms = ["UNFUSED", "GGML"]
    if P.one_per_seq():
        forms.append("FUSED")
        if P.n_head == 2 * P.n_kv and int(P.slot.max()) < R.PAGE:
            forms += ["SHORT1", "SHORT2"]
    return forms


def all_cases():
    return context_cases() + short_cases() + gqa_cases() + ntok_cases() + prefill_cases() + mrope_cases() + edge_cases()
