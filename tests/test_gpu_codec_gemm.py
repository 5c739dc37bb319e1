"""Every codec GEMM form (csrc/codec.hip: k_skinny_gemm, k_conv_gemm, k_conv_gemm_h, k_conv_gemm_h3, both split-K reducers), forced through
q3tts_op_codec_gemm, against a float64 reference element by element: shape edges, segmented rows, epilogues in isolation, stores outside the
logical output, AUTO dispatch = the form it reports, and the split-f16 precision contract over weight / activation scales.  (-m gpu)"""
import numpy as np
import pytest

import codec_gemm_ref as R

pytestmark = pytest.mark.gpu

SENTINEL = 0x7FA5A5A5   # a NaN bit pattern no kernel computes


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


class Problem:
    """one GEMM with its buffers: A in a batched extended layout (G segments of T rows, H history rows each), the output in one with
    OH history rows per segment and ldo > N (padding columns), all of it filled with SENTINEL before the call"""

    def __init__(self, rng, M, N, cin, taps=1, dil=1, G=1, H=0, a_split=False, out_pad=None, OH=2, out_misalign=0, wrow_scale=None,
                 arow_scale=None):
        self.M, self.N, self.cin, self.taps, self.dil, self.K = M, N, cin, taps, dil, cin * taps
        self.T = -(-M // G)
        self.segT = 0 if (G == 1 and H == 0) else self.T
        self.a_skip = H if self.segT else 0
        a_rows = (M - 1) + ((M - 1) // self.segT * H if self.segT else 0) + (taps - 1) * dil + 3
        lda = cin + 4
        if arow_scale is None:
            vals = rng.standard_normal((a_rows, cin)).astype(np.float32)
        else:
            vals = (rng.uniform(-1, 1, (a_rows, cin)) * arow_scale(a_rows)[:, None]).astype(np.float32)
        self.a_split = a_split
        if a_split:
            A = np.zeros((a_rows, lda), np.uint32)
            A[:, :cin] = R.split_rows(vals)
            self.A, self.A_val = A, R.unsplit_rows(A, cin)[2]
        else:
            A = rng.standard_normal((a_rows, lda)).astype(np.float32)
            A[:, :cin] = vals
            self.A, self.A_val = A, vals.astype(np.float64)
        W = rng.standard_normal((N, self.K)) / np.sqrt(self.K)
        if wrow_scale is not None:
            W = W * wrow_scale(N)[:, None]
        self.W = W.astype(np.float32)
        pad = out_pad if out_pad is not None else (4 if N % 4 == 0 else 3)
        self.ldo = N + pad
        self.o_segT = self.T if G > 1 else 0
        self.o_skip = OH * self.ldo if self.o_segT else 0
        self.out_off = OH * self.ldo + out_misalign
        m = M - 1
        self.out_floats = self.out_off + m * self.ldo + (m // self.o_segT * self.o_skip if self.o_segT else 0) + N + 2 * self.ldo
        self.idx = R.out_index(M, N, self.ldo, self.out_off, self.o_segT, self.o_skip)
        self._ref = None

    def ref(self):
        if self._ref is None:
            self._ref = R.gemm_ref(self.A_val, self.W, self.M, self.cin, self.taps, self.dil, self.segT, self.a_skip)
        return self._ref

    def run(self, q3, form="AUTO", ksplit=1, reducer=-1, ws_floats=1 << 22, **kw):
        buf = np.full(self.out_floats, SENTINEL, np.uint32).view(np.float32)
        out, info = q3.op_codec_gemm(self.A, self.W, self.M, self.cin, self.taps, self.dil, out=buf, ldo=self.ldo, out_off=self.out_off,
                                     o_segT=self.o_segT, o_skip=self.o_skip, a_segT=self.segT, a_skip=self.a_skip, a_split=self.a_split,
                                     ws_floats=ws_floats, form=form, ksplit=ksplit, reducer=reducer, **kw)
        bits = out.view(np.uint32)
        outside = np.ones(self.out_floats, bool)
        outside[self.idx.ravel()] = False
        bad = np.flatnonzero(outside & (bits != SENTINEL))
        assert bad.size == 0, "%s wrote %d floats outside the logical output, first at %s" % (info, bad.size, bad[:8])
        return out[self.idx], info, bits


@pytest.mark.parametrize("case", R.FORCED_CASES, ids=lambda c: "%s-M%d-N%d-cin%d-k%dd%d-G%dH%d-ks%d-r%d%s" % (c[:10] + ("-split" if c[10] else "",)))
def test_forced_form_matches_float64(gpu, case):
    form, M, N, cin, taps, dil, G, H, ks, red, a_split = case
    rng = np.random.default_rng(R.FORCED_CASES.index(case))
    p = Problem(rng, M, N, cin, taps, dil, G, H, a_split)
    out, info, _ = p.run(gpu, form, ks, red)
    assert info == (form, ks, red)
    ref, absb = p.ref()
    err = np.abs(out.astype(np.float64) - ref)
    bar = R.shape_bar(p.K) * absb + 2.0 ** -22 * np.abs(ref)
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    assert np.all(err <= bar), "row %d col %d: |err| %.3g > bar %.3g (normalised %.3g)" % (worst + (err[worst], bar[worst], err[worst] / absb[worst]))


# one shape per kernel family for the epilogue checks: (form, M, N, cin, taps, dil, G, H, ksplit, reducer)
EPI_FORMS = [("SKINNY8", 7, 100, 64, 7, 3, 3, 6, 1, -1), ("F32_1", 31, 100, 64, 2, 1, 3, 1, 2, 0), ("F32_2", 65, 68, 32, 7, 1, 16, 18, 2, 1),
             ("H1", 65, 100, 64, 7, 9, 3, 54, 1, -1), ("H1_EPL", 65, 100, 64, 7, 1, 3, 6, 2, 1), ("H2", 129, 100, 96, 2, 1, 16, 1, 2, 0),
             ("H2_EPL", 129, 68, 64, 7, 3, 3, 18, 1, -1), ("H3", 129, 96, 64, 7, 1, 3, 6, 1, -1), ("H3_EPL", 129, 192, 64, 2, 1, 16, 1, 2, 1)]


@pytest.mark.parametrize("fc", EPI_FORMS, ids=lambda c: c[0])
def test_epilogues_isolated(gpu, fc):
    form, M, N, cin, taps, dil, G, H, ks, red = fc
    rng = np.random.default_rng(7 + len(form) * 131 + M)
    p = Problem(rng, M, N, cin, taps, dil, G, H)
    acc, info, _ = p.run(gpu, form, ks, red)
    assert info == (form, ks, red)
    bias = rng.standard_normal(N).astype(np.float32) * 0.5
    scale = rng.uniform(-2, 2, N).astype(np.float32)
    ea = rng.uniform(0.5, 2.0, N).astype(np.float32)
    ib = rng.uniform(0.25, 1.0, N).astype(np.float32)
    # segmented residual rows with their own history rows and ldr > N
    ldr, RH = N + 4, 5
    r_segT, r_skip = p.T, RH * ldr
    res_idx = R.out_index(M, N, ldr, 0, r_segT, r_skip)
    res = rng.standard_normal(res_idx.max() + 1 + ldr).astype(np.float32)
    res_rows = res[res_idx].astype(np.float64)
    v = acc.astype(np.float64) + bias.astype(np.float64)
    kw = dict(bias=bias, res=res, ldr=ldr, r_segT=r_segT, r_skip=r_skip, scale=scale, ea=ea, ib=ib)
    for epi in (R.EPI_NONE, R.EPI_GELU, R.EPI_RES_SCALE, R.EPI_RES, R.EPI_SNAKE):
        out, info, _ = p.run(gpu, form, ks, red, epi=epi, **kw)
        assert info == (form, ks, red)
        ref = R.epilogue(acc, epi, bias, res_rows, scale, ea, ib)
        mag = np.maximum(np.abs(ref), np.abs(v))
        if epi in (R.EPI_RES, R.EPI_RES_SCALE):
            mag = np.maximum(mag, np.abs(res_rows))
        if epi == R.EPI_RES_SCALE:
            mag = np.maximum(mag, np.abs(scale * v))
        tol = 4 * _ulp(mag) + (2e-7 if epi in (R.EPI_GELU, R.EPI_SNAKE) else 0.0)
        err = np.abs(out.astype(np.float64) - ref)
        assert np.all(err <= tol), "epi %d: max err %.3g (tol there %.3g)" % (epi, err.max(), tol.ravel()[np.argmax(err - tol)])
        if epi in (R.EPI_NONE, R.EPI_SNAKE):   # the pre-split output of the same values: hi = f16(v), lo = f16(v - hi), bit for bit
            sp, info, _ = p.run(gpu, form, ks, red, epi=epi, o_split=True, **kw)
            hi, lo, _ = R.unsplit_rows(sp.view(np.uint32), N)
            ehi, elo = R.f16_split(out)
            assert np.array_equal(hi.view(np.uint16), ehi.view(np.uint16)) and np.array_equal(lo.view(np.uint16), elo.view(np.uint16)), epi


# AUTO (the decoder's dispatch) runs exactly the form it reports, deterministically: (M, N, cin, taps, dil, G, H, out_misalign, ws_floats)
AUTO_SHAPES = [(4, 1024, 512, 3, 1, 1, 2, 0, 1 << 20), (12, 3072, 1024, 1, 1, 1, 0, 0, 1 << 20), (32, 1536, 1024, 7, 1, 4, 6, 0, 1 << 20),
               (64, 768, 768, 2, 1, 4, 1, 0, 1 << 20), (64, 100, 64, 7, 3, 4, 18, 0, 1 << 20), (256, 96, 96, 7, 9, 16, 54, 0, 1 << 20),
               (2048, 768, 96, 7, 1, 16, 6, 0, 1 << 22), (2048, 640, 64, 2, 1, 16, 1, 0, 1 << 22), (2048, 640, 64, 2, 1, 16, 1, 1, 1 << 22),
               (512, 192, 192, 7, 3, 16, 18, 1, 1 << 16), (128, 384, 384, 1, 1, 16, 0, 0, 1 << 20)]


@pytest.mark.parametrize("shape", AUTO_SHAPES)
def test_auto_equals_the_form_it_reports(gpu, shape):
    M, N, cin, taps, dil, G, H, mis, ws = shape
    rng = np.random.default_rng(M * 7 + N)
    p = Problem(rng, M, N, cin, taps, dil, G, H, out_misalign=mis)
    bias = rng.standard_normal(N).astype(np.float32)
    a, info, abits = p.run(gpu, "AUTO", ws_floats=ws, bias=bias)
    b, info_b, bbits = p.run(gpu, "AUTO", ws_floats=ws, bias=bias)
    assert info == info_b and np.array_equal(abits, bbits), "two identical AUTO calls differ"
    f, info_f, fbits = p.run(gpu, info[0], info[1], info[2], ws_floats=ws, bias=bias)
    assert info_f == info and np.array_equal(abits, fbits), "AUTO (%s) differs from the forced form it reports" % (info,)
    assert info == gpu.codec_gemm_plan(M, N, cin, taps, dil, lda=cin + 4, ldo=p.ldo, out_off=p.out_off, o_segT=p.o_segT, o_skip=p.o_skip,
                                       a_segT=p.segT, a_skip=p.a_skip, ws_floats=ws)   # the host-only plan agrees with what ran


def precision_sweep(q3, form, ks=1, red=-1):
    """split-f16 contract over scales: weight rows 2^-20 .. 2^12 (neighbouring rows 2^10 apart), activation rows 2^-10 .. 2^13.
    Returns (ok, {weight-row exponent: max |err| / sum|a||w|}, worst bar ratio)"""
    rng = np.random.default_rng(11)
    N = 192 if form.startswith("H3") else 160
    M = 16 if form.startswith("SKINNY") else 192
    e_w = np.linspace(-20, 12, N // 2).round().astype(int)
    e_pair = np.where(e_w + 10 <= 12, e_w + 10, e_w - 10)
    ew = np.stack([e_w, e_pair], axis=1).ravel()
    p = Problem(rng, M, N, 128, 7, 1, 1, 0, wrow_scale=lambda n: np.exp2(ew[:n]),
                arow_scale=lambda r: np.exp2(np.linspace(-10, 13, r)))
    out, info, _ = p.run(q3, form, ks, red)
    assert info == (form, ks, red)
    ref, absb = p.ref()
    err = np.abs(out.astype(np.float64) - ref)
    sw = np.abs(p.W.astype(np.float64)).sum(axis=1)[None, :]
    bar = R.shape_bar(p.K) * absb + 2.0 ** -25 * sw
    per_scale = {}
    nerr = err / absb
    for e in sorted(set(ew.tolist())):
        per_scale[e] = float(nerr[:, ew == e].max())
    return bool(np.all(err <= bar)), per_scale, float((err / bar).max())


@pytest.mark.parametrize("form,ks,red", [("H1", 1, -1), ("H1_EPL", 2, 1), ("H2", 2, 0), ("H2_EPL", 1, -1), ("H3", 1, -1), ("H3_EPL", 7, 1),
                                         ("F32_2", 2, 0), ("SKINNY16", 1, -1)])
def test_split_f16_precision_contract(gpu, form, ks, red):
    ok, per_scale, worst = precision_sweep(gpu, form, ks, red)
    assert ok, "%s: |err| / bar up to %.3g; max |err| / sum|a||w| per weight-row exponent: %s" % (
        form, worst, {k: "%.2g" % v for k, v in per_scale.items()})


def _refused(q3, p, **kw):
    with pytest.raises(q3.Q3Error, match="not applicable"):
        p.run(q3, **kw)


def test_illegal_forced_forms_are_refused(gpu):
    rng = np.random.default_rng(3)
    p16 = Problem(rng, 128, 96, 16, 7, 1)      # cin % 32 != 0
    _refused(gpu, p16, form="H1")
    _refused(gpu, p16, form="H3_EPL")
    p = Problem(rng, 128, 100, 64, 7, 1)       # K = 448, N % 96 != 0
    _refused(gpu, p, form="H3")
    _refused(gpu, p, form="H1", ksplit=4, reducer=0)           # K / 4 = 112: not a multiple of 32
    _refused(gpu, p, form="H1", ksplit=3, reducer=0)           # 3 does not divide K
    _refused(gpu, p, form="F32_2", ksplit=2, reducer=0, ws_floats=128 * 100)   # workspace holds one slab
    _refused(gpu, p, form="H1", ksplit=2, reducer=-1)          # split-K without a reducer
    _refused(gpu, p, form="H1", ksplit=1, reducer=0)           # a reducer without split-K
    _refused(gpu, p, form="SKINNY16")                          # M > 16
    _refused(gpu, p, form=12)                                  # no such form
    pm = Problem(rng, 128, 100, 64, 7, 1, out_misalign=1)      # output not 16-byte aligned
    _refused(gpu, pm, form="H1_EPL")
    _refused(gpu, pm, form="H2", ksplit=2, reducer=1)
    po = Problem(rng, 128, 99, 64, 7, 1)                       # N % 4 != 0
    _refused(gpu, po, form="H2_EPL")
    _refused(gpu, po, form="F32_2", ksplit=2, reducer=1)
    ps = Problem(rng, 5, 64, 64, 1, 1)
    _refused(gpu, ps, form="SKINNY4")
    _refused(gpu, ps, form="SKINNY8", ksplit=2, reducer=0)
    _refused(gpu, Problem(rng, 64, 64, 8, 1, 1), form="F32_1")   # cin % 16 != 0
    # and nothing was left behind: a legal call still runs and is correct
    out, info, _ = p.run(gpu, "H1", 2, 0)
    ref, absb = p.ref()
    assert info == ("H1", 2, 0) and np.all(np.abs(out - ref) <= R.shape_bar(p.K) * absb + 2.0 ** -22 * np.abs(ref))
