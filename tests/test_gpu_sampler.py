"""The token-selection kernels -- k_sample, k_sample_pred, k_argmax, k_argmax_keys -- through q3tts_op_select_rows, at every width, stride
and edge of tests/sampler_cases.py.  The yardstick is LlamaSampler::sample (llama/mod.rs:666-776) as q3oracle.sample states it, or
tests/sampler_ref.py where a stream starts past word 0; tests/test_sampler_cases_cpu.py holds those two and the host sampler against each
other on the same cases.  Every comparison is equality of integers: there is no tolerance anywhere in this file.

The op entry keeps 3e38 in every logits column a kernel must not read and a fixed pattern in every output slot it must not write, so a kernel
that strays changes its pick or trips _check_slots."""
import numpy as np
import pytest

import sampler_cases as SC
import sampler_ref as SR

pytestmark = pytest.mark.gpu
ND = SC.N_DRAWS
_WANT = {}


def _want(oracle, case, cfgs):
    """[len(cfgs)][ND] reference tokens of one case, computed once and shared"""
    key = (case.name, case.n, case.mask, len(cfgs))
    if key not in _WANT:
        row, out = case.masked_row(), []
        for T, k, p, draw0, seed in cfgs:
            if draw0 == 0:
                st = None
                toks = []
                for _ in range(ND):
                    t, st = oracle.sample(row, 0, row.size, T, k, p, seed, state=st)
                    toks.append(t)
            else:
                toks = case.ref().sample(T, k, p, seed, draw0, ND)
            out.append(toks)
        arr = np.array(out, np.int32)
        arr.setflags(write=False)
        _WANT[key] = arr
    return _WANT[key]


def _check_slots(q3, tokens, raw, out_stride, keys=True):
    """slot b*out_stride of every launch holds pack_key(0, token) (int32 token for k_argmax); every other slot still holds the sentinel"""
    nl, B = tokens.shape
    raw = raw.reshape(nl, B, out_stride)
    sent = q3.SELECT_SENTINEL if keys else q3.SELECT_SENTINEL & 0xFFFFFFFF
    assert (raw[:, :, 1:] == np.uint64(sent)).all(), "a slot between two outputs was written"
    if keys:
        want = (np.uint64(0x80000000) << np.uint64(32)) | (~tokens.astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)
        assert np.array_equal(raw[:, :, 0], want), "an output key is not pack_key(0, token)"


def _run_sampler(q3, kernel, case, cfgs, want, stride, row_off, out_stride, mask=False):
    for lo in range(0, len(cfgs), 64):
        cf = cfgs[lo:lo + 64]
        B = len(cf)
        T = np.array([c[0] for c in cf], np.float32)
        d0 = np.array([c[3] for c in cf], np.uint32)
        tok, raw, draws = q3.op_select_rows(kernel, np.tile(case.row if mask else case.masked_row(), (B, 1)), stride=stride, row_off=row_off,
                                            temperature=T, top_k=[c[1] for c in cf], top_p=[c[2] for c in cf], seed=[c[4] for c in cf], draw0=d0,
                                            mask_idx=np.full(B, case.mask, np.int32) if mask else None, n_draws=ND, out_stride=out_stride)
        bad = np.argwhere(tok.T != want[lo:lo + B])
        assert bad.size == 0, (case.name, case.n, stride, [(cf[b][:4], int(d), int(tok[d, b]), int(want[lo + b, d])) for b, d in bad[:4]])
        assert np.array_equal(draws, d0 + np.where(T > 0, ND, 0).astype(np.uint32)), (case.name, "draw counters")
        _check_slots(q3, tok, raw, out_stride)


@pytest.mark.parametrize("n", SC.PRED_NS)
def test_sample_pred(gpu, oracle, n):
    """k_sample_pred == the reference on every family, grid value and stride; k_sample on the same rows gives the same tokens"""
    for ci, case in enumerate(SC.sampling_cases(n)):
        cfgs = SC.configs(n, case.extra_top_k, ci)
        want = _want(oracle, case, cfgs)
        for si, stride in enumerate(SC.strides(n)):
            _run_sampler(gpu, gpu.SEL_SAMPLE_PRED, case, cfgs, want, stride, (0, 3, 1)[si], (1, 16, 1)[si])
        _run_sampler(gpu, gpu.SEL_SAMPLE, case, cfgs, want, SC.strides(n)[1], 1, 16)


@pytest.mark.parametrize("n", SC.TALK_NS)
def test_sample(gpu, oracle, n):
    """k_sample == the reference on every family, grid value and stride, without a mask and with the row's first maximum masked"""
    for ci, case in enumerate(SC.sampling_cases(n)):
        cfgs = SC.configs(n, case.extra_top_k, ci)
        want = _want(oracle, case, cfgs)
        for si, stride in enumerate(SC.strides(n)):
            _run_sampler(gpu, gpu.SEL_SAMPLE, case, cfgs, want, stride, (0, 3, 1)[si], (1, 16, 1)[si])
        masked = SC.Case(case.name, case.row, case.extra_top_k, mask=SR.greedy(case.row))
        _run_sampler(gpu, gpu.SEL_SAMPLE, masked, cfgs, _want(oracle, masked, cfgs), SC.strides(n)[2], 2, 1, mask=True)


PEN_CFG = ((0.0, 0, 1.0), (0.9, 50, 0.8), (1.3, 0, 1.0), (0.05, 2, 0.5))


@pytest.mark.parametrize("n", [33, 2160])
def test_sample_penalty(gpu, oracle, n):
    """penalise (every distinct history code inside [0, n) once), then the mask, then the sampler: the kernel's order"""
    rng = np.random.default_rng(n)
    lg = (rng.standard_normal(n) * 3).astype(np.float32)
    top = SR.greedy(lg)
    iz, inz, ininf, ineg, imask = [int(i) for i in np.setdiff1d(rng.permutation(n), [top], assume_unique=True)[:5]]
    lg[iz], lg[inz], lg[ininf], lg[ineg] = 0.0, -0.0, -np.inf, -2.5
    kinds = {
        "dups": [top, ineg, top, top, ineg, 7, 7],
        "out_of_range": [n, n + 5, 4095, 4096, 70000, 2 ** 31 - 1, -1, -7, -2 ** 31, top],
        "zeros_and_inf": [iz, inz, ininf, ineg],
        "masked_in_history": [imask, top, ineg],
        "long_1500": [int(c) for c in rng.integers(0, n, 1497)] + [top, n, -1],     # more codes than k_sample has threads
        "empty": [],
    }
    assert len(kinds["long_1500"]) == 1500
    for with_cur in (True, False):
        names = [k for k in kinds if with_cur or kinds[k]]
        rows = [(k, pen, cfg) for k in names for pen in (0.7, 1.0, 1.5) for cfg in PEN_CFG]
        for lo in range(0, len(rows), 64):
            part = rows[lo:lo + 64]
            B = len(part)
            cur = [top if k in ("empty", "zeros_and_inf") else (n + 1 if k == "dups" else ineg) for k, _, _ in part]
            mask = np.array([imask if k == "masked_in_history" else (top if k == "dups" else -1) for k, _, _ in part], np.int32)
            seed = np.arange(B, dtype=np.uint64) * 977 + 5 + lo
            tok, raw, draws = gpu.op_select_rows(gpu.SEL_SAMPLE, np.tile(lg, (B, 1)), stride=n + 1, row_off=1, temperature=[c[0] for _, _, c in part],
                                                 top_k=[c[1] for _, _, c in part], top_p=[c[2] for _, _, c in part], seed=seed, n_draws=ND,
                                                 mask_idx=mask, penalty=[p for _, p, _ in part], history=[kinds[k] for k, _, _ in part],
                                                 cur_code=cur if with_cur else None, out_stride=16)
            _check_slots(gpu, tok, raw, 16)
            live = False
            for b, (k, pen, (T, tk, tp)) in enumerate(part):
                hist = [c for c in kinds[k] + ([cur[b]] if with_cur else []) if 0 <= c < n]
                ref = SR.penalise(lg, hist, pen)
                if mask[b] >= 0:
                    ref[mask[b]] = -np.inf
                st, want = None, []
                for _ in range(ND):
                    t, st = oracle.sample(ref, 0, n, T, tk, tp, int(seed[b]), state=st)
                    want.append(t)
                assert list(tok[:, b]) == want, (k, pen, T, tk, tp, with_cur)
                base = lg.copy()
                if mask[b] >= 0:
                    base[mask[b]] = -np.inf
                live = live or not np.array_equal(ref.view(np.uint32), base.view(np.uint32))
            assert live


GREEDY_NS = (1, 2, 33, 255, 256, 257, 1000, 2047, 2048, 2160, 4095, 4096)


@pytest.mark.parametrize("n", GREEDY_NS)
def test_greedy_forms(gpu, n):
    """k_argmax (three windows), k_argmax_keys, k_sample and k_sample_pred at T = 0 return the reference's first maximum on the same rows"""
    cases = SC.greedy_cases(n)
    B = len(cases)
    rows = np.stack([c.row for c in cases])
    pre = np.stack([c.masked_row() for c in cases])
    mask = np.array([c.mask for c in cases], np.int32)
    want = np.array([SR.greedy(r) for r in pre], np.int32)
    all_inf = np.array([np.isneginf(r).all() for r in pre])
    assert all_inf.sum() >= (2 if n > 1 else 1) and (want[all_inf] == 0).all()
    for si, stride in enumerate(SC.strides(n)):
        off, os_ = (0, 3, 1)[si], (1, 16, 16)[si]
        for start, end, add in SC.ARGMAX_WINDOWS(n):
            if not 0 <= start <= end <= n:
                continue
            tok, raw, _ = gpu.op_select_rows(gpu.SEL_ARGMAX, rows, stride=stride, row_off=off, mask_idx=mask, start=start, end=end, add=add, out_stride=os_)
            ref = np.array([SR.greedy(r, start, end) + add for r in pre], np.int32)
            assert np.array_equal(tok[0], ref), (n, stride, start, end, add, [c.name for c, a, b in zip(cases, tok[0], ref) if a != b])
            assert (ref[all_inf] == start + add).all()
            _check_slots(gpu, tok, raw, os_, keys=False)
        tok, raw, _ = gpu.op_select_rows(gpu.SEL_ARGMAX_KEYS, rows, stride=stride, row_off=off, mask_idx=mask, out_stride=os_)
        assert np.array_equal(tok[0], want), (n, stride, "k_argmax_keys", [c.name for c, a, b in zip(cases, tok[0], want) if a != b])
        keys = raw.reshape(B, os_)
        assert (keys[:, 1:] == np.uint64(gpu.SELECT_SENTINEL)).all()
        for b in range(B):                                          # the key carries the winning value; an all -inf row keeps pack_key(-inf, 0)
            assert int(keys[b, 0]) == SC.pack_key(pre[b, want[b]], want[b]), cases[b].name
        samplers = [(gpu.SEL_SAMPLE, rows, mask)] + ([(gpu.SEL_SAMPLE_PRED, pre, None)] if n <= 2048 else [])
        for kernel, lg, mk in samplers:
            tok, raw, draws = gpu.op_select_rows(kernel, lg, stride=stride, row_off=off, temperature=0.0, top_k=[0, 40][si % 2], top_p=[1.0, 0.9][si % 2],
                                                 mask_idx=mk, seed=7, draw0=np.arange(B, dtype=np.uint32), n_draws=2, out_stride=os_)
            assert np.array_equal(tok, np.stack([want, want])), (n, stride, kernel, [c.name for c, a, b in zip(cases, tok[0], want) if a != b])
            assert np.array_equal(draws, np.arange(B, dtype=np.uint32))
            _check_slots(gpu, tok, raw, os_)


@pytest.mark.parametrize("kernel,n", [(0, 2160), (1, 2048), (1, 1000)])
def test_side_effects_mixed_launch(gpu, oracle, kernel, n):
    """B = 64 with every fourth row greedy: sampled rows advance their draw counter by exactly n_draws, greedy rows leave it alone, and no
    output slot but b*16 is written"""
    rng = np.random.default_rng(5 + n)
    B, nd = 64, 20
    lg = (rng.standard_normal((B, n)) * 3).astype(np.float32)
    T = np.where(np.arange(B) % 4 == 3, 0.0, 0.9).astype(np.float32)
    d0 = rng.integers(0, 2 ** 20, B).astype(np.uint32)
    d0[:4] = (2 ** 32 - 21, 15, 16, 0)
    seed = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    tok, raw, draws = gpu.op_select_rows(kernel, lg, stride=n + 16, temperature=T, top_k=50, top_p=0.8, seed=seed, draw0=d0, n_draws=nd, out_stride=16)
    assert np.array_equal(draws, d0 + np.where(T > 0, nd, 0).astype(np.uint32))
    _check_slots(gpu, tok, raw, 16)
    for b in range(B):
        assert list(tok[:, b]) == SR.sample(lg[b], T[b], 50, 0.8, seed[b], int(d0[b]), nd), b


@pytest.mark.parametrize("kernel,n", [(0, 300), (1, 257)])
def test_b256_launch_equals_single_rows(gpu, kernel, n):
    rng = np.random.default_rng(11 + n)
    B, nd = 256, 2
    lg = (rng.standard_normal((B, n)) * 3).astype(np.float32)
    lg[rng.integers(0, B, 40), rng.integers(0, n, 40)] = -np.inf
    cfg = [SC.configs(n)[i % len(SC.configs(n))] for i in range(B)]
    kw = lambda s: dict(temperature=[c[0] for c in cfg[s]], top_k=[c[1] for c in cfg[s]], top_p=[c[2] for c in cfg[s]],
                        draw0=np.array([c[3] for c in cfg[s]], np.uint32), seed=[c[4] for c in cfg[s]])
    tok, raw, draws = gpu.op_select_rows(kernel, lg, stride=n + 1, n_draws=nd, **kw(slice(0, B)))
    _check_slots(gpu, tok, raw, 1)
    for b in range(B):
        t1, _, d1 = gpu.op_select_rows(kernel, lg[b:b + 1], stride=n + 1, n_draws=nd, **kw(slice(b, b + 1)))
        assert np.array_equal(t1[:, 0], tok[:, b]) and d1[0] == draws[b], b


def test_refusals_leave_outputs_untouched(gpu):
    lg = lambda n: np.zeros((2, n), np.float32)
    bad = [dict(kernel=gpu.SEL_SAMPLE_PRED, logits=lg(64), penalty=1.1, history=[[1], [2]]),
           dict(kernel=gpu.SEL_SAMPLE_PRED, logits=lg(64), mask_idx=3),
           dict(kernel=gpu.SEL_SAMPLE_PRED, logits=lg(2049)),
           dict(kernel=gpu.SEL_SAMPLE, logits=lg(4097))]
    for kw in bad:
        out = gpu.select_outputs(2, 3, 16)
        with pytest.raises(gpu.Q3Error):
            gpu.op_select_rows(temperature=0.9, seed=1, n_draws=3, out_stride=16, outputs=out, **kw)
        fresh = gpu.select_outputs(2, 3, 16)
        assert all(np.array_equal(a, b) for a, b in zip(out, fresh)), kw["kernel"]
    ok = dict(bad[2], logits=lg(2048))                              # the same call inside the limit runs and writes all three
    out = gpu.select_outputs(2, 3, 16)
    gpu.op_select_rows(temperature=0.9, seed=1, n_draws=3, out_stride=16, outputs=out, **ok)
    assert (out[0] >= 0).all() and (out[2] == 3).all()
