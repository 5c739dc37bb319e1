"""Every attention form (k_qk_rope_append + k_attention, k_attention_fused, k_attention_short<1|2>, the ggml-mode pair), forced through
q3tts_op_attention on synthetic problems (tests/attention_cases.py; no model weights): bit for bit against the oracle's per-head S4'/S5/S7/S2
(q3o_head_rope, q3o_attn_head / q3o_attn_head_ggml, q3o_quant_act), against a float64 reference within a bound derived from the
arithmetic (tests/attention_ref.py), against each other, with every f16 the launch must not read set to NaN, and with every cache byte
outside the appended rows unchanged.  Illegal forced forms are refused.  Positions outside [0, n_ctx) are clamped to the RoPE table's
ends (pinned by the mrope_clamp case).  (-m gpu)"""
import numpy as np
import pytest

import attention_cases as AC
import attention_ref as R
from attention_cases import expect, check_f64

pytestmark = pytest.mark.gpu

CASES = AC.all_cases()
S7_FORMS = ("UNFUSED", "FUSED", "SHORT1", "SHORT2")
def run(q3, P, form, poison=True, **flags):
    args, kw = P.op_args(poison)
    kin, vin = args[3].copy(), args[4].copy()
    r = q3.op_attention(*args, form=form, **kw, **flags)
    return r, kin, vin


def _same(a, b, what):
    assert a is not None and b is not None and np.array_equal(a, b), what


@pytest.mark.parametrize("P", CASES, ids=[P.name for P in CASES])
def test_attention_forms(gpu, oracle, P):
    forms = AC.forms_for(P)
    exp = {}
    results = {}
    for form in forms:
        ggml = form == "GGML"
        r, kin, vin = run(gpu, P, form)
        assert r["form"] == form
        if ggml not in exp:
            exp[ggml] = expect(oracle, P, ggml, kin, vin)
        e = exp[ggml]
        # bit-exact against the oracle, every cache byte included (appended rows = the oracle's, everything else = the input)
        if r["att"] is not None:
            _same(r["att"].view(np.uint32), e["att"].view(np.uint32), (P.name, form, "att"))
        if not ggml:
            _same(r["aq"], e["aq"], (P.name, form, "aq"))
            _same(r["ad"], e["ad"], (P.name, form, "ad"))
        _same(r["k_cache"], e["k_cache"], (P.name, form, "K cache"))
        _same(r["v_cache"], e["v_cache"], (P.name, form, "V cache"))
        # poison: nothing the launch must not read was read
        c, _, _ = run(gpu, P, form, poison=False)
        for key in ("att", "aq", "ad"):
            if r[key] is not None:
                assert np.all(np.isfinite(r[key])) and np.array_equal(r[key], c[key]), (P.name, form, key, "differs from the clean-cache run")
        worst, rel = check_f64(P, form, r)
        if r["att"] is not None:
            print("F64 %-8s %-16s max|y-y64|/sum(p|v|) = %.3e  (%.3f of the bound)" % (form, P.name, worst, rel))
        results[form] = r
    # where preconditions overlap, the S7 forms agree bit for bit
    s7 = [f for f in forms if f in S7_FORMS]
    for f in s7[1:]:
        for key in ("aq", "ad", "k_cache", "v_cache"):
            _same(results[f][key], results[s7[0]][key], (P.name, f, s7[0], key))
        if results[f]["att"] is not None and results["UNFUSED"]["att"] is not None:
            _same(results[f]["att"].view(np.uint32), results["UNFUSED"]["att"].view(np.uint32), (P.name, f, "att"))


AUTO = [  # (case, flags, the form plan_attention must pick)
    ("ntok7", dict(fused=True, fused_max_tok=8, short_attn_min=0), "FUSED"),
    ("ntok9", dict(fused=True, fused_max_tok=8, short_attn_min=0), "UNFUSED"),
    ("ntok64", dict(fused=True, fused_max_tok=8, short_attn_min=8), "SHORT1"),
    ("ntok129", dict(fused=True, fused_max_tok=8, short_attn_min=8), "SHORT2"),
    ("short_uniform17", dict(fused=True, fused_max_tok=8, short_attn_min=2), "SHORT1"),
    ("short_uniform17", dict(fused=True, fused_max_tok=8, short_attn_min=2, hpw1_max=4), "SHORT2"),
    ("prefill", dict(fused=True, fused_max_tok=64, same_seq=True, short_attn_min=8), "UNFUSED"),
    ("ntok7", dict(float_mode=True, short_attn_min=0), "UNFUSED"),
    ("ntok9", dict(float_mode=True, short_attn_min=8), "SHORT1"),
    ("ctx17", dict(ggml_mode=True), "GGML"),
]


@pytest.mark.parametrize("name,flags,want", AUTO, ids=["%s-%s" % (a[0], a[2]) for a in AUTO])
def test_auto_is_the_form_it_reports(gpu, name, flags, want):
    P = next(p for p in CASES if p.name == name)
    a, _, _ = run(gpu, P, "AUTO", **flags)
    assert a["form"] == want
    f, _, _ = run(gpu, P, want)
    for key in ("att", "aq", "ad", "k_cache", "v_cache"):
        if f[key] is None:
            assert a[key] is None
        else:
            assert np.array_equal(a[key].view(np.uint8), f[key].view(np.uint8)), key


def _refuse(q3, P, form, **over):
    args, kw = P.op_args(True)
    kin, vin = args[3].copy(), args[4].copy()
    kw.update(over)
    with pytest.raises(q3.Q3Error):
        q3.op_attention(*args, form=form, **kw)
    assert np.array_equal(args[3], kin) and np.array_equal(args[4], vin)


def test_refused_forms(gpu):
    by = {p.name: p for p in CASES}
    # n_head not a multiple of n_kv (the qkv rows are wide enough for 12 + 2 * 8 heads)
    _refuse(gpu, by["ctx17"], "UNFUSED", n_head=12)
    _refuse(gpu, by["ctx17"], "GGML", n_head=12)
    # two tokens of one sequence in a fused or short launch
    for f in ("FUSED", "SHORT1", "SHORT2"):
        _refuse(gpu, by["prefill_identity"], f)
    # the short forms: n_head != 2 n_kv, a slot beyond page 0
    for f in ("SHORT1", "SHORT2"):
        _refuse(gpu, by["short_mixed"], f, n_head=8)        # 8 q heads on 8 kv heads (every slot < 64)
        _refuse(gpu, by["short_mixed"], f, n_head=32)       # 32 on 8 (the rows are too narrow as well)
        _refuse(gpu, by["ctx65"], f)
    # a slot beyond the page table, a page entry out of range, identity paging beyond one page, a slot beyond n_ctx
    P = by["ctx65"]
    for f in AC.forms_for(P):
        _refuse(gpu, P, f, slot=np.array([P.table.shape[1] * 64], np.int32))
        bad = P.table.copy()
        bad[0, -1] = P.n_pages
        _refuse(gpu, P, f, page_table=bad)
        _refuse(gpu, P, f, page_table=None)
        _refuse(gpu, P, f, n_ctx=64)
    # the predictor's uniform form: token t = sequence t must have a page
    _refuse(gpu, by["short_uniform17"], "SHORT1", uniform_pos=64)


def test_mrope_clamp(gpu, oracle):
    """positions outside [0, n_ctx) rotate as the nearest table end (the kernels' and the oracle's clamp)"""
    P = next(p for p in CASES if p.name == "mrope_clamp")
    Q = AC.Problem("mrope_clamp_in", 94, [(10, 1), (33, 1)], pos=lambda t, s: [4095, 0, 4095, 4095], sec=(16, 8, 8, 0))
    assert np.array_equal(P.qkv, Q.qkv)
    for form in ("UNFUSED", "FUSED", "GGML"):
        a, _, _ = run(gpu, P, form)
        b, _, _ = run(gpu, Q, form)
        for key in ("att", "aq", "ad", "k_cache", "v_cache"):
            if a[key] is not None:
                assert np.array_equal(a[key], b[key]), (form, key)


def test_engine_predictor_short2(gpu, tiny_model, vivian):
    """132 slots: the code predictor's passes run k_attention_short<2> (> 128 tokens); every slot's codes equal a 2-slot engine's"""
    assert gpu.attention_plan(132, n_head=2, n_kv=1, short_attn_min=8) == "SHORT2"
    rng = np.random.default_rng(132)
    ge = gpu.Engine(tiny_model, "q8_0", max_batch=132, max_steps=8, load_codec=False)
    prompts = [ge.assets.build_core(rng.integers(0, 4000, 3 + i % 11).astype(np.int32), lang_id=2055, spk_emb=vivian) for i in range(132)]
    wide = ge.generate_batch(prompts, max_steps=5, seed=list(range(132)), mask_eos=True)
    ge.close()
    two = gpu.Engine(tiny_model, "q8_0", max_batch=2, max_steps=8, load_codec=False)
    narrow = two.generate_batch(prompts, max_steps=5, seed=list(range(132)), mask_eos=True)
    two.close()
    for i, (a, b) in enumerate(zip(wide, narrow)):
        assert a["codes"].shape[0] > 0 and np.array_equal(a["codes"], b["codes"]), i
