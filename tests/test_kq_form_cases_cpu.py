"""Host-only checks of tests/kq_form_cases.py, the case table of tests/test_gpu_kq_forms.py: what the table covers (a deleted case fails here,
it does not thin the GPU test), that the engine's dispatch (q3tts_linear_plan) launches nothing on a full-size K-quant model that the table
leaves out, and that the references of the table's shapes are sound on their own: the oracle's result on the twin rows lies within the float64
bound the GPU test uses, and the copied-row ties of the argmax cases are what they are built to be.  No GPU needed."""
import itertools

import numpy as np
import pytest

import kq_form_cases as C
import kq_ref as KR
import linear_ref as R
import q3tts as Q
from test_linear_plan_cpu import _full_dims

SINGLES = [(t,) for t in C.SINGLE]
MIX = list(C.MIXTURES)
PAIRS = set(itertools.product(C.LPRS, C.MTS))


def _of(form, types=None, **where):
    return [c for c in C.CASES if c.form == form and (types is None or c.types == tuple(types)) and not c.params.get("refuse")
            and all((getattr(c, k) if k in C.Case._fields else c.params.get(k)) == v for k, v in where.items())]


def test_table_shape_rules():
    assert tuple(C.OPS.index(n) for n in ("GEMV", "GATEUP", "NORM_GEMV", "NORM_ARGMAX", "NORM_GATEUP")) == (
        Q.LOP_GEMV, Q.LOP_GATEUP, Q.LOP_NORM_GEMV, Q.LOP_NORM_ARGMAX, Q.LOP_NORM_GATEUP)
    assert {c.form for c in C.CASES} == set(C.FAMILIES)
    for c in C.CASES:
        assert c.K % 256 == 0 and c.K <= 6144 and c.nt <= 300 and max(c.rows) <= 128 and c.row0 + c.nrows <= sum(c.rows), c
        assert set(c.types) <= {8, 11, 12, 13, 14} and len(c.types) == len(c.rows), c
        if c.op in ("GATEUP", "NORM_GATEUP"):
            assert len(c.types) == 2 and c.types[0] == c.types[1] and c.rows[0] == c.rows[1] and c.nrows == 2 * c.rows[0], c
        elif len(c.types) > 1:
            assert c.types in C.MIXTURES and c.rows == (32, 32, 32), c
        else:
            assert c.rows[0] in (64, 96, 128), c
    assert [C.ts_class(t) for t in MIX] == [-1, -1, -2, -2, -1] and C.ts_class((12, 12)) == 12 and C.ts_class((8,)) == 8


def test_table_covers_gemv_norm():
    classes = set()
    for types in SINGLES + [C.Q8_KQ] + MIX:
        got = _of("GEMV_NORM", types)
        assert {(c.params["lpr"], c.params["mt"]) for c in got} == PAIRS, types
        assert {1024, 2048} <= {c.K for c in got}, types
        for mt, ragged in ((2, 3), (4, 3), (8, 9)):   # a ragged last token group, and nt == mt exactly
            for lpr in C.LPRS:
                assert _of("GEMV_NORM", types, lpr=lpr, mt=mt, nt=ragged) and _of("GEMV_NORM", types, lpr=lpr, mt=mt, nt=mt), (types, lpr, mt)
        assert all(_of("GEMV_NORM", types, lpr=lpr, mt=1, nt=1) for lpr in C.LPRS), types
        if any(c.K == 256 for c in got):
            classes.add(C.ts_class(types))
    assert classes == {8, 11, 12, 13, 14, -1, -2}   # a workgroup of one wave, once per TS class
    assert {c.params["nparts"] for c in _of("GEMV_NORM")} == {0, 1, 2, 3} and {c.params["keys"] for c in _of("GEMV_NORM")} == {0, 1}


def test_table_covers_argmax():
    for types in SINGLES:
        for add in (0, 7):
            got = _of("GEMV_NORM_ARGMAX", types, idx_add=add)
            assert {c.params["mt"] for c in got} == set(C.MTS) and all(c.params["lpr"] == 2 and sum(c.rows) >= 128 for c in got), types
            assert all(c.nt > KR.ARGMAX_TIES and c.params["nrows_valid"] <= c.nrows - 2 for c in got)


def test_table_covers_gu_swiglu_norm():
    for types in [(t, t) for t in C.SINGLE]:
        got = _of("GU_SWIGLU_NORM", types)
        assert {(c.K, c.params["mt"]) for c in got} == set(itertools.product((1024, 2048), (1, 2, 4))), types
        assert {c.nt for c in got} == {1, 2, 3, 5, 7} and {c.rows[0] for c in got} == {32, 96}, types


def test_table_covers_gemv_kq():
    for types in SINGLES + MIX:
        assert {(c.params["lpr"], c.params["mt"]) for c in _of("GEMV_KQ", types, K=512, nt=11)} == PAIRS, types
        assert _of("GEMV_KQ", types, K=2304), types


def test_table_covers_gemm_kq_mfma():
    for types in SINGLES + MIX:
        got = _of("GEMM_KQ_MFMA", types)
        assert {256, 1024, 2304, 6144} <= {c.K for c in got} and {16, 33, 97, 300} <= {c.nt for c in got}, types
        for nt in (16, 33, 97, 300):
            want = {z for z in (1, 3, C.tiles(nt)) if z <= C.tiles(nt)}
            assert want <= {c.params["ztiles"] for c in _of("GEMM_KQ_MFMA", types, nt=nt)}, (types, nt)
        assert set().union(*[C.parked(c.nt, c.params["ztiles"]) for c in got]) >= {1, 2, 3, 4, 10}, types
        assert C.parked(300, 3) == {3, 4} and C.parked(97, 3) == {1, 2}   # ztiles 3: 10 tiles as 4 / 3 / 3, 4 tiles as 2 / 1 / 1 per workgroup
        if len(types) == 3:
            assert _of("GEMM_KQ_MFMA", types, row0=32, nrows=64), types
        else:
            assert _of("GEMM_KQ_MFMA", types, row0=32, nrows=40), types


def test_table_covers_gu_kq_mfma():
    for types in [(t, t) for t in C.SINGLE]:
        got = _of("GU_KQ_MFMA", types)
        assert {c.K for c in got} == {1024, 2048} and {c.nt for c in got} == {16, 40, 128, 129, 300} and {c.rows[0] for c in got} == {32, 64}, types
        for nt in (16, 40, 128, 129, 300):
            zs = {c.params["ztiles"] for c in _of("GU_KQ_MFMA", types, nt=nt)}
            assert {(C.tiles(nt) + 3) // 4, C.tiles(nt)} <= zs, (types, nt)
        assert _of("GU_KQ_MFMA", types, nt=300, ztiles=3) and _of("GU_KQ_MFMA", types, nt=129, ztiles=2), types   # unequal parking: 4 / 3 / 3 and 3 / 2
        assert set().union(*[C.parked(c.nt, c.params["ztiles"]) for c in got]) == {1, 2, 3, 4}, types
        assert C.parked(300, 3) == {3, 4} and C.parked(129, 2) == {2, 3}, types
        refused = [c for c in C.CASES if c.form == "GU_KQ_MFMA" and c.types == types and c.params.get("refuse")]
        assert [(C.tiles(c.nt), c.params["ztiles"]) for c in refused] == [(5, 1)], types


# ------------------------------------------------------------------ the engine launches nothing the table leaves out ------------------------------
def _table_keys(cases=None):
    keys, parks = set(), {}
    for c in C.CASES if cases is None else cases:
        if c.params.get("refuse"):
            continue
        ts = C.ts_class(c.types)
        keys.add((c.form, c.params.get("lpr", 0), c.params.get("mt", 0), ts))
        if "ztiles" in c.params:
            parks.setdefault((c.form, ts), set()).update(C.parked(c.nt, c.params["ztiles"]))
    return keys, parks


def _mix(quant):
    """the tensor types of one full-size layer + the head, every alternative of tools/q3synth.c's mix: name -> [types of the fused matrix]"""
    if quant == "q3_k_m":
        return {"qkv": [(11, 11, 13), (11, 11, 12)], "o": [(12,)], "gate_up": [(11, 11)], "down": [(13,), (12,)], "head": [(14,)]}
    a = 13 if quant == "q5_k_m" else 12
    return {"qkv": [(a, a, a), (a, a, 14)], "o": [(a,)], "gate_up": [(a, a)], "down": [(a,), (14,)], "head": [(14,)]}


def _model_launches(c, head_row0, head_rows, mix):
    """(op, K, row0, nrows, ff, types, rows per tensor) of every quantised linear launch of Transformer::forward / head, fused decode steps and
    the unfused sequence alike"""
    d, dq, dkv, ff = c["d"], c["nh"] * 128, c["nkv"] * 128, c["ff"]
    out = []
    for t in mix["qkv"]:
        out += [(op, d, 0, dq + 2 * dkv, 0, t, (dq, dkv, dkv)) for op in (Q.LOP_GEMV, Q.LOP_NORM_GEMV)]
    out += [(Q.LOP_GEMV, dq, 0, d, 0, t, (d,)) for t in mix["o"]]
    for t in mix["gate_up"]:
        out += [(Q.LOP_GATEUP, d, 0, 2 * ff, ff, t, (ff, ff)), (Q.LOP_NORM_GATEUP, d, 0, 2 * ff, ff, t, (ff, ff))]
    out += [(Q.LOP_GEMV, ff, 0, d, 0, t, (d,)) for t in mix["down"]]
    for t in mix["head"]:
        out += [(op, d, head_row0, head_rows, 0, t, (head_row0 + head_rows,)) for op in (Q.LOP_GEMV, Q.LOP_NORM_GEMV, Q.LOP_NORM_ARGMAX)]
        out.append((Q.LOP_NORM_GEMV, d, 0, 32, 0, t, (head_row0 + head_rows,)))   # hidden states only: the prologue through a 32-row GEMV
    return out


PLAN_TOKS = list(range(1, 9)) + [16, 17, 64, 256, 300]


@pytest.mark.parametrize("quant", ["q5_k_m", "q4_k_m", "q3_k_m"])
@pytest.mark.parametrize("model", ["talker", "predictor"])
def test_planned_launches_are_in_the_table(model, quant):
    talker, pred = _full_dims()
    c = talker if model == "talker" else pred
    assert (talker["d"], (talker["nh"] + 2 * talker["nkv"]) * 128, talker["ff"], pred["d"]) == (2048, 4096, 6144, 1024)   # the shapes the table is built around
    head_row0, head_rows = (0, c["nv"]) if model == "talker" else (2048, 2048)   # predictor: one 2048-row codebook slice
    keys, parks = _table_keys()
    seen = set()
    for op, K, row0, nrows, ff, types, rows in _model_launches(c, head_row0, head_rows, _mix(quant)):
        weights = [(np.zeros(0, np.uint8), t, n) for t, n in zip(types, rows)]
        ts = C.ts_class(types)
        for nt in PLAN_TOKS:
            f, lpr, mt, z = Q.linear_plan(op, weights=weights, K=K, row0=row0, nrows=nrows, ntok=nt, ff=ff, x_stride=K, out_stride=nrows, kq_layout=1)
            if f == "GU_UNFUSED":   # the plain GEMV over the 2 ff rows + k_swiglu_quant
                assert op == Q.LOP_GATEUP
                f, lpr, mt, z = Q.linear_plan(Q.LOP_GEMV, weights=weights, K=K, nrows=nrows, ntok=nt, out_stride=nrows, kq_layout=1)
            assert f in C.FAMILIES, (f, op, types, nt)
            z_used = f in ("GEMM_KQ_MFMA", "GU_KQ_MFMA")
            key = (f, 0 if z_used else lpr, 0 if z_used else mt, ts)
            assert key in keys, (key, K, nrows, nt)
            if z_used:
                assert 1 <= z <= C.tiles(nt) and C.parked(nt, z) <= parks[(f, ts)], (key, nt, z)
            seen.add(key)
    assert {k[0] for k in seen} == set(C.FAMILIES)   # the plans were really asked: every family is launched by this model


def test_a_removed_case_is_missed():
    """without its (GEMV_NORM, lpr 4, mt 8, TS -2) cases the table no longer holds what the Q3_K_M talker's fused QKV launches at 8 tokens"""
    talker, _ = _full_dims()
    d, dq, dkv = talker["d"], talker["nh"] * 128, talker["nkv"] * 128
    w = [(np.zeros(0, np.uint8), t, n) for t, n in zip((11, 11, 12), (dq, dkv, dkv))]
    f, lpr, mt, _ = Q.linear_plan(Q.LOP_NORM_GEMV, weights=w, K=d, nrows=dq + 2 * dkv, ntok=8, out_stride=dq + 2 * dkv, kq_layout=1)
    key = (f, lpr, mt, C.ts_class((11, 11, 12)))
    assert key == ("GEMV_NORM", 4, 8, -2) and key in _table_keys()[0]
    thinned = [c for c in C.CASES if not (c.form == f and C.ts_class(c.types) == -2 and c.params["lpr"] == lpr and c.params["mt"] == mt)]
    assert len(thinned) < len(C.CASES) and key not in _table_keys(thinned)[0]


# ------------------------------------------------------------------ the references alone are sound ------------------------------------------------
@pytest.mark.parametrize("form", [f for f in C.FAMILIES if f != "GEMV_NORM_ARGMAX"])
def test_oracle_on_the_twin_is_within_the_float64_bound(oracle, form):
    """for every shape of the table the oracle's result on the twin rows stays within the bound the GPU test holds the device to (the device is
    bit-equal to it): the inputs chosen here leave the bound something to say"""
    worst = 0.0
    for shape, _ in C.shapes(form):
        r = KR.reference(oracle.lib(), shape)
        assert 0.0 < r.ratio <= 1.0, (C.shape_id(shape), r.ratio)
        worst = max(worst, r.ratio)
    print("%s: %d cases on %d shapes, worst oracle err / bound %.3g" % (form, len([c for c in C.CASES if c.form == form]), len(C.shapes(form)), worst))


def test_argmax_ties_are_what_they_are_built_to_be(oracle):
    for shape, _ in C.shapes("GEMV_NORM_ARGMAX"):
        r = KR.reference(oracle.lib(), shape)
        st = dict(shape.setup)
        nv, add = st["nrows_valid"], st["idx_add"]
        lg, code = r.logits, lambda t: R.key_code(r.keys[t]) - add
        for t, (a, b) in zip(r.toks, r.pairs):
            assert (a // 32 != b // 32 or b >= nv) and _same_bits(lg[t, a], lg[t, b]) and lg[t, a] == np.nanmax(lg[t, :nv]), (C.shape_id(shape), t)
            assert (lg[t, :nv] == lg[t, a]).sum() == (2 if b < nv else 1), (C.shape_id(shape), t)   # no third row ties
        assert len({x for p in r.pairs for x in p}) == 2 * KR.ARGMAX_TIES and len(set(r.toks)) == KR.ARGMAX_TIES
        (a0, b0), (a1, b1), (a2, b2), (a3, b3) = r.pairs
        t0, t1, t2, t3 = r.toks
        assert max(b0, b1) < nv <= min(b2, b3)
        assert code(t0) == min(a0, b0) and code(t1) == max(a1, b1) and code(t2) == a2 and code(t3) not in (a3, b3)
        assert R.key_code(R.greedy_key(lg[t3], int(r.mask[t3]), add, r.armed)) - add == b3   # without the valid-row limit the copy would win
        assert all(code(t) == int(np.argmax(lg[t, :nv])) for t in range(shape.nt) if t not in r.toks)


def _same_bits(a, b):
    return np.float32(a).view(np.uint32) == np.float32(b).view(np.uint32)
