"""The case table of tests/test_gpu_kq_forms.py: every K-quant linear form (k_gemv_kq, k_gemv_q8_norm, k_gateup_swiglu, k_gemm_kq_mfma) at each
weight type, lane split and tile walk the engine can launch.  Pure Python, no device: tests/test_kq_form_cases_cpu.py asserts what the table
covers, so that a deleted case fails there instead of thinning the GPU test.

A table entry is Case(op, form, types, K, rows, row0, nrows, nt, params).  params holds the launch parameters (lpr, mt, ztiles) and the input
settings of the shape (nparts, keys, nrows_valid, idx_add, refuse).  Entries that differ only in form and launch parameters share one Shape:
the GPU test builds weights and references once per shape and runs its forms, and AUTO, on them."""
from collections import namedtuple

Case = namedtuple("Case", "op form types K rows row0 nrows nt params")
Shape = namedtuple("Shape", "op op_id types K rows row0 nrows nt setup")

SINGLE = (11, 12, 13, 14)                                     # Q3_K, Q4_K, Q5_K, Q6_K
MIXTURES = ((13, 13, 14), (12, 12, 14), (11, 11, 12), (11, 11, 13), (13, 14, 8))   # as the files fuse q, k, v; the last one has a Q8_0 part
Q8_KQ = (8,)                                                  # an all-Q8_0 matrix in the K-quant layout
OPS = ("GEMV", "GATEUP", "NORM", "NORM_GEMV", "NORM_ARGMAX", "NORM_GATEUP")   # q3tts.LOP_* in order
LAUNCH_KEYS = ("lpr", "mt", "ztiles")
LPRS, MTS = (2, 4, 8), (1, 2, 4, 8)


def ts_class(types):
    """the TS the launch instantiates (wslice.h): the type of a one-type matrix, -1 mixed, -2 mixed with a Q3_K part"""
    parts = [t for i, t in enumerate(types) if i == 0 or t != types[i - 1]]
    return parts[0] if len(parts) == 1 else -2 if 11 in parts else -1


def tiles(nt):
    return (nt + 31) // 32


def parked(nt, z):
    """the token-tile counts the workgroups of an MFMA launch walk (workgroup b takes tiles b, b + z, ...)"""
    return {(tiles(nt) - b + z - 1) // z for b in range(z)}


def _rows(types, single=64):
    return (single,) if len(types) == 1 else (32,) * len(types)


def _case(op, form, types, K, rows, row0, nrows, nt, **params):
    return Case(op, form, tuple(types), K, tuple(rows), row0, nrows, nt, params)


def _gemv_norm():
    out = []
    one_wave = [(t,) for t in SINGLE] + [Q8_KQ, MIXTURES[0], MIXTURES[2]]   # one per TS class
    for i, types in enumerate([(t,) for t in SINGLE] + [Q8_KQ] + list(MIXTURES)):
        rows = _rows(types)
        n = sum(rows)
        # (d, nt, the mt values run): a ragged last token group for each mt (nt 3: mt 2, 4 and three z tiles of mt 1; nt 9: mt 8 leaves a second
        # z tile with one token, mt 4 a third), then nt == mt
        groups = [(1024, 3, (1, 2, 4)), (2048, 9, (4, 8)), (2048, 1, (1,)), (1024, 2, (2,)), (2048, 4, (4,)), (1024, 8, (8,))]
        if types in one_wave:   # d 256: a workgroup of one wave
            groups.append((256, 3, (1, 2, 4)))
        for j, (d, nt, mts) in enumerate(groups):
            for lpr in LPRS:
                for mt in mts:
                    out.append(_case("NORM_GEMV", "GEMV_NORM", types, d, rows, 0, n, nt, lpr=lpr, mt=mt, nparts=(i + j) % 4, keys=(i + j // 2) % 2))
    return out


def _argmax():
    out = []
    for i, t in enumerate(SINGLE):
        for add in (0, 7):   # 128 rows: four workgroups contend for a token's key; nt 9 is ragged for every mt > 1
            for mt in MTS:
                out.append(_case("NORM_ARGMAX", "GEMV_NORM_ARGMAX", (t,), 1024, (128,), 0, 128, 9, lpr=2, mt=mt, nparts=1 + i % 2, keys=1,
                                 nrows_valid=120, idx_add=add))
    return out


def _gu_norm():
    out = []
    for i, t in enumerate(SINGLE):
        for j, (d, ff, nt) in enumerate([(1024, 32, 1), (2048, 96, 2), (1024, 96, 3), (2048, 32, 5), (2048, 96, 7), (1024, 32, 7)]):
            for mt in (1, 2, 4):
                out.append(_case("NORM_GATEUP", "GU_SWIGLU_NORM", (t, t), d, (ff, ff), 0, 2 * ff, nt, mt=mt, nparts=(i + j) % 4, keys=1))
    return out


def _gemv_kq():
    out = []
    for types in [(t,) for t in SINGLE] + list(MIXTURES):
        rows = _rows(types)
        n = sum(rows)
        for lpr in LPRS:       # nt 11: a ragged last z tile for every mt
            for mt in MTS:
                out.append(_case("GEMV", "GEMV_KQ", types, 512, rows, 0, n, 11, lpr=lpr, mt=mt))
        for lpr, mt in ((2, 1), (4, 2), (8, 4), (4, 8)):   # K 2304: two super-segments, the second holds one segment
            out.append(_case("GEMV", "GEMV_KQ", types, 2304, rows, 0, n, 3, lpr=lpr, mt=mt))
    return out


def _gemm_kq():
    out = []
    for types in [(t,) for t in SINGLE] + [Q8_KQ] + list(MIXTURES):
        rows = _rows(types, 96)
        n = sum(rows)
        for K, nt in ((256, 16), (1024, 33), (2304, 97), (6144, 300)):   # 1, 2, 4 and 10 token tiles
            for z in sorted({1, 3, tiles(nt)}):
                if z <= tiles(nt):   # ztiles 3: 4 tiles as 2 / 1 / 1, 10 tiles as 4 / 3 / 3 per workgroup
                    out.append(_case("GEMV", "GEMM_KQ_MFMA", types, K, rows, 0, n, nt, ztiles=z))
        if len(types) == 3:    # a window that starts in one tensor and ends in the next
            for z in (1, 2):
                out.append(_case("GEMV", "GEMM_KQ_MFMA", types, 1024, rows, 32, 64, 33, ztiles=z))
        else:                  # nrows no multiple of 32: the second workgroup stores 8 of its 32 columns
            for z in (1, 2):
                out.append(_case("GEMV", "GEMM_KQ_MFMA", types, 1024, rows, 32, 40, 33, ztiles=z))
    return out


def _gu_kq():
    out = []
    for t in SINGLE:
        # (K, ff, nt, ztiles): 1, 2, 4, 5 and 10 tiles; ceil(tiles / 4) parks 4, or 3 and 2; 10 tiles over z = 3 park 4 / 3 / 3, 5 tiles over z = 2 park 3 / 2
        for K, ff, nt, zs in ((1024, 64, 16, (1,)), (2048, 32, 40, (1, 2)), (1024, 32, 128, (1, 2, 4)), (2048, 64, 129, (2, 5)),
                              (1024, 64, 300, (3, 10)), (2048, 32, 300, (3, 5, 10))):
            for z in zs:
                out.append(_case("GATEUP", "GU_KQ_MFMA", (t, t), K, (ff, ff), 0, 2 * ff, nt, ztiles=z))
        out.append(_case("GATEUP", "GU_KQ_MFMA", (t, t), 2048, (64, 64), 0, 128, 129, ztiles=1, refuse=1))   # below ceil(5 / 4): five gate tiles do not fit
    return out


CASES = _gemv_norm() + _argmax() + _gu_norm() + _gemv_kq() + _gemm_kq() + _gu_kq()
FAMILIES = ("GEMV_NORM", "GEMV_NORM_ARGMAX", "GU_SWIGLU_NORM", "GEMV_KQ", "GEMM_KQ_MFMA", "GU_KQ_MFMA")


def launch(case):
    return {k: v for k, v in case.params.items() if k in LAUNCH_KEYS}


def shape_of(case):
    setup = tuple(sorted((k, v) for k, v in case.params.items() if k not in LAUNCH_KEYS and k != "refuse"))
    return Shape(case.op, OPS.index(case.op), case.types, case.K, case.rows, case.row0, case.nrows, case.nt, setup)


def shapes(form, cases=None):
    """-> [(Shape, [Case])] of one form, in table order"""
    out = {}
    for c in CASES if cases is None else cases:
        if c.form == form:
            out.setdefault(shape_of(c), []).append(c)
    return list(out.items())


def shape_id(s):
    return "%s_k%d_n%d+%d_t%d%s" % ("-".join(map(str, s.types)), s.K, s.row0, s.nrows, s.nt, "".join("_%s%d" % (k[:2], v) for k, v in s.setup))
