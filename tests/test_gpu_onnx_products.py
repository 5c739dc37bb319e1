"""The ONNX executor's product and row kernels (csrc/onnx_exec.hip) against float64 at every tile edge, operand layout and on both kernel
families; rank 8 data movement against numpy bit for bit, rank 9 refused, int64 payloads kept whole.  The case tables, the references and the
derivation of every bound are in tests/onnx_cases.py; a result is compared as |got - ref| <= bound, element by element, and nothing else.

ONNX_F64_REPORT=<path> appends one line per kernel family with the largest error / bound (profiles/voice_front_end_f64.md)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import onnx_cases as OC
import onnx_writer as W

pytestmark = pytest.mark.gpu
F32, I64 = W.F32, W.I64
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def products():
    return OC.product_cases()


@pytest.fixture(scope="module")
def rows():
    return OC.row_cases()


def _report(tag, worst):
    rep = os.environ.get("ONNX_F64_REPORT")
    for fam, (r, name) in sorted(worst.items()):
        line = "%s %s %.4g %s" % (tag, fam, r, name)
        print(line)
        if rep:
            with open(rep, "a") as f:
                f.write(line + "\n")


def _check(case, got, bound, worst, failures):
    if isinstance(case.ref, dict):
        r, at = 0.0, ""
        for o in case.ref:
            ro = OC.ratio(got[o], case.ref[o], bound[o])
            if ro >= r:
                r, at = ro, o
        label = case.name + ":" + at
    else:
        r, label = OC.ratio(got, case.ref, bound), case.name
    if r >= worst.get(case.family, (-1.0, ""))[0]:
        worst[case.family] = (r, label)
    if not r <= 1.0:
        failures.append("%s: error / bound %.4g" % (label, r))


FAMILIES = ("k_mm_mfma", "k_matmul", "conv1d_mfma", "convtr1d_mfma+col2im", "k_conv2d", "k_convtr2d")


@pytest.mark.parametrize("family", FAMILIES)
def test_products_against_float64(family, gpu, tmp_path, products):
    worst, failures = {}, []
    mine = [c for c in products if c.family == family]
    assert mine
    for case in mine:
        got, launches = OC.run_case(gpu, tmp_path, case)
        assert launches == case.launches, (case.name, launches)     # which family ran, where the counter can tell (onnx_cases.py)
        _check(case, got, case.bound, worst, failures)
    _report("default", worst)
    assert not failures, failures


def test_case_table_covers_the_edges(products):
    """the table itself: every tile edge the issue lists appears, on the side of mm_fast_ok its shape says"""
    gem = [c for c in products if c.name.startswith("gemm")]
    dims = [tuple(int(v) for v in c.name.split("_")[1].split("x")) for c in gem]
    for v in (15, 16, 17, 63, 64, 65, 128):
        assert sum(d[0] == v for d in dims) >= 2 and sum(d[1] == v for d in dims) >= 2, v
    for k in (1, 15, 16, 17, 31, 32, 33, 48):
        assert sum(d[2] == k for d in dims) >= 2, k
    for lay in ("_rm_", "_tA_", "_tB_", "_tAtB_"):
        assert any(lay in c.name and c.fast for c in gem) and any(lay in c.name and not c.fast for c in gem), lay
    for kind in ("scalar", "n", "1n", "m1", "mn", "None"):
        assert any("bias-" + kind in c.name for c in gem)
    for c in products:
        assert c.fast == (c.family in ("k_mm_mfma", "conv1d_mfma", "convtr1d_mfma+col2im")), c.name


def test_products_on_the_naive_kernels(gpu, tmp_path, products):
    """Q3_ONNX_NAIVE is read once when the library loads, so ONE fresh child process runs the whole product table with it set and writes the
    outputs to an .npz; they are held here to the same float64 bounds (the direct kernels' chain for the convolutions).  This puts k_matmul,
    k_conv2d and k_convtr2d on every shape.  Nothing else uses the GPU while the child runs."""
    out = str(tmp_path / "naive.npz")
    env = dict(os.environ, Q3_ONNX_NAIVE="1", PYTHONPATH=os.pathsep.join([p for p in sys.path if p]))
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "onnx_cases.py"), out], env=env, capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        pytest.exit("the Q3_ONNX_NAIVE child ran into its time limit: nothing further runs on this GPU", returncode=1)
    if r.returncode < 0:
        pytest.exit("the Q3_ONNX_NAIVE child died of signal %d: nothing further runs on this GPU\n%s" % (-r.returncode, r.stderr[-2000:]), returncode=1)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    worst, failures = {}, []
    for case in products:
        assert int(z["launches:" + case.name]) == case.naive_launches, case.name
        fam = case.family
        case.family = {"k_mm_mfma": "k_matmul", "conv1d_mfma": "k_conv2d", "convtr1d_mfma+col2im": "k_convtr2d"}.get(fam, fam)
        try:
            _check(case, z[case.name], case.naive_bound, worst, failures)
        finally:
            case.family = fam
    _report("naive", worst)
    assert not failures, failures


@pytest.mark.parametrize("group", ["reduce", "arg", "softmax", "norm", "cumsum"])
def test_row_kernels_against_float64(group, gpu, tmp_path, rows):
    worst, failures = {}, []
    mine = [c for c in rows if c.name.startswith(group)]
    assert mine
    for case in mine:
        got, _ = OC.run_case(gpu, tmp_path, case)
        for o in case.ref:
            assert got[o].shape == np.shape(case.ref[o]), (case.name, o, got[o].shape)
        _check(case, got, case.bound, worst, failures)
    _report("default", worst)
    assert not failures, failures


def test_softmax_masked_entries_are_exact(gpu, tmp_path, rows):
    """an entry at -inf gives exactly 0 (Softmax) and exactly -inf (LogSoftmax); no output is NaN or inf otherwise"""
    n = 0
    for case in [c for c in rows if c.name.startswith("softmax")]:
        got, _ = OC.run_case(gpu, tmp_path, case)
        masked = np.isneginf(case.feeds["x"])
        n += int(masked.sum())
        assert np.all(got["y_sm"][masked] == 0) and np.all(np.isneginf(got["y_lsm"][masked]))
        assert np.all(np.isfinite(got["y_sm"])) and np.all(np.isfinite(got["y_lsm"][~masked]))
    assert n > 1000


# ------------------------------------------------------------------------------------------------------------------ rank 8 / rank 9
R8 = (2, 1, 2, 1, 2, 1, 2, 3)


def _run(gpu, tmp_path, name, nodes, inits, feeds, outs, opset=18):
    path = os.path.join(str(tmp_path), name + ".onnx")
    ins = [W.value_info(k, I64 if np.issubdtype(np.asarray(v).dtype, np.integer) else F32, list(np.asarray(v).shape)) for k, v in feeds.items()]
    with open(path, "wb") as f:
        f.write(W.model(nodes, inits, ins, [W.value_info(o, F32, []) for o in outs], opset=opset))
    s = gpu.OnnxSession(path)
    try:
        assert s.unsupported() == []
        return s.run(feeds, outs)
    finally:
        s.close()


def test_rank8_data_movement_is_bit_exact(gpu, tmp_path):
    rng = np.random.default_rng(8)
    a = rng.standard_normal(R8).astype(np.float32)
    b = rng.standard_normal((1, 2, 1, 2, 1, 2, 1, 3)).astype(np.float32)
    full = (2, 2, 2, 2, 2, 2, 2, 3)
    i = lambda n, v: W.tensor(n, np.asarray(v, np.int64))
    pads = [0, 0, 0, 0, 0, 0, 1, 2, 0, 0, 0, 0, 0, 0, 1, 1]                   # axes 6 and 7, all sixteen entries spelled out
    inits = [i("full", full), i("reps", [1, 2, 1, 2, 1, 1, 2, 1]), i("pads16", pads), i("pads_ax", [1, 2, 1, 1]), i("ax67", [6, 7]),
             i("st", [-1, 2]), i("en", [-9, -9]), i("sax", [0, 7]), i("sst", [-1, -1])]
    nodes = [W.node("Add", ["a", "b"], ["y_add"]), W.node("Less", ["a", "b"], ["lt"]), W.node("Where", ["lt", "a", "b"], ["y_where"]),
             W.node("Pad", ["a", "pads16"], ["y_pad_c"], attrs=[W.attr_str("mode", "constant")]),
             W.node("Pad", ["a", "pads_ax", "", "ax67"], ["y_pad_r"], attrs=[W.attr_str("mode", "reflect")]),
             W.node("Pad", ["a", "pads_ax", "", "ax67"], ["y_pad_e"], attrs=[W.attr_str("mode", "edge")]),
             W.node("Transpose", ["a"], ["y_tr"], attrs=[W.attr_ints("perm", [7, 6, 5, 4, 3, 2, 1, 0])]),
             W.node("Expand", ["b", "full"], ["y_exp"]), W.node("Tile", ["a", "reps"], ["y_tile"]),
             W.node("Slice", ["a", "st", "en", "sax", "sst"], ["y_slice"])]
    outs = ["y_add", "y_where", "y_pad_c", "y_pad_r", "y_pad_e", "y_tr", "y_exp", "y_tile", "y_slice"]
    r = _run(gpu, tmp_path, "rank8", nodes, inits, {"a": a, "b": b}, outs)
    pw = [(0, 0)] * 6 + [(1, 1), (2, 1)]
    want = {"y_add": a + b, "y_where": np.where(a < b, a, b), "y_pad_c": np.pad(a, pw), "y_pad_r": np.pad(a, pw, mode="reflect"),
            "y_pad_e": np.pad(a, pw, mode="edge"), "y_tr": a.transpose(7, 6, 5, 4, 3, 2, 1, 0), "y_exp": np.broadcast_to(b, full),
            "y_tile": np.tile(a, (1, 2, 1, 2, 1, 1, 2, 1)), "y_slice": a[::-1, ..., 2::-1]}
    for o in outs:
        assert r[o].shape == want[o].shape, o
        assert np.array_equal(r[o], want[o]), o


def test_rank9_is_refused_and_the_library_carries_on(gpu, tmp_path):
    """Each of these overran (Add, Where, Pad) or already refused (Transpose, Expand, Resize) before the rank checks; now every one is an error
    from run() that names the rank, and a good graph runs afterwards."""
    a = np.arange(np.prod(R8), dtype=np.float32).reshape(R8)
    i = lambda n, v: W.tensor(n, np.asarray(v, np.int64))
    un = W.node("Unsqueeze", ["a", "ax0"], ["a9"])
    rs = W.node("Reshape", ["a", "shape9"], ["a9"])
    shape9 = (1,) + R8
    graphs = {
        "Add": [un, W.node("Add", ["a9", "a9"], ["y"])],
        "Where": [rs, W.node("Less", ["a", "a"], ["lt"]), W.node("Where", ["lt", "a9", "a"], ["y"])],
        "Pad": [un, W.node("Pad", ["a9", "pads18"], ["y"])],
        "Transpose": [rs, W.node("Transpose", ["a9"], ["y"], attrs=[W.attr_ints("perm", [8, 7, 6, 5, 4, 3, 2, 1, 0])])],
        "Expand": [un, W.node("Expand", ["a9", "full9"], ["y"])],
        "Resize": [un, W.node("Resize", ["a9", "", "", "sizes9"], ["y"], attrs=[W.attr_str("mode", "nearest")])],
    }
    inits = [i("ax0", [0]), i("shape9", shape9), i("pads18", [0] * 17 + [1]), i("full9", (3,) + R8), i("sizes9", (2,) + R8)]
    for op, nodes in graphs.items():
        with pytest.raises(gpu.Q3Error) as e:
            _run(gpu, tmp_path, "rank9_" + op, nodes, inits, {"a": a}, ["y"])
        msg = str(e.value)
        assert "(" + op in msg and "rank" in msg and "9" in msg.split("rank", 1)[1], msg
        good = _run(gpu, tmp_path, "after_" + op, [W.node("Add", ["a", "a"], ["y"])], [], {"a": a}, ["y"])
        assert np.array_equal(good["y"], a + a)


def test_int64_payloads_stay_whole(gpu, tmp_path):
    """Graph inputs are uploaded by set_input and stay device tensors, so every op below takes the device route (k_gather<int64_t>,
    k_nd_copy<int64_t>, k_where<int64_t>, the device Concat); none of them may pass the payload through f32 or double arithmetic that
    loses 2^40 + 1."""
    big = (1 << 40) + 1
    x = (np.arange(24, dtype=np.int64).reshape(2, 3, 4) - 12) * big
    x[0, 0, 0], x[1, 2, 3] = big, -big
    z = x[::-1].copy() + 7
    f = np.random.default_rng(4).standard_normal((2, 3, 4)).astype(np.float32)
    i = lambda n, v: W.tensor(n, np.asarray(v, np.int64))
    inits = [i("idx", [[2, 0], [1, 1]]), i("st", [3]), i("en", [-9]), i("sax", [2]), i("sst", [-2]), i("eshape", [2, 2, 3, 4]), i("hostpart", [[[big, -big, 5, 6]] * 3])]
    nodes = [W.node("Gather", ["x", "idx"], ["y_gather"], attrs=[W.attr_int("axis", 1)]),
             W.node("Concat", ["x", "z", "hostpart"], ["y_cat"], attrs=[W.attr_int("axis", 0)]),
             W.node("Less", ["f", "zero"], ["neg"]), W.node("Where", ["neg", "x", "z"], ["y_where"]),
             W.node("Transpose", ["x"], ["y_tr"], attrs=[W.attr_ints("perm", [2, 0, 1])]),
             W.node("Slice", ["x", "st", "en", "sax", "sst"], ["y_slice"]), W.node("Expand", ["x", "eshape"], ["y_exp"])]
    inits.append(W.tensor("zero", np.zeros((), np.float32)))
    outs = ["y_gather", "y_cat", "y_where", "y_tr", "y_slice", "y_exp"]
    r = _run(gpu, tmp_path, "i64", nodes, inits, {"x": x, "z": z, "f": f}, outs)
    want = {"y_gather": x[:, [[2, 0], [1, 1]]], "y_cat": np.concatenate([x, z, np.asarray([[[big, -big, 5, 6]] * 3], np.int64)]),
            "y_where": np.where(f < 0, x, z), "y_tr": x.transpose(2, 0, 1), "y_slice": x[:, :, 3::-2], "y_exp": np.broadcast_to(x, (2, 2, 3, 4))}
    for o in outs:
        assert r[o].dtype == np.int64 and r[o].shape == want[o].shape, o
        assert np.array_equal(r[o], want[o]), o
