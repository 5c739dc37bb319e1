"""q3tts_op_attention_keyed: the attention front ends reading their q/k/v rows from a table through argmax keys (QkvRows with keys: the code
predictor's layer 0 on its load-time table), against q3tts_op_attention on the same rows gathered on the host -- every output and both
caches byte for byte -- and against the float64 bound of tests/attention_ref.py.  The table (padding floats included) and every cache byte
outside the appended rows must come back unchanged.  k_attention_fused at 1 and 3 tokens, k_attention_short<1|2> and the unfused pair at
9, with the predictor's uniform positions and with per-token seq / slot / pos on permuted pages.  (-m gpu)"""
import numpy as np
import pytest

import attention_cases as AC
import attention_ref as R

pytestmark = pytest.mark.gpu

N_HEAD, N_KV, N_LAYER, LAYER = 2, 1, 2, 1
ROW = (N_HEAD + 2 * N_KV) * R.HD
STRIDE = ROW + 64
TABLE_ROWS = 5
SELECT = [3, 0, 3, 4, 1, 2, 0, 4, 1]    # out of order; row 3 serves two tokens (from 3 tokens on)
KEY_STRIDE = 3                           # keys [ntok][3]: column 0 selects, the others name rows far outside the table
CASES = [("FUSED", 1), ("FUSED", 3), ("SHORT1", 9), ("SHORT2", 9), ("UNFUSED", 9)]


def _problem(form, ntok, uniform):
    seed = 500 + 10 * ntok + (1 if uniform else 0)
    if uniform:   # the predictor's passes: token t = sequence t = page t, one position everywhere
        P = AC.Problem("keyed_u%d" % ntok, seed, [(0, 1)] * ntok, n_head=N_HEAD, n_kv=N_KV, n_layer=N_LAYER, layer=LAYER, uniform_pos=5)
    else:
        P = AC.Problem("keyed_e%d" % ntok, seed, [(int(i * 7 % 17), 1) for i in range(ntok)], n_head=N_HEAD, n_kv=N_KV, n_layer=N_LAYER,
                       layer=LAYER, pos="distinct")
    rng = np.random.default_rng(seed + 7)
    table = (rng.standard_normal((TABLE_ROWS, STRIDE)) * 1.5).astype(np.float32)
    sel = SELECT[:ntok]
    P.qkv, P.qkv_stride = np.ascontiguousarray(table[sel]), STRIDE   # the gathered rows: what the float64 checks and the plain op read
    return P, table, sel


def _keys(gpu, sel, seed):
    rng = np.random.default_rng(seed)
    keys = np.zeros((len(sel), KEY_STRIDE), np.uint64)
    for t, c in enumerate(sel):
        keys[t, 0] = gpu.argmax_key(float(rng.standard_normal()), c)
        for j in range(1, KEY_STRIDE):
            keys[t, j] = gpu.argmax_key(float(rng.standard_normal()), 100000 + t)
    return keys


@pytest.mark.parametrize("uniform", [True, False], ids=["uniform_pos", "seq_slot_pos"])
@pytest.mark.parametrize("form,ntok", CASES, ids=["%s-%d" % c for c in CASES])
def test_keyed_rows_equal_gathered_rows(gpu, form, ntok, uniform):
    P, table, sel = _problem(form, ntok, uniform)
    keys = _keys(gpu, sel, 900 + ntok)
    args, kw = P.op_args(True)
    kin, vin = args[3].copy(), args[4].copy()
    plain = gpu.op_attention(*args, form=form, **kw)
    keyed = gpu.op_attention(table, *args[1:], form=form, keys=keys, **kw)
    assert plain["form"] == form and keyed["form"] == form
    # the same bytes as the launch on the gathered rows
    for key in ("aq", "ad", "k_cache", "v_cache"):
        assert np.array_equal(keyed[key], plain[key]), (form, ntok, key)
    if form == "FUSED":
        assert keyed["att"] is None and plain["att"] is None
    else:
        assert np.array_equal(keyed["att"].view(np.uint32), plain["att"].view(np.uint32)), (form, ntok, "att")
    # the float64 contract of the form, on what the keyed launch wrote
    worst, rel = AC.check_f64(P, form, keyed)
    if keyed["att"] is not None:
        print("F64 keyed %-8s %-10s max|y-y64|/sum(p|v|) = %.3e  (%.3f of the bound)" % (form, P.name, worst, rel))
    # nothing else was written: the whole table, and every cache byte but the appended rows
    assert np.array_equal(keyed["qkv"].view(np.uint32), table.view(np.uint32)), (form, ntok, "the table changed")
    shape_k, shape_v = (P.n_pages, N_LAYER, N_KV, 16, R.PAGE, 8), (P.n_pages, N_LAYER, N_KV, R.PAGE, R.HD)
    ek, ev = kin.copy().reshape(shape_k), vin.copy().reshape(shape_v)
    for t in range(ntok):
        K, V = P.appended(keyed["k_cache"], keyed["v_cache"], t)
        R.write_rows(ek, ev, P.pages[int(P.seq[t])], LAYER, [int(P.slot[t])], K[None], V[None])
    assert np.array_equal(keyed["k_cache"].reshape(shape_k), ek) and np.array_equal(keyed["v_cache"].reshape(shape_v), ev), (form, ntok, "cache")


def test_keyed_refusals(gpu):
    """a key outside the table and the ggml form are refused before anything is launched"""
    P, table, sel = _problem("UNFUSED", 3, True)
    args, kw = P.op_args(True)
    keys = _keys(gpu, sel, 1)
    bad = keys.copy()
    bad[1, 0] = gpu.argmax_key(0.5, TABLE_ROWS)
    with pytest.raises(gpu.Q3Error):
        gpu.op_attention(table, *args[1:], form="UNFUSED", keys=bad, **kw)
    with pytest.raises(gpu.Q3Error):
        gpu.op_attention(table, *args[1:], form="GGML", keys=keys, **kw)
