"""[EXT] KV cache type Q8_0, the oracle's side (oracle/q3o_model.c: q3o_attn_head_q8, q3o_model_set_kv_type), without a GPU.  Before any
kernel is compared with q3o_attn_head_q8 bit for bit, the head itself is held to float64: on every problem of tests/test_gpu_kv_q8.py, over
the cache the append leaves behind, |y - y64| <= bound with the bound the kernel is held to (attention_ref.attention_q8).  Then the model
with the Q8_0 cache on the tiny synthetic talker: finite rows that differ from the F16 cache's and come back bit for bit after clear_kv."""
import os

import numpy as np
import pytest

import test_gpu_kv_q8 as G


@pytest.mark.parametrize("P", G.CASES, ids=[P.name for P in G.CASES])
def test_oracle_head_within_f64_bound(oracle, P):
    qrot, C = G.appended(oracle, P, G.caches(P, poison=True))
    att = np.zeros((P.ntok, P.n_head * G.R.HD), np.float32)
    grp = P.n_head // P.n_kv
    for t in range(P.ntok):
        for h in range(P.n_head):
            Kq, ks, Vq, vs = G.stored(P, C, t, h // grp)
            att[t, h * G.R.HD:(h + 1) * G.R.HD] = oracle.attn_head_q8(qrot[t, h * G.R.HD:(h + 1) * G.R.HD], Kq.reshape(-1, G.R.HD), ks, Vq, vs)
    assert np.all(np.isfinite(att))
    worst = G.check_heads(P, C, qrot, att)
    print("F64 Q8KV oracle %-12s max |y-y64| / bound = %.3f" % (P.name, worst))


def test_model_q8_cache_on_tiny_talker(oracle, tiny_model):
    path = os.path.join(tiny_model, "gguf_q8_0", "qwen3_tts_talker.gguf")
    n, d = 70, 2048
    x = (np.random.default_rng(5).standard_normal((n, d)) * 0.3).astype(np.float32)
    pos = np.stack([np.arange(n), np.arange(n) // 2 + 3, np.arange(n), 0 * np.arange(n)], 1).astype(np.int32)
    q, f = oracle.Model(path, 256, kv_type="q8_0"), oracle.Model(path, 256)
    rows = lambda m: np.stack([m.eval(x[t], pos[t], d)[0] for t in range(n)])
    hq, hf = rows(q), rows(f)
    assert np.all(np.isfinite(hq)) and not np.array_equal(hq, hf)
    q.clear()
    assert np.array_equal(rows(q).view(np.uint32), hq.view(np.uint32))
    print("oracle Q8_0 against F16 cache: max |h_q8 - h_f16| = %.3e (rms of h_f16 %.3e)" % (float(np.abs(hq - hf).max()),
                                                                                         float(np.sqrt(np.mean(hf.astype(np.float64) ** 2)))))
    g = oracle.Model(path, 256, kv_type="f16")
    assert np.array_equal(rows(g).view(np.uint32), hf.view(np.uint32))          # the named F16 type is the default
    for m in (q, f, g):
        m.close()
    with pytest.raises(RuntimeError, match="unknown KV cache type"):
        oracle.Model(path, 256, kv_type=2)
    oracle.set_arith_mode(1)
    try:
        with pytest.raises(RuntimeError, match="Q3_SPEC=ggml has no KV cache type Q8_0"):
            oracle.Model(path, 256, kv_type="q8_0")
    finally:
        oracle.set_arith_mode(0)
