"""Host overhead of the ONNX executor per node: a chain of 512 element-wise nodes on a [1, 64] tensor (Add and Sub of a [64] initialiser each,
Mul by a host scalar, Tanh), so every kernel is one workgroup and a run is dominated by dispatch, edge bookkeeping and whatever run() does per
initialiser.  5 warm-up runs, 50 timed runs of session.run() + the fetch of the one output; prints one JSON line with the median."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import q3tts as Q
import onnx_writer as W

NODES, WARMUP, RUNS = 512, 5, 50
rng = np.random.default_rng(0)
nodes, inits, cur = [], [W.tensor("half", np.float32(0.5).reshape(()))], "x"
for k in range(NODES):
    nxt = "t%d" % k if k + 1 < NODES else "y"
    if k % 4 == 0 or k % 4 == 3:
        inits.append(W.tensor("c%d" % k, rng.standard_normal(64).astype(np.float32)))
        nodes.append(W.node("Add" if k % 4 == 0 else "Sub", [cur, "c%d" % k], [nxt]))
    elif k % 4 == 1:
        nodes.append(W.node("Mul", [cur, "half"], [nxt]))
    else:
        nodes.append(W.node("Tanh", [cur], [nxt]))
    cur = nxt
x = rng.standard_normal((1, 64)).astype(np.float32)
with tempfile.TemporaryDirectory() as tmp:
    path = os.path.join(tmp, "chain.onnx")
    with open(path, "wb") as f:
        f.write(W.model(nodes, inits, [W.value_info("x", W.F32, [1, 64])], [W.value_info("y", W.F32, [1, 64])], opset=17))
    s = Q.OnnxSession(path)
    assert s.unsupported() == []
    ms = []
    for i in range(WARMUP + RUNS):
        t0 = time.perf_counter()
        y = s.run({"x": x}, ["y"])["y"]
        ms.append((time.perf_counter() - t0) * 1e3)
    launches = s.launches()
    s.close()
ms = sorted(ms[WARMUP:])
print(json.dumps({"nodes": NODES, "runs": RUNS, "median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                  "launches_per_run": launches // (WARMUP + RUNS), "checksum": float(np.abs(y).sum())}))
