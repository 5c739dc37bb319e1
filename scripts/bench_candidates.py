"""Cost of [EXT] candidate sets (q3tts_submit_candidates), full-size model, Q8_0, codes only, the scheduler stepped by this thread, rounds
interleaved in one process on one GPU.  For prompt rows {43, 300} x n {2, 4, 8}, twice -- on an idle engine (an in-line wave) and beside 32
running slots (an asynchronous wave on the second talker instance) --
  (a) set:    one q3tts_submit_candidates call with n seeds,
  (b) plain:  n q3tts_submit calls of the same prompt with the same seeds (the parent commit's only way; this path is unchanged),
each timed from the first submit call until every candidate has its first frame (q3tts_poll n_frames > 0), with the engine's prefill_ms
(device time of the wave's prefill, HIP events) over the same span.  The codes of (a) and (b) are compared bit for bit.  Prints one JSON
line per (busy, rows, n) with medians over the rounds.  --only ROWSxN runs one shape (for a kernel trace of k_kv_fork).
Usage: python scripts/bench_candidates.py [--model-dir DIR] [--rounds 5] [--rows 43,300] [--n 2,4,8] [--busy 0,32] [--only 300x4]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SAMPLING = dict(temperature=0.9, top_k=50, top_p=1.0)
FRAMES = 8


def _first_frames(eng, ids, t0):
    """steps the scheduler until every request has a frame; ms since t0"""
    while any(eng.poll(r)["n_frames"] == 0 for r in ids):
        assert time.perf_counter() - t0 < 120.0, "no first frame"
        eng.sched_step()
    return (time.perf_counter() - t0) * 1e3


def _finish(eng, ids):
    while any(eng.poll(r)["state"] not in (3, 4, -1) for r in ids):
        eng.sched_step()
    return [eng.result(r)["codes"] for r in ids]


def _round(eng, prompt, seeds, as_set, background):
    """one measurement: `background` running requests first (at least one frame group each), then the candidates"""
    bg = [eng.submit(p, max_steps=400, seed=1000 + i, mask_eos=True, **SAMPLING) for i, p in enumerate(background)]
    if bg:
        _first_frames(eng, bg, time.perf_counter())
    pf0 = eng.stats()["prefill_ms"]
    t0 = time.perf_counter()
    if as_set:
        ids = eng.submit_candidates(prompt, seeds, max_steps=FRAMES, **SAMPLING)
    else:
        ids = [eng.submit(prompt, max_steps=FRAMES, seed=s, mask_eos=True, **SAMPLING) for s in seeds]
    ms = _first_frames(eng, ids, t0)
    pf = eng.stats()["prefill_ms"] - pf0
    codes = _finish(eng, ids)
    for r in bg:
        eng.cancel(r)
    while eng.sched_step():
        pass
    for r in bg:
        eng.release(r)
    return ms, pf, codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", default="43,300")
    ap.add_argument("--n", default="2,4,8")
    ap.add_argument("--busy", default="0,32")
    ap.add_argument("--only", default=None)
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    shapes = [(int(r), int(n)) for r in a.rows.split(",") for n in a.n.split(",")]
    if a.only:
        shapes = [tuple(int(x) for x in a.only.split("x"))]
    busy = [int(b) for b in a.busy.split(",")]
    eng = Q.Engine(model, "q8_0", max_batch=max(busy) + max(n for _, n in shapes), max_prompt=512, max_steps=400, load_codec=False)
    rng = np.random.default_rng(1)
    base = eng.assets.build_core(rng.integers(0, 4000, 24).astype(np.int32), lang_id=2055, spk_emb=spk)
    try:
        for nb in busy:
            background = [eng.assets.build_core(rng.integers(0, 4000, 8 + i % 5).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(nb)]
            for rows, n in shapes:
                prompt = np.ascontiguousarray(base[np.arange(rows) % base.shape[0]], np.float32)
                seeds = list(range(7000, 7000 + n))
                _round(eng, prompt, seeds, True, background)                  # warm-up: graphs of these widths captured
                _round(eng, prompt, seeds, False, background)
                res = {"set": [], "plain": [], "set_pf": [], "plain_pf": []}
                for _ in range(a.rounds):
                    ms, pf, got = _round(eng, prompt, seeds, True, background)
                    res["set"].append(ms), res["set_pf"].append(pf)
                    ms, pf, want = _round(eng, prompt, seeds, False, background)
                    res["plain"].append(ms), res["plain_pf"].append(pf)
                    assert all(np.array_equal(g, w) for g, w in zip(got, want)), "a candidate differs from its plain submission"
                med = {k: statistics.median(v) for k, v in res.items()}
                print(json.dumps({"running_slots": nb, "prompt_rows": rows, "n": n, "rounds": a.rounds,
                                  "set_first_frames_ms": round(med["set"], 3), "plain_first_frames_ms": round(med["plain"], 3),
                                  "set_prefill_ms": round(med["set_pf"], 3), "plain_prefill_ms": round(med["plain_pf"], 3),
                                  "pages_copied_per_set": (n - 1) * ((rows + 63) // 64)}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
