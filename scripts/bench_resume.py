"""Cost of [EXT] resume (q3tts_submit_resume), full-size model, Q8_0, one request on an otherwise idle engine, EOS masked, talker
T 0.9 / top-k 50, a running driver thread, rounds interleaved in one process on one GPU.  For each split point k of a request of
--frames frames, the time from the submit call to the first NEW frame (q3tts_poll reading n_frames > k; poll spins in this thread) and
to the end of the request, for
  (a) resume:      q3tts_submit_resume with the k frames the request had,
  (b) regenerate:  the parent commit's only alternative -- the same request submitted again without a prefix, whose frame k + 1 arrives
                   after k frames have been generated a second time,
  (c) no prefix:   the time to the first frame of the same prompt without a prefix (what the k extra prefill rows add).
Every resumed run's codes are checked against the uninterrupted run.  Prints one JSON line per k with medians over the rounds.
Usage: python scripts/bench_resume.py [--model-dir DIR] [--frames 64] [--rounds 5] [--k 4,16,32,60] [--text 24]"""
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


def _timed(eng, prompt, frames, seed, first_after, prefix=None):
    """(ms to n_frames > first_after, ms to the end, codes)"""
    t0 = time.perf_counter()
    rid = eng.submit(prompt, max_steps=frames, seed=seed, mask_eos=True, prefix_codes=prefix, **SAMPLING)
    while eng.poll(rid)["n_frames"] <= first_after:
        assert time.perf_counter() - t0 < 120.0, "no new frame"
    t1 = time.perf_counter()
    assert eng.wait(rid, 600000)
    t2 = time.perf_counter()
    return (t1 - t0) * 1e3, (t2 - t0) * 1e3, eng.result(rid)["codes"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--k", default="4,16,32,60")
    ap.add_argument("--text", type=int, default=24)
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=4, max_steps=a.frames, load_codec=False)
    prompt = eng.assets.build_core(np.random.default_rng(1).integers(0, 4000, a.text).astype(np.int32), lang_id=2055, spk_emb=spk)
    ks = [int(k) for k in a.k.split(",") if 0 < int(k) < a.frames]
    eng.sched_start()
    try:
        _, _, want = _timed(eng, prompt, a.frames, 7, 0)                  # warm-up: graphs captured, codes of the uninterrupted run
        for k in ks:
            res = {"resume": [], "regenerate": [], "no_prefix": []}
            for _ in range(a.rounds):
                first, total, codes = _timed(eng, prompt, a.frames, 7, k, prefix=want[:k])
                assert np.array_equal(codes, want), "resumed codes differ from the uninterrupted run"
                res["resume"].append((first, total))
                first, total, codes = _timed(eng, prompt, a.frames, 7, k)
                assert np.array_equal(codes, want)
                res["regenerate"].append((first, total))
                first, total, _ = _timed(eng, prompt, a.frames, 7, 0)
                res["no_prefix"].append((first, total))
            med = {n: [statistics.median(x[i] for x in v) for i in (0, 1)] for n, v in res.items()}
            print(json.dumps({"k": k, "frames": a.frames, "n_prompt": int(prompt.shape[0]), "rounds": a.rounds,
                              "resume_first_new_frame_ms": round(med["resume"][0], 3), "resume_total_ms": round(med["resume"][1], 3),
                              "regenerate_first_new_frame_ms": round(med["regenerate"][0], 3), "regenerate_total_ms": round(med["regenerate"][1], 3),
                              "no_prefix_first_frame_ms": round(med["no_prefix"][0], 3), "no_prefix_total_ms": round(med["no_prefix"][1], 3)}), flush=True)
    finally:
        eng.sched_stop()
        eng.close()


if __name__ == "__main__":
    main()
