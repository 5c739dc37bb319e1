"""Cost of [EXT] scoring given frames (q3tts_submit_score), full-size model, Q8_0, one request on an otherwise idle engine, a running
driver thread, rounds interleaved in one process on one GPU.  For each n, the time from the submit call to the end of the request for
  (a) score:       q3tts_submit_score of the n frames a sampled request produced (submit -> REQ_DONE),
  (b) regenerate:  the parent commit's only way to those numbers -- the same request generated again with its seed and recording on
                   (q3tts_engine_set_logprobs), submit -> REQ_DONE,
  (c) resume:      the time to the first new frame of a plain resume behind the same n frames (q3tts_submit_resume with max_steps n + 4;
                   q3tts_poll reading n_frames > n): what the batched prefill of the same rows costs without the predictor passes.
The scored rows are checked against the recorded ones within 2e-5 * max(1, |lp|).  Prints one JSON line per n with medians over the rounds.
The frames per predictor pass can be changed for an A/B with Q3_SCORE_WIDTH (read when the engine is created).
Usage: python scripts/bench_score.py [--model-dir DIR] [--rounds 5] [--n 16,64,256] [--text 24]"""
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


def _generate(eng, prompt, n, seed):
    t0 = time.perf_counter()
    rid = eng.submit(prompt, max_steps=n, seed=seed, mask_eos=True, **SAMPLING)
    assert eng.wait(rid, 600000)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, eng.result(rid)


def _score(eng, prompt, codes):
    t0 = time.perf_counter()
    rid = eng.submit_score(prompt, codes)
    assert eng.wait(rid, 600000)
    ms = (time.perf_counter() - t0) * 1e3
    return ms, eng.result(rid)


def _resume_first(eng, prompt, codes, seed):
    n = codes.shape[0]
    t0 = time.perf_counter()
    rid = eng.submit(prompt, max_steps=n + 4, seed=seed, mask_eos=True, prefix_codes=codes, **SAMPLING)
    while eng.poll(rid)["n_frames"] <= n:
        assert time.perf_counter() - t0 < 120.0, "no new frame"
    ms = (time.perf_counter() - t0) * 1e3
    assert eng.wait(rid, 600000)
    eng.release(rid)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=None)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--n", default="16,64,256")
    ap.add_argument("--text", type=int, default=24)
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    ns = [int(x) for x in a.n.split(",")]
    eng = Q.Engine(model, "q8_0", max_batch=4, max_steps=max(ns) + 4, load_codec=False)
    prompt = eng.assets.build_core(np.random.default_rng(1).integers(0, 4000, a.text).astype(np.int32), lang_id=2055, spk_emb=spk)
    eng.set_logprobs(True)
    eng.sched_start()
    try:
        for n in ns:
            _, rec = _generate(eng, prompt, n, 7)                         # warm-up: graphs captured, the codes and their recorded rows
            codes = rec["codes"]
            assert codes.shape == (n, 16)
            _score(eng, prompt, codes)
            res = {"score": [], "regenerate": [], "resume": []}
            worst = 0.0
            for _ in range(a.rounds):
                ms, got = _score(eng, prompt, codes)
                res["score"].append(ms)
                lp, want = got["logprobs"].astype(np.float64), rec["logprobs"].astype(np.float64)
                worst = max(worst, float(np.max(np.abs(lp - want) / (2e-5 * np.maximum(1.0, np.abs(want))))))
                ms, again = _generate(eng, prompt, n, 7)
                assert np.array_equal(again["codes"], codes)
                res["regenerate"].append(ms)
                res["resume"].append(_resume_first(eng, prompt, codes, 7))
            assert worst <= 1.0, worst
            med = {k: statistics.median(v) for k, v in res.items()}
            print(json.dumps({"n": n, "score_width": eng.score_width(), "n_prompt": int(prompt.shape[0]), "rounds": a.rounds,
                              "score_ms": round(med["score"], 3), "score_ms_per_frame": round(med["score"] / n, 4),
                              "regenerate_recording_ms": round(med["regenerate"], 3), "resume_first_new_frame_ms": round(med["resume"], 3),
                              "worst_vs_recorded_of_2e-5_bound": round(worst, 4)}), flush=True)
    finally:
        eng.sched_stop()
        eng.close()


if __name__ == "__main__":
    main()
