"""Cost of [EXT] pitch (q3tts_engine_set_pitch), full-size model, Q8_0, one 16-slot engine with its codec, the scheduler stepped by this
thread.  16 sampled requests with PCM run side by side for --frames frames, so every codec pass carries 16 streams; the arms -- native, rate
125 alone (the stretcher's kernel), pitch 80 alone (the same tempo 1.25, so the same WSOLA work plus stage 2), pitch 107 and pitch 50 --
are interleaved on the one engine, --rounds times after a warm-up of each.  The engine's max_steps is --frames + 2: a request with a pitch
delivers the native duration and at most a hop more.  One JSON line per arm: submit to all DONE (median, min, max), the same per codec pass
of 16 streams and its difference from the native arm, the stretcher's and the shifter's counters, the samples delivered.
Usage: python scripts/bench_pitch.py [--model-dir DIR] [--rounds 2] [--frames 64]"""
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
ENDED = (3, 4, -1)
ARMS = [("native", 100, 100), ("rate_125", 125, 100), ("pitch_80", 100, 80), ("pitch_107", 100, 107), ("pitch_50", 100, 50)]
N = 16


def _run(eng, prompts, frames, rate, pitch):
    t0s, p0s, c0 = eng.tsm_stats(), eng.pitch_stats(), eng.stats()["codec_calls"]
    eng.set_speech_rate(rate)
    eng.set_pitch(pitch)
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=100 + i, mask_eos=True, want_pcm=True, **SAMPLING) for i, p in enumerate(prompts)]
    eng.set_pitch(100)
    eng.set_speech_rate(100)
    while not all(eng.poll(r)["state"] in ENDED for r in ids):
        assert time.perf_counter() - t0 < 300.0, "requests did not end"
        eng.sched_step()
    ms = (time.perf_counter() - t0) * 1e3
    n_pcm = sum(eng.poll(r)["n_pcm"] for r in ids)
    for r in ids:
        eng.release(r)
    t1s, p1s = eng.tsm_stats(), eng.pitch_stats()
    return (ms, {k: t1s[k] - t0s[k] for k in t1s}, {k: p1s[k] - p0s[k] for k in p1s if k != "table_bytes"}, n_pcm,
            eng.stats()["codec_calls"] - c0, p1s["table_bytes"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=64)
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=N, max_prompt=512, max_steps=a.frames + 2, load_codec=True)
    rng = np.random.default_rng(1)
    prompts = [eng.assets.build_core(rng.integers(0, 4000, 8 + i % 5).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(N)]
    try:
        for _, rate, pitch in ARMS:                                          # warm-up: graphs captured, tables uploaded, state allocated
            _run(eng, prompts, a.frames, rate, pitch)
        res = {name: [] for name, _, _ in ARMS}
        for _ in range(a.rounds):
            for name, rate, pitch in ARMS:
                res[name].append(_run(eng, prompts, a.frames, rate, pitch))
        passes = -(-a.frames // 4)
        base = statistics.median([r[0] for r in res["native"]])
        for name, rate, pitch in ARMS:
            ms = [r[0] for r in res[name]]
            med = statistics.median(ms)
            last = res[name][-1]
            print(json.dumps({"measure": "engine", "arm": name, "rate_pct": rate, "pitch_pct": pitch, "streams": N, "frames": a.frames,
                              "rounds": a.rounds, "submit_to_done_ms": round(med, 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)],
                              "ms_per_pass_of_16": round(med / passes, 4), "ms_per_pass_over_native": round((med - base) / passes, 4),
                              "codec_chunk_decodes": last[4], "tsm": last[1], "pitch": last[2], "table_bytes": last[5],
                              "samples_delivered": last[3]}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
