"""Cost of [EXT] volume (q3tts_engine_set_volume), full-size model, Q8_0, one 16-slot engine with its codec, the scheduler stepped by this
thread.  16 sampled requests with PCM run side by side for --frames frames, so every codec pass carries 16 streams; the arms -- native,
-6 dB (the limiter never engages), +12 dB, +12 dB in front of the converter (16000 Hz s16) and +12 dB in front of the stretcher (rate 125)
-- are interleaved on the one engine, --rounds times after a warm-up of each.  One JSON line per arm: submit to all DONE (median, min, max),
the same per codec pass of 16 streams and its difference from the native arm, the stage's counters, the samples delivered.
Usage: python scripts/bench_volume.py [--model-dir DIR] [--rounds 2] [--frames 64]"""
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
# (name, volume in tenths of a dB, output format or None, rate)
ARMS = [("native", 0, None, 100), ("minus_6_db", -60, None, 100), ("plus_12_db", 120, None, 100), ("plus_12_db_16k_s16", 120, (16000, 1), 100),
        ("plus_12_db_rate_125", 120, None, 125)]
N = 16


def _run(eng, prompts, frames, vol, fmt, rate):
    v0, c0 = eng.volume_stats(), eng.stats()["codec_calls"]
    if fmt:
        eng.set_output_format(*fmt)
    eng.set_speech_rate(rate)
    eng.set_volume(vol)
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=100 + i, mask_eos=True, want_pcm=True, **SAMPLING) for i, p in enumerate(prompts)]
    eng.set_volume(0)
    eng.set_speech_rate(100)
    eng.set_output_format(None)
    while not all(eng.poll(r)["state"] in ENDED for r in ids):
        assert time.perf_counter() - t0 < 300.0, "requests did not end"
        eng.sched_step()
    ms = (time.perf_counter() - t0) * 1e3
    n_pcm = sum(eng.poll(r)["n_pcm"] for r in ids)
    for r in ids:
        eng.release(r)
    v1 = eng.volume_stats()
    return ms, {k: v1[k] - v0[k] for k in v1}, n_pcm, eng.stats()["codec_calls"] - c0


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
        for _, vol, fmt, rate in ARMS:                                       # warm-up: graphs captured, tables uploaded, state allocated
            _run(eng, prompts, a.frames, vol, fmt, rate)
        res = {arm[0]: [] for arm in ARMS}
        for _ in range(a.rounds):
            for name, vol, fmt, rate in ARMS:
                res[name].append(_run(eng, prompts, a.frames, vol, fmt, rate))
        passes = -(-a.frames // 4)
        base = statistics.median([r[0] for r in res["native"]])
        for name, vol, fmt, rate in ARMS:
            ms = [r[0] for r in res[name]]
            med = statistics.median(ms)
            last = res[name][-1]
            print(json.dumps({"measure": "engine", "arm": name, "volume_db10": vol, "format": list(fmt) if fmt else None, "rate_pct": rate,
                              "streams": N, "frames": a.frames, "rounds": a.rounds, "submit_to_done_ms": round(med, 3),
                              "min_max_ms": [round(min(ms), 3), round(max(ms), 3)], "ms_per_pass_of_16": round(med / passes, 4),
                              "ms_per_pass_over_native": round((med - base) / passes, 4), "codec_chunk_decodes": last[3], "volume": last[1],
                              "samples_delivered": last[2]}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
