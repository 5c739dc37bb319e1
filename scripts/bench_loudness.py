"""Cost of [EXT] loudness (q3tts_engine_set_loudness), full-size model, Q8_0, one engine of --streams slots with its codec and codec passes
of --streams streams (Q3_CODEC_GROUP), the scheduler stepped by this thread.  --streams sampled requests with PCM run side by side for
--frames frames; the two arms -- unmetered and metered -- are interleaved on the one engine, --rounds times after a warm-up of each.  One
JSON line per arm: submit to all DONE (median, min, max), the same per codec pass and its difference from the unmetered arm, the meter's
counters.  --trace: one metered run alone, no timing, for a kernel trace of its own (rocprofv3 --kernel-trace --stats -- python this ...).
Usage: python scripts/bench_loudness.py [--model-dir DIR] [--streams 16] [--rounds 2] [--frames 64] [--trace]"""
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


def _run(eng, prompts, frames, metered):
    l0, c0 = eng.loudness_stats(), eng.stats()["codec_calls"]
    eng.set_loudness(metered)
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=100 + i, mask_eos=True, want_pcm=True, **SAMPLING) for i, p in enumerate(prompts)]
    eng.set_loudness(False)
    while not all(eng.poll(r)["state"] in ENDED for r in ids):
        assert time.perf_counter() - t0 < 300.0, "requests did not end"
        eng.sched_step()
    ms = (time.perf_counter() - t0) * 1e3
    lufs = [eng.request_loudness(r)["integrated_lufs"] for r in ids] if metered else []
    for r in ids:
        eng.release(r)
    l1 = eng.loudness_stats()
    return ms, {k: l1[k] - l0[k] for k in l1}, eng.stats()["codec_calls"] - c0, lufs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    os.environ["Q3_CODEC_GROUP"] = str(a.streams)   # read once, when the first engine is made
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    N = a.streams
    eng = Q.Engine(model, "q8_0", max_batch=N, max_prompt=512, max_steps=a.frames + 2, load_codec=True)
    rng = np.random.default_rng(1)
    prompts = [eng.assets.build_core(rng.integers(0, 4000, 8 + i % 5).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(N)]
    try:
        if a.trace:
            ms, loud, calls, lufs = _run(eng, prompts, a.frames, True)
            print(json.dumps({"measure": "trace", "streams": N, "frames": a.frames, "codec_chunk_decodes": calls, "loudness": loud}), flush=True)
            return
        for metered in (False, True):                                        # warm-up: graphs captured, the stage and its buffers made
            _run(eng, prompts, a.frames, metered)
        res = {False: [], True: []}
        for _ in range(a.rounds):
            for metered in (False, True):
                res[metered].append(_run(eng, prompts, a.frames, metered))
        passes = -(-a.frames // 4)
        base = statistics.median([r[0] for r in res[False]])
        for metered in (False, True):
            ms = [r[0] for r in res[metered]]
            med = statistics.median(ms)
            last = res[metered][-1]
            print(json.dumps({"measure": "engine", "arm": "metered" if metered else "unmetered", "streams": N, "frames": a.frames, "rounds": a.rounds,
                              "submit_to_done_ms": round(med, 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)],
                              "ms_per_pass": round(med / passes, 4), "ms_per_pass_over_unmetered": round((med - base) / passes, 4),
                              "codec_chunk_decodes": last[2], "loudness": last[1],
                              "integrated_lufs_min_max": [round(min(last[3]), 2), round(max(last[3]), 2)] if last[3] else None}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
