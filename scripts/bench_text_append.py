"""Cost of [EXT] live text append (q3tts_submit_trailing_open / q3tts_text_append), full-size model, Q8_0, 64 slots, codec on, EOS masked,
talker T 0.9 / top-k 50, rounds interleaved in one process on one GPU:
  (a) gate: every request open but fed ahead (trail longer than the run, never closed), so the gated frame graph runs and nothing waits,
      against the same texts submitted closed; frame time per graph replay
  (b) feed: a feeder thread appends one text token per stream every 1/R s (R text tokens/s per stream) to text-level open requests;
      time from the first id to the first audio chunk, audio-s/s, and the share of slot-frames that produced no frame
      (1 - frames / slot_frames: waiting slots plus graph width past the last live slot)
Prints one JSON line per run and a summary line with medians.
Usage: python scripts/bench_text_append.py [--model-dir DIR] [--frames 64] [--rounds 3] [--rates 10,25,50] [--only gate|feed]"""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
SAMPLING = dict(temperature=0.9, top_k=50, top_p=1.0)


def _gate_leg(eng, prompts, trails, frames, seeds, open_trail):
    eng.reset_stats()
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=s, mask_eos=True, want_pcm=True, trailing_ids=t, open_trail=open_trail, **SAMPLING)
           for p, t, s in zip(prompts, trails, seeds)]
    for rid in ids:
        assert eng.wait(rid, 600000)
    pcm = sum(eng.result(rid, want_pcm=True)["pcm"].size for rid in ids)
    wall = time.perf_counter() - t0
    st = eng.stats()
    return {"ms_per_graph_frame": st["frame_loop_ms"] / max(st["graph_frames"], 1), "audio_s_per_s": pcm / 24000.0 / wall, "wall_s": wall}


def _feed_leg(eng, vid, texts, frames, seeds, rate):
    eng.reset_stats()
    t0 = time.perf_counter()
    ids = [eng.submit_text(vid, t[:1], max_steps=frames, seed=s, mask_eos=True, want_pcm=True, streaming_text=True, open_text=True, **SAMPLING)
           for t, s in zip(texts, seeds)]

    def feeder():
        for j in range(1, max(len(t) for t in texts)):
            time.sleep(1.0 / rate)
            for rid, t in zip(ids, texts):
                if j < len(t):
                    eng.text_append(rid, t[j:j + 1], is_last=(j == len(t) - 1))
    th = threading.Thread(target=feeder)
    th.start()
    th.join()
    for rid in ids:
        assert eng.wait(rid, 600000)
    res = [eng.result(rid, want_pcm=True) for rid in ids]
    wall = time.perf_counter() - t0
    st = eng.stats()
    return {"first_chunk_ms": statistics.median(r["first_chunk_ms"] for r in res), "audio_s_per_s": sum(r["pcm"].size for r in res) / 24000.0 / wall,
            "no_frame_share": 1.0 - st["frames"] / max(st["slot_frames"], 1.0), "wall_s": wall}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--rates", default="10,25,50")
    ap.add_argument("--only", default="", choices=["", "gate", "feed"])
    args = ap.parse_args()
    import q3tts as Q
    model = args.model_dir
    if not model:
        import synth_models
        model = synth_models.full("q8_0")
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=args.slots, max_prompt=1024, max_steps=args.frames, load_codec=True)
    vid = eng.register_voice(spk)
    seeds = list(range(args.slots))
    # (a) trails longer than the run: an open request never waits and is never closed (it ends at max_steps)
    long_texts = [np.random.default_rng(42 + i).integers(0, 4000, args.frames + 8).astype(np.int32) for i in range(args.slots)]
    built = [eng.assets.prompt_build_streaming(t, lang_id=2055, spk_emb=spk) for t in long_texts]
    prompts, trails = [b[0] for b in built], [b[1] for b in built]
    # (b) 32 text tokens per stream
    texts = [np.random.default_rng(7 + i).integers(0, 4000, 32).astype(np.int32) for i in range(args.slots)]
    rates = [float(r) for r in args.rates.split(",")]
    eng.sched_start()
    res = {}
    try:
        for op in (False, True):   # warm-up: captures the frame graphs of both legs
            _gate_leg(eng, prompts, trails, 8, seeds, op)
        for r in range(args.rounds):
            if args.only in ("", "gate"):
                for name, op in (("closed", False), ("open", True)):
                    line = {"leg": "gate", "trail": name, "round": r, "slots": args.slots, "frames": args.frames,
                            **_gate_leg(eng, prompts, trails, args.frames, [1000 * r + s for s in seeds], op)}
                    res.setdefault(("gate", name), []).append(line)
                    print(json.dumps(line), flush=True)
            if args.only in ("", "feed"):
                for rate in rates:
                    line = {"leg": "feed", "tokens_per_s": rate, "round": r, "slots": args.slots, "frames": args.frames,
                            **_feed_leg(eng, vid, texts, args.frames, [1000 * r + s for s in seeds], rate)}
                    res.setdefault(("feed", rate), []).append(line)
                    print(json.dumps(line), flush=True)
    finally:
        eng.sched_stop()
    eng.close()
    summ = {}
    for (leg, key), v in res.items():
        fields = ("ms_per_graph_frame", "audio_s_per_s") if leg == "gate" else ("first_chunk_ms", "audio_s_per_s", "no_frame_share")
        summ["%s_%s" % (leg, key)] = {f: statistics.median(x[f] for x in v) for f in fields}
    if ("gate", "open") in res and ("gate", "closed") in res:
        summ["open_over_closed_frame_time"] = summ["gate_open"]["ms_per_graph_frame"] / summ["gate_closed"]["ms_per_graph_frame"]
    print(json.dumps({"summary": summ}), flush=True)


if __name__ == "__main__":
    main()
