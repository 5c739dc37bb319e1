"""Cost of the [EXT] streaming-text talker input, alternated in one process on one GPU (full-size model, EOS masked, codec on):
  C3 shape: 64 utterances (text lengths 16 / 32 / 64) through 64 slots, talker sampling (T 0.9, top-k 50); every request in the streaming
            layout (q3tts_prompt_build_streaming + trailing ids) against every request in the reference layout, same texts and seeds
  C2 shape: time to first chunk of a single 32-token utterance through a 1-slot engine, both layouts
Prints one JSON line per run and a summary line (medians; the streaming / reference frame-time ratio).
Usage: python scripts/bench_text_stream.py [--model-dir DIR] [--frames 64] [--rounds 3] [--only stream|ref]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--only", default="", choices=["", "stream", "ref"], help="run one layout's C3 leg once (for a kernel trace)")
    args = ap.parse_args()
    import q3tts as Q
    model = args.model_dir
    if not model:
        import synth_models
        model = synth_models.full("q8_0")
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=args.slots, max_prompt=1024, max_steps=args.frames, load_codec=True)
    texts = [np.random.default_rng(42 + i).integers(0, 4000, (16, 32, 64)[i % 3]).astype(np.int32) for i in range(args.slots)]
    layouts = {"ref": ([eng.assets.build_core(t, lang_id=2055, spk_emb=spk) for t in texts], None)}
    built = [eng.assets.prompt_build_streaming(t, lang_id=2055, spk_emb=spk) for t in texts]
    layouts["stream"] = ([b[0] for b in built], [b[1] for b in built])
    names = [args.only] if args.only else ["ref", "stream"]
    rounds = 1 if args.only else args.rounds
    seeds = list(range(args.slots))
    for name in names:   # warm-up: captures every frame graph the run uses (and uploads the text table for the streaming layout)
        eng.generate_batch(layouts[name][0], max_steps=4, seed=seeds, mask_eos=True, want_pcm=True, trailing_ids=layouts[name][1], **SAMPLING)
    res = {n: [] for n in names}
    for r in range(rounds):
        for name in names:
            eng.reset_stats()
            t0 = time.perf_counter()
            out = eng.generate_batch(layouts[name][0], max_steps=args.frames, seed=[1000 * r + i for i in range(args.slots)], mask_eos=True,
                                     want_pcm=True, trailing_ids=layouts[name][1], **SAMPLING)
            wall = time.perf_counter() - t0
            st = eng.stats()
            line = {"leg": "c3", "layout": name, "round": r, "ms_per_graph_frame": st["frame_loop_ms"] / max(st["graph_frames"], 1),
                    "prefill_ms": st["prefill_ms"], "audio_s_per_s": sum(o["pcm"].size for o in out) / 24000.0 / wall, "wall_s": wall,
                    "slots": args.slots, "frames": args.frames}
            res[name].append(line)
            print(json.dumps(line), flush=True)
    eng.close()
    summ = {n: {"ms_per_graph_frame": statistics.median(x["ms_per_graph_frame"] for x in v),
                "prefill_ms": statistics.median(x["prefill_ms"] for x in v)} for n, v in res.items()}
    if not args.only:
        summ["stream_over_ref_frame_time"] = summ["stream"]["ms_per_graph_frame"] / summ["ref"]["ms_per_graph_frame"]
        e1 = Q.Engine(model, "q8_0", max_batch=1, max_prompt=1024, max_steps=16, load_codec=True)
        t = texts[1]
        c2 = {"ref": (e1.assets.build_core(t, lang_id=2055, spk_emb=spk), None)}
        c2["stream"] = e1.assets.prompt_build_streaming(t, lang_id=2055, spk_emb=spk)
        lat = {n: [] for n in c2}
        for name in c2:   # warm-up
            e1.generate_batch([c2[name][0]], max_steps=8, want_pcm=True, trailing_ids=[c2[name][1]])
        for r in range(5):
            for name in ("ref", "stream"):
                o = e1.generate_batch([c2[name][0]], max_steps=8, seed=r, want_pcm=True, trailing_ids=[c2[name][1]], **SAMPLING)[0]
                lat[name].append(o["first_chunk_ms"])
                print(json.dumps({"leg": "c2", "layout": name, "round": r, "first_chunk_ms": o["first_chunk_ms"], "prefill_ms": o["prefill_ms"],
                                  "n_prompt": int(c2[name][0].shape[0])}), flush=True)
        e1.close()
        summ["c2_first_chunk_ms"] = {n: statistics.median(v) for n, v in lat.items()}
    print(json.dumps({"summary": summ}), flush=True)


if __name__ == "__main__":
    main()
