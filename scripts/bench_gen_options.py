"""Cost of the [EXT] generation controls on a C3-shaped workload: 64 utterances through 64 slots of the full-size model, EOS masked,
codec on, three settings alternated on one GPU:
  (a) talker sampling only (T 0.9, top-k 50)                      -- the sampled path that exists without the options
  (b) (a) + repetition penalty 1.05
  (c) (b) + sampled code predictor (T 0.9, top-k 50, top-p 0.8)   -- upstream's settings
Prints one JSON line per run and a summary line (median ms per graph frame and audio-s/s per setting).
Usage: python scripts/bench_gen_options.py [--model-dir DIR] [--frames 64] [--rounds 3]"""
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

SETTINGS = {
    "a_talker_sampled": dict(temperature=0.9, top_k=50, top_p=1.0),
    "b_plus_penalty": dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05),
    "c_plus_predictor": dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50,
                             predictor_top_p=0.8),
}


def kernel_times(Q, B):
    """back-to-back launches of one sampler kernel over B rows of 2048 logits (q3tts_op_sample_rows: the frame graph's argument packing);
    per-launch time = (wall of 420 draws - wall of 20 draws) / 400, which cancels the entry point's allocations and copies"""
    lg = np.random.default_rng(1).standard_normal((B, 2048)).astype(np.float32) * 3
    for kernel, name in ((0, "k_sample"), (1, "k_sample_pred")):
        for T, k, p in ((0.9, 50, 0.8), (0.9, 0, 1.0), (0.0, 0, 1.0)):
            walls = []
            for n in (20, 420):
                Q.op_sample_rows(lg, T, k, p, 7, n_draws=n, kernel=kernel)   # warm
                t0 = time.perf_counter()
                Q.op_sample_rows(lg, T, k, p, 7, n_draws=n, kernel=kernel)
                walls.append(time.perf_counter() - t0)
            print(json.dumps({"kernel": name, "B": B, "T": T, "top_k": k, "top_p": p, "us_per_launch": 1e6 * (walls[1] - walls[0]) / 400}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--only", default="", help="run one setting once (for a kernel trace)")
    ap.add_argument("--kernel-times", action="store_true", help="only time k_sample vs k_sample_pred launches at B = slots")
    args = ap.parse_args()
    import q3tts as Q
    if args.kernel_times:
        kernel_times(Q, args.slots)
        return
    model = args.model_dir
    if not model:
        import synth_models
        model = synth_models.full("q8_0")
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=args.slots, max_prompt=1024, max_steps=args.frames, load_codec=True)
    prompts = [eng.assets.build_core(np.random.default_rng(42 + i).integers(0, 4000, (16, 32, 64)[i % 3]).astype(np.int32), lang_id=2055,
                                     spk_emb=spk) for i in range(args.slots)]
    names = [args.only] if args.only else list(SETTINGS)
    rounds = 1 if args.only else args.rounds
    for name in names:   # warm-up: captures every frame graph the run uses
        eng.generate_batch(prompts, max_steps=4, seed=list(range(args.slots)), mask_eos=True, want_pcm=True, **SETTINGS[name])
    res = {n: [] for n in names}
    for r in range(rounds):
        for name in names:
            eng.reset_stats()
            t0 = time.perf_counter()
            out = eng.generate_batch(prompts, max_steps=args.frames, seed=[1000 * r + i for i in range(args.slots)], mask_eos=True,
                                     want_pcm=True, **SETTINGS[name])
            wall = time.perf_counter() - t0
            st = eng.stats()
            audio_s = sum(o["pcm"].size for o in out) / 24000.0
            line = {"setting": name, "round": r, "ms_per_graph_frame": st["frame_loop_ms"] / max(st["graph_frames"], 1),
                    "audio_s_per_s": audio_s / wall, "wall_s": wall, "slots": args.slots, "frames": args.frames}
            res[name].append(line)
            print(json.dumps(line), flush=True)
    summ = {n: {"ms_per_graph_frame": statistics.median(x["ms_per_graph_frame"] for x in v),
                "audio_s_per_s": statistics.median(x["audio_s_per_s"] for x in v)} for n, v in res.items()}
    if "a_talker_sampled" in summ and "c_plus_predictor" in summ:
        summ["c_over_a_frame_time"] = summ["c_plus_predictor"]["ms_per_graph_frame"] / summ["a_talker_sampled"]["ms_per_graph_frame"]
    print(json.dumps({"summary": summ}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
