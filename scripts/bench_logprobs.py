"""Cost of recording [EXT] token log-probabilities (q3tts_engine_set_logprobs) on the C3-shaped workload of scripts/bench_gen_options.py: 64
utterances through 64 slots of the full-size model, EOS masked, codec on, recording off / on alternated on one engine, for two settings:
  a_talker_sampled   talker T 0.9 / top-k 50, greedy predictor: recording also moves the 15 predictor heads from their fused argmax epilogue
                     to logits + k_sample_pred (first-max branch), + k_logprob_rows                  -> +16 launches per frame
  c_plus_predictor   upstream's settings (penalty 1.05, sampled predictor): every head writes logits already -> +1 launch per frame
(a greedy batch pays +17: the talker head leaves its argmax epilogue too).  The launch counts are read off Engine::record_frame, not
measured.  Requests go through submit (q3tts_generate_batch never records) and the scheduler is stepped by this thread.
Prints one JSON line per run and a summary line (median ms per graph frame per leg, on / off ratio).
Usage: python scripts/bench_logprobs.py [--model-dir DIR] [--frames 64] [--rounds 2] [--slots 64]"""
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
    "a_talker_sampled": (dict(temperature=0.9, top_k=50, top_p=1.0), 16),
    "c_plus_predictor": (dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50,
                              predictor_top_p=0.8), 1),
}


def run(eng, prompts, frames, seeds, kw, record):
    eng.set_logprobs(record)
    eng.reset_stats()
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=s, mask_eos=True, want_pcm=True, **kw) for p, s in zip(prompts, seeds)]
    while eng.sched_step():
        pass
    wall = time.perf_counter() - t0
    st = eng.stats()
    out = [eng.result(r, want_pcm=True) for r in ids]
    assert all(("logprobs" in o) == record for o in out)
    if record:
        lp = np.concatenate([o["logprobs"] for o in out])
        assert lp.shape == (sum(o["codes"].shape[0] for o in out), 17) and np.all(lp <= 0.0)
    audio_s = sum(o["pcm"].size for o in out) / 24000.0
    return {"ms_per_graph_frame": st["frame_loop_ms"] / max(st["graph_frames"], 1), "audio_s_per_s": audio_s / wall, "wall_s": wall,
            "graph_frames": st["graph_frames"]}, [o["codes"] for o in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--slots", type=int, default=64)
    args = ap.parse_args()
    import q3tts as Q
    model = args.model_dir
    if not model:
        import synth_models
        model = synth_models.full("q8_0")
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=args.slots, max_prompt=1024, max_steps=args.frames, load_codec=True)
    prompts = [eng.assets.build_core(np.random.default_rng(42 + i).integers(0, 4000, (16, 32, 64)[i % 3]).astype(np.int32), lang_id=2055,
                                     spk_emb=spk) for i in range(args.slots)]
    for name, (kw, _) in SETTINGS.items():   # warm-up: captures every frame graph the run uses
        for record in (False, True):
            run(eng, prompts, 4, list(range(args.slots)), kw, record)
    res = {(n, rec): [] for n in SETTINGS for rec in (False, True)}
    for r in range(args.rounds):
        for name, (kw, extra) in SETTINGS.items():
            codes = {}
            for record in (False, True):
                line, codes[record] = run(eng, prompts, args.frames, [1000 * r + i for i in range(args.slots)], kw, record)
                line.update(setting=name, recording=record, round=r, slots=args.slots, frames=args.frames, extra_launches_per_frame=extra if record else 0)
                res[(name, record)].append(line)
                print(json.dumps(line), flush=True)
            assert all(np.array_equal(a, b) for a, b in zip(codes[False], codes[True])), "recording changed the codes"
    summ = {}
    for name in SETTINGS:
        off = statistics.median(x["ms_per_graph_frame"] for x in res[(name, False)])
        on = statistics.median(x["ms_per_graph_frame"] for x in res[(name, True)])
        summ[name] = {"off_ms_per_graph_frame": off, "on_ms_per_graph_frame": on, "on_over_off": on / off, "extra_launches_per_frame": SETTINGS[name][1]}
    print(json.dumps({"summary": summ}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
