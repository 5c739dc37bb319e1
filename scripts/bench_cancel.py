"""Cost of [EXT] request cancellation (q3tts_cancel), full-size model, Q8_0, 64 slots, EOS masked, talker T 0.9 / top-k 50, a running driver
thread, rounds interleaved in one process on one GPU:
  (a) latency: 64 requests run; at a fixed frame count k of them are cancelled one after the other, and for each the time from q3tts_cancel
      returning to q3tts_poll reading CANCELLED is taken (poll spins in this thread) -- for codes-only requests and for PCM requests.
      The yardstick is one frame group of the same run, frame_loop_ms / sched_steps (a cancel is honoured between two groups), plus,
      for PCM requests, one codec group pass (the fence waits for the chunk in flight): codec_group_ms is timed on the same engine as
      the wall time of a 4-frame PCM request alone minus that of the same request without PCM
  (b) survivors: the frame rate (frames of the surviving requests per second of wall time) with k of 64 cancelled mid-run against the
      same run with nobody cancelled; with 64 - k live slots the frame graph keeps its width until the high slots retire, so the
      time per graph replay is reported beside it
Prints one JSON line per run and a summary line with medians.
Usage: python scripts/bench_cancel.py [--model-dir DIR] [--frames 64] [--rounds 3] [--cancel 16] [--at 16] [--timed 8] [--only latency|survivors]"""
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


def _run(eng, Q, prompts, frames, seeds, want_pcm, doomed, at, time_each, others=None):
    """submits everything, waits until a survivor has `at` frames, cancels `doomed`; returns stats of the run.  others: the requests whose
    frames count as the survivors' (default: all but `doomed`), so that a run without cancels counts the same requests"""
    eng.reset_stats()
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=s, mask_eos=True, want_pcm=want_pcm, **SAMPLING) for p, s in zip(prompts, seeds)]
    lat, accepted = [], []
    if doomed:
        watch = ids[[i for i in range(len(ids)) if i not in doomed][0]]
        while eng.poll(watch)["n_frames"] < at:
            time.sleep(0.0005)
        if time_each:
            for i in doomed:   # one after the other: each cancel meets a scheduler that is somewhere inside a frame group
                if not eng.cancel(ids[i]):
                    continue       # the run was over before its turn came
                accepted.append(i)
                t1 = time.perf_counter()
                while eng.poll(ids[i])["state"] != Q.REQ_CANCELLED:
                    assert time.perf_counter() - t1 < 30.0, "cancel not honoured"
                lat.append((time.perf_counter() - t1) * 1e3)
        else:
            accepted = [i for i in doomed if eng.cancel(ids[i])]
    for rid in ids:
        assert eng.wait(rid, 600000)
    wall = time.perf_counter() - t0
    res = [eng.result(rid) for rid in ids]
    st = eng.stats()
    alive = [r for i, r in enumerate(res) if i not in (doomed if others is None else others)]
    assert all(r["state"] == Q.REQ_DONE and r["n_frames"] == frames for r in alive)
    assert all(res[i]["state"] == (Q.REQ_CANCELLED if i in accepted else Q.REQ_DONE) for i in doomed)
    return {"cancel_ms": lat, "frame_group_ms": st["frame_loop_ms"] / max(st["sched_steps"], 1),
            "ms_per_graph_frame": st["frame_loop_ms"] / max(st["graph_frames"], 1),
            "survivor_frames_per_s": sum(r["n_frames"] for r in alive) / wall, "wall_s": wall,
            "frames_of_cancelled": [res[i]["n_frames"] for i in accepted]}


def _codec_group_ms(eng, prompt, rounds=5):
    """one 4-frame chunk through the codec: wall time of a 4-frame request alone with PCM minus without"""
    t = {}
    for pcm in (False, True) * rounds:
        t0 = time.perf_counter()
        rid = eng.submit(prompt, max_steps=4, seed=1, mask_eos=True, want_pcm=pcm, **SAMPLING)
        assert eng.wait(rid, 600000)
        t.setdefault(pcm, []).append((time.perf_counter() - t0) * 1e3)
        eng.release(rid)
    return max(statistics.median(t[True]) - statistics.median(t[False]), 0.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--cancel", type=int, default=16, help="requests cancelled mid-run")
    ap.add_argument("--at", type=int, default=16, help="frame count at which the cancels start")
    ap.add_argument("--timed", type=int, default=8, help="latency leg: cancels timed one after the other (each takes about a frame group)")
    ap.add_argument("--only", default="", choices=["", "latency", "survivors"])
    args = ap.parse_args()
    import q3tts as Q
    model = args.model_dir
    if not model:
        import synth_models
        model = synth_models.full("q8_0")
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=args.slots, max_prompt=1024, max_steps=args.frames, load_codec=True)
    prompts = [eng.assets.build_core(np.random.default_rng(42 + i).integers(0, 4000, (16, 32, 64)[i % 3]).astype(np.int32), lang_id=2055, spk_emb=spk)
               for i in range(args.slots)]
    seeds = list(range(args.slots))
    stride = max(1, args.slots // max(args.cancel, 1))
    doomed = list(range(1, args.slots, stride))[:args.cancel]   # spread over the slots, slot 0 stays
    eng.sched_start()
    res = {}
    try:
        for pcm in (False, True):   # warm-up: captures the frame graphs, fills the codec's lanes once
            _run(eng, Q, prompts, 8, seeds, pcm, [], 0, False)
        codec_ms = _codec_group_ms(eng, prompts[0])
        print(json.dumps({"leg": "codec_group", "codec_group_ms": codec_ms}), flush=True)
        for r in range(args.rounds):
            sd = [1000 * r + s for s in seeds]
            if args.only in ("", "latency"):
                for pcm in (False, True):
                    line = {"leg": "latency", "pcm": pcm, "round": r, "slots": args.slots, "frames": args.frames, "cancelled": min(len(doomed), args.timed),
                            **_run(eng, Q, prompts, args.frames, sd, pcm, doomed[:args.timed], args.at, True)}
                    res.setdefault(("latency", pcm), []).append(line)
                    print(json.dumps(line), flush=True)
            if args.only in ("", "survivors"):
                for name, dm in (("nobody", []), ("cancelled", doomed)):
                    line = {"leg": "survivors", "run": name, "round": r, "slots": args.slots, "frames": args.frames, "cancelled": len(dm),
                            **_run(eng, Q, prompts, args.frames, sd, True, dm, args.at, False, doomed)}
                    res.setdefault(("survivors", name), []).append(line)
                    print(json.dumps(line), flush=True)
    finally:
        eng.sched_stop()
    eng.close()
    summ = {"codec_group_ms": codec_ms}
    for (leg, key), v in res.items():
        if leg == "latency":
            lat = [x for line in v for x in line["cancel_ms"]]
            summ["latency_%s" % ("pcm" if key else "codes")] = {
                "cancel_ms_median": statistics.median(lat), "cancel_ms_max": max(lat), "n": len(lat),
                "frame_group_ms": statistics.median(x["frame_group_ms"] for x in v)}
        else:
            summ["survivors_%s" % key] = {f: statistics.median(x[f] for x in v) for f in ("survivor_frames_per_s", "ms_per_graph_frame", "wall_s")}
    if ("survivors", "nobody") in res and ("survivors", "cancelled") in res:
        a, b = summ["survivors_cancelled"], summ["survivors_nobody"]   # the same requests are counted in both
        summ["survivor_rate_cancelled_over_nobody"] = a["survivor_frames_per_s"] / b["survivor_frames_per_s"]
    print(json.dumps({"summary": summ}), flush=True)


if __name__ == "__main__":
    main()
