"""Cost of [EXT] codec preambles (q3tts_preamble_*), full-size model, Q8_0, one 4-slot engine with its codec, the scheduler stepped by this
thread.  One greedy request with PCM at a time, --frames frames; the arms -- unprimed, primed behind a preamble of 64 frames, primed behind
one of 256 -- are interleaved on the one engine, --rounds times after a warm-up of each.  One JSON line per arm: first_chunk_ms and submit
to DONE (median, min, max).  Then the build of a preamble, create to READY, per length (median of --rounds builds after one warm-up), the
device bytes of one snapshot and the restores the engine counted.
--trace-run: the short form for a kernel trace taken in a run of its own, on the stand-alone decoder at full size (no engine: a kernel
trace of the engine's graph replay has ended in a segmentation fault inside the HIP runtime under the tool, DESIGN.md "Sampler"): 64
frames decoded on stream 0, then --rounds times one snapshot and three restores into stream 1, each followed by a 4-frame decode --
k_hist_copy in both directions, on a cold and on a just-written store.
Usage: python scripts/bench_preamble.py [--model-dir DIR] [--rounds 5] [--frames 16] [--trace-run]"""
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
ENDED = (3, 4, -1)
LENGTHS = (64, 256)


def _run(eng, prompt, frames, pid):
    eng.set_preamble(pid)
    t0 = time.perf_counter()
    rid = eng.submit(prompt, max_steps=frames, seed=7, mask_eos=True, want_pcm=True)
    eng.set_preamble(None)
    while eng.poll(rid)["state"] not in ENDED:
        assert time.perf_counter() - t0 < 300.0, "the request did not end"
        eng.sched_step()
    ms = (time.perf_counter() - t0) * 1e3
    assert eng.request_preamble(rid) == (-1 if pid is None else pid)
    r = eng.result(rid, want_pcm=True)
    assert r["state"] == 3 and r["pcm"].size == frames * 1920
    return ms, r["first_chunk_ms"], r


def _build(eng, codes):
    t0 = time.perf_counter()
    pid = eng.preamble_create(codes)
    assert eng.preamble_wait(pid, 300000.0) and eng.preamble_poll(pid)[0] == 1
    return pid, (time.perf_counter() - t0) * 1e3


def _mmm(v):
    return [round(statistics.median(v), 3), round(min(v), 3), round(max(v), 3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--trace-run", action="store_true")
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    if a.trace_run:
        dec = Q.Decoder(os.path.join(model, "onnx", "q3tts_codec.gguf"), n_streams=2, max_frames=4)
        rng = np.random.default_rng(1)
        ref = rng.integers(0, 2048, (64, 16)).astype(np.int64)
        try:
            for i in range(0, 64, 4):
                dec.decode(ref[i: i + 4], stream=0)
            for _ in range(a.rounds):
                snap = dec.snapshot_create(0)
                for _ in range(3):
                    dec.snapshot_restore(snap, 1)
                    dec.decode(ref[:4], stream=1)
                dec.snapshot_free(snap)
            print(json.dumps({"measure": "trace_run", "snapshots": a.rounds, "restores": 3 * a.rounds, "bytes_per_snapshot": dec.snapshot_bytes()}), flush=True)
        finally:
            dec.close()
        return
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=4, max_prompt=512, max_steps=max(LENGTHS), load_codec=True)
    rng = np.random.default_rng(1)
    prompt = eng.assets.build_core(rng.integers(0, 4000, 10).astype(np.int32), lang_id=2055, spk_emb=spk)
    ref = rng.integers(0, 2048, (max(LENGTHS), 16)).astype(np.int32)
    try:
        pids = {}
        for m in LENGTHS:
            _build(eng, ref[:m])                                             # warm-up: the slot's buffer, the pass shapes
            ms = []
            for _ in range(a.rounds):
                if m in pids:
                    eng.preamble_release(pids[m])
                pids[m], t = _build(eng, ref[:m])
                ms.append(t)
            print(json.dumps({"measure": "build", "preamble_frames": m, "rounds": a.rounds, "create_to_ready_ms": _mmm(ms),
                              "ms_per_4_frame_pass": round(statistics.median(ms) / (m // 4), 4)}), flush=True)
        arms = [("unprimed", None)] + [("primed_m%d" % m, pids[m]) for m in LENGTHS]
        for _, p in arms:                                                    # warm-up: graphs captured
            _run(eng, prompt, a.frames, p)
        res = {name: [] for name, _ in arms}
        codes = {}
        for _ in range(a.rounds):
            for name, p in arms:
                ms, first, r = _run(eng, prompt, a.frames, p)
                res[name].append((ms, first))
                codes[name] = r["codes"]
        assert all(np.array_equal(c, codes["unprimed"]) for c in codes.values())   # the codes never change
        for name, _ in arms:
            print(json.dumps({"measure": "request", "arm": name, "frames": a.frames, "rounds": a.rounds,
                              "first_chunk_ms": _mmm([r[1] for r in res[name]]), "submit_to_done_ms": _mmm([r[0] for r in res[name]])}), flush=True)
        print(json.dumps({"measure": "store", **eng.preamble_stats()}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
