"""Cost of [EXT] prompt stems (q3tts_stem_*), full-size model, Q8_0, codes only, the scheduler stepped by this thread, the two arms
interleaved round by round in one process on one GPU.  The prompts are a 300-row head followed by 30 rows of their own:
  (a) stem:   the head is a READY stem set at engine level; every submission takes it,
  (b) plain:  the same submissions with no stem set (the parent commit's only way; this path is unchanged).
Measured, medians over the rounds after one warm-up of each arm:
  first     submit until every request has its first frame (q3tts_poll n_frames > 0), n = 1 and n = 64 requests, on an idle engine (an
            in-line wave) and beside 32 running slots (an asynchronous wave); the engine's prefill_ms (HIP events) over the same span; the
            time of the q3tts_submit calls themselves (the memcmp of the take rule runs there)
  all_done  submit until all of 64 requests of 64 frames are DONE
  build     q3tts_stem_create until READY
The codes of both arms are compared bit for bit in every round.  Prints one JSON line per measurement.  --only-restore runs a few stemmed
waves and nothing else (for a kernel trace of k_kv_stem).
Usage: python scripts/bench_stem.py [--model-dir DIR] [--rounds 5] [--head 300] [--tail 30] [--only-restore]"""
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


def _first_frames(eng, ids, t0):
    while any(eng.poll(r)["n_frames"] == 0 for r in ids):
        assert time.perf_counter() - t0 < 120.0, "no first frame"
        eng.sched_step()
    return (time.perf_counter() - t0) * 1e3


def _all_done(eng, ids, t0):
    while any(eng.poll(r)["state"] not in (3, 4, -1) for r in ids):
        assert time.perf_counter() - t0 < 300.0, "not done"
        eng.sched_step()
    return (time.perf_counter() - t0) * 1e3


def _round(eng, prompts, sid, frames, background, until_done):
    """one measurement: `background` running requests first (one frame group each), then the prompts, stemmed (sid) or plain (None)"""
    bg = [eng.submit(p, max_steps=400, seed=1000 + i, mask_eos=True, **SAMPLING) for i, p in enumerate(background)]
    if bg:
        _first_frames(eng, bg, time.perf_counter())
    eng.set_stem(sid)
    pf0 = eng.stats()["prefill_ms"]
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=7000 + i, mask_eos=True, **SAMPLING) for i, p in enumerate(prompts)]
    submit_ms = (time.perf_counter() - t0) * 1e3
    eng.set_stem(None)
    assert all(eng.request_stem(r) == ((sid, eng.stem_poll(sid)[1]) if sid is not None else (-1, 0)) for r in ids)
    first = _first_frames(eng, ids, t0)
    pf = eng.stats()["prefill_ms"] - pf0
    done = _all_done(eng, ids, t0)
    codes = [eng.result(r)["codes"] for r in ids]
    for r in bg:
        eng.cancel(r)
    while eng.sched_step():
        pass
    for r in bg:
        eng.release(r)
    return dict(first=first, prefill=pf, submit=submit_ms, done=done if until_done else 0.0), codes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--head", type=int, default=300)
    ap.add_argument("--tail", type=int, default=30)
    ap.add_argument("--only-restore", action="store_true")
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=96, max_prompt=512, max_steps=400, load_codec=False)
    rng = np.random.default_rng(1)
    base = eng.assets.build_core(rng.integers(0, 4000, 24).astype(np.int32), lang_id=2055, spk_emb=spk)
    head = np.ascontiguousarray(base[np.arange(a.head) % base.shape[0]], np.float32)
    prompts = [np.concatenate([head, np.ascontiguousarray(base[(np.arange(a.tail) + 3 * i) % base.shape[0]] * np.float32(1.0 + i / 256.0), np.float32)])
               for i in range(64)]
    background = [eng.assets.build_core(rng.integers(0, 4000, 8 + i % 5).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(32)]
    try:
        builds = []
        for _ in range(max(1, a.rounds if not a.only_restore else 1)):
            t0 = time.perf_counter()
            sid = eng.stem_create(head)
            assert eng.stem_wait(sid, 60000.0) and eng.stem_poll(sid)[0] == Q.STEM_READY
            builds.append((time.perf_counter() - t0) * 1e3)
            if len(builds) < max(1, a.rounds if not a.only_restore else 1):
                eng.stem_release(sid)
                eng.sched_step()
        if a.only_restore:
            for _ in range(4):
                _round(eng, prompts, sid, 4, [], False)
            print(json.dumps({"only_restore": True, "stats": eng.stem_stats()}), flush=True)
            return
        print(json.dumps({"what": "build", "head_rows": a.head, "rounds": a.rounds, "build_ms": round(statistics.median(builds), 3),
                          "device_bytes": eng.stem_stats()["device_bytes"]}), flush=True)
        for what, n, nb, frames, until_done in (("first", 1, 0, 8, False), ("first", 64, 0, 8, False), ("first", 1, 32, 8, False),
                                                ("first", 64, 32, 8, False), ("all_done", 64, 0, 64, True)):
            ps, bg = prompts[:n], background[:nb]
            _round(eng, ps, sid, frames, bg, until_done)                      # warm-up: graphs of these widths captured
            _round(eng, ps, None, frames, bg, until_done)
            res = {"stem": [], "plain": []}
            for _ in range(a.rounds):
                m, got = _round(eng, ps, sid, frames, bg, until_done)
                res["stem"].append(m)
                m, want = _round(eng, ps, None, frames, bg, until_done)
                res["plain"].append(m)
                assert all(np.array_equal(g, w) for g, w in zip(got, want)), "a stemmed request differs from its plain submission"
            out = {"what": what, "requests": n, "running_slots": nb, "frames": frames, "head_rows": a.head, "tail_rows": a.tail, "rounds": a.rounds}
            for arm in ("stem", "plain"):
                for k in ("first", "prefill", "submit") + (("done",) if until_done else ()):
                    vals = [m[k] for m in res[arm]]
                    out["%s_%s_ms" % (arm, k)] = round(statistics.median(vals), 3)
                    out["%s_%s_spread_ms" % (arm, k)] = [round(min(vals), 3), round(max(vals), 3)]
            print(json.dumps(out), flush=True)
        print(json.dumps({"what": "stats", **eng.stem_stats()}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
