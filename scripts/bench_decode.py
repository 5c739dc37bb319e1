"""Cost of [EXT] decoding given frames (q3tts_submit_decode), full-size model, Q8_0, one 40-slot engine with its codec, the scheduler stepped
by this thread, rounds interleaved in one process on one GPU.  Three measurements, medians over the rounds, one JSON line each:
  (a) idle:      submit -> REQ_DONE of one decode-only request of 64 and of 256 frames on the idle engine, against a standalone q3tts_decoder
                 (one stream, 4 frames a call) fed the same 4-frame chunks one synchronous call after the other; the PCM of the two is compared;
  (b) best-of-4: 4 sampled candidates of one prompt, 64 frames each, recording on -- a set with want_pcm = 1 until every member is DONE (the
                 winner's PCM is complete) against a codes-only set, the pick by summed log-probability and one q3tts_submit_decode until it is
                 DONE -- with the codec calls of each;
  (c) loaded:    8 decode-only requests of 64 frames beside 32 running slots with PCM (two full passes of 16 a frame group) and beside 24 (a
                 full pass and one with 8 seats left): submit -> REQ_DONE of each (median and last), and the share of their chunks that sat in
                 a pass with a running request's chunk (q3tts_engine_decode_stats).
Usage: python scripts/bench_decode.py [--model-dir DIR] [--rounds 5] [--running 32,24]"""
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


def _finish(eng, ids, t0=None):
    """steps the scheduler until every request has ended; ms since t0 at which each was first seen ended"""
    at = {}
    while len(at) < len(ids):
        assert t0 is None or time.perf_counter() - t0 < 120.0, "requests did not end"
        for r in ids:
            if r not in at and eng.poll(r)["state"] in ENDED:
                at[r] = (time.perf_counter() - (t0 or 0.0)) * 1e3
        if len(at) < len(ids):
            eng.sched_step()
    return [at[r] for r in ids]


def _idle_engine(eng, codes):
    t0 = time.perf_counter()
    rid = eng.submit_decode(codes)
    ms = _finish(eng, [rid], t0)[0]
    st = eng.poll(rid)
    return ms, st["first_chunk_ms"], eng.result(rid, want_pcm=True)["pcm"]


def _idle_decoder(dec, codes):
    t0 = time.perf_counter()
    dec.reset()
    pcm = [dec.decode(codes[f:f + 4], is_last=f + 4 >= codes.shape[0]) for f in range(0, codes.shape[0], 4)]
    return (time.perf_counter() - t0) * 1e3, np.concatenate(pcm)


def _best_of(eng, prompt, seeds, frames, with_pcm):
    c0 = eng.stats()["codec_calls"]
    t0 = time.perf_counter()
    ids = eng.submit_candidates(prompt, seeds, max_steps=frames, want_pcm=with_pcm, **SAMPLING)
    _finish(eng, ids, t0)
    out = [eng.result(r, want_pcm=with_pcm) for r in ids]
    best = int(np.argmax([float(np.sum(o["logprobs"][:, :16], dtype=np.float64)) for o in out]))
    if with_pcm:
        pcm = out[best]["pcm"]
    else:
        rid = eng.submit_decode(out[best]["codes"])
        _finish(eng, [rid], t0)
        pcm = eng.result(rid, want_pcm=True)["pcm"]
    return (time.perf_counter() - t0) * 1e3, eng.stats()["codec_calls"] - c0, best, pcm


def _loaded(eng, background, given):
    bg = [eng.submit(p, max_steps=400, seed=1000 + i, mask_eos=True, want_pcm=True, **SAMPLING) for i, p in enumerate(background)]
    while any(eng.poll(r)["n_frames"] < 8 for r in bg):                   # two frame groups each: the codec passes of the 32 are under way
        eng.sched_step()
    s0 = eng.decode_stats()
    t0 = time.perf_counter()
    ids = [eng.submit_decode(c) for c in given]
    ms = _finish(eng, ids, t0)
    s1 = eng.decode_stats()
    pcm = [eng.result(r, want_pcm=True)["pcm"] for r in ids]
    for r in bg:
        eng.cancel(r)
    while eng.sched_step():
        pass
    for r in bg:
        eng.release(r)
    return ms, s1["chunks"] - s0["chunks"], s1["chunks_shared"] - s0["chunks_shared"], pcm


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--running", default="32,24")
    a = ap.parse_args()
    import q3tts as Q
    import synth_models
    model = synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    eng = Q.Engine(model, "q8_0", max_batch=40, max_prompt=512, max_steps=400, load_codec=True)
    dec = Q.Decoder(os.path.join(model, "onnx", "q3tts_codec.gguf"), n_streams=1, max_frames=4)
    rng = np.random.default_rng(1)
    prompt = eng.assets.build_core(rng.integers(0, 4000, 24).astype(np.int32), lang_id=2055, spk_emb=spk)
    background = [eng.assets.build_core(rng.integers(0, 4000, 8 + i % 5).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(32)]
    rms = lambda x, y: float(np.sqrt(np.mean((x - y) ** 2))) if x.size == y.size else float("inf")
    try:
        eng.set_logprobs(True)
        # the frames every measurement decodes: one sampled request of 256 frames, and 8 of 64 for (c)
        rid = eng.submit(prompt, max_steps=256, seed=7, mask_eos=True, **SAMPLING)
        given = [eng.submit(background[i], max_steps=64, seed=50 + i, mask_eos=True, **SAMPLING) for i in range(8)]
        _finish(eng, [rid] + given)
        long = eng.result(rid)["codes"]
        given = [eng.result(r)["codes"] for r in given]
        # (a)
        for n in (64, 256):
            _idle_engine(eng, long[:n]), _idle_decoder(dec, long[:n])       # warm-up
            e, f, d, worst = [], [], [], 0.0
            for _ in range(a.rounds):
                ms, first, pe = _idle_engine(eng, long[:n])
                e.append(ms), f.append(first)
                ms, pd = _idle_decoder(dec, long[:n])
                d.append(ms)
                worst = max(worst, rms(pe, pd))
            print(json.dumps({"measure": "idle", "frames": n, "rounds": a.rounds, "engine_ms": round(statistics.median(e), 3),
                              "engine_min_max_ms": [round(min(e), 3), round(max(e), 3)], "engine_first_chunk_ms": round(statistics.median(f), 3),
                              "decoder_ms": round(statistics.median(d), 3), "decoder_min_max_ms": [round(min(d), 3), round(max(d), 3)],
                              "pcm_rms_engine_vs_decoder": worst}), flush=True)
        # (b)
        seeds = [7000, 7001, 7002, 7003]
        _best_of(eng, prompt, seeds, 64, True), _best_of(eng, prompt, seeds, 64, False)   # warm-up: graphs of this width captured
        res = {"pcm": [], "codes": [], "pcm_calls": [], "codes_calls": []}
        worst = 0.0
        for _ in range(a.rounds):
            ms, calls, b1, p1 = _best_of(eng, prompt, seeds, 64, True)
            res["pcm"].append(ms), res["pcm_calls"].append(calls)
            ms, calls, b2, p2 = _best_of(eng, prompt, seeds, 64, False)
            res["codes"].append(ms), res["codes_calls"].append(calls)
            assert b1 == b2, "the two arms picked different winners"
            worst = max(worst, rms(p1, p2))
        med = {k: statistics.median(v) for k, v in res.items()}
        print(json.dumps({"measure": "best_of_4", "frames": 64, "rounds": a.rounds, "set_with_pcm_ms": round(med["pcm"], 3),
                          "set_with_pcm_codec_calls": med["pcm_calls"], "codes_only_then_decode_ms": round(med["codes"], 3),
                          "codes_only_then_decode_codec_calls": med["codes_calls"], "pcm_rms_between_arms": worst}), flush=True)
        # (c)
        eng.set_logprobs(False)
        want = [_idle_engine(eng, c)[2] for c in given]
        for nb in [int(b) for b in a.running.split(",")]:
            _loaded(eng, background[:nb], given)                            # warm-up
            med_ms, last_ms, share, worst = [], [], [], 0.0
            for _ in range(a.rounds):
                ms, chunks, shared, pcm = _loaded(eng, background[:nb], given)
                med_ms.append(statistics.median(ms)), last_ms.append(max(ms)), share.append(shared / max(chunks, 1))
                worst = max(worst, max(rms(p, w) for p, w in zip(pcm, want)))
            print(json.dumps({"measure": "loaded", "running_slots": nb, "decode_requests": 8, "frames": 64, "rounds": a.rounds,
                              "decode_width": eng.decode_width(), "median_done_ms": round(statistics.median(med_ms), 3),
                              "last_done_ms": round(statistics.median(last_ms), 3), "chunks_shared_share": round(statistics.median(share), 3),
                              "pcm_rms_vs_idle": worst}), flush=True)
    finally:
        dec.close()
        eng.close()


if __name__ == "__main__":
    main()
