"""Cost of [EXT] output formats (q3tts_engine_set_output_format), full-size model, Q8_0, one 16-slot engine with its codec, the scheduler stepped
by this thread.  16 sampled requests with PCM run side by side for --frames frames, so every codec pass carries 16 streams; the arms -- native,
{16000, s16}, {48000, s16} -- are interleaved on the one engine, --rounds times after a warm-up of each.  One JSON line per arm: submit to
all DONE (median, min, max), the same per codec pass of 16 streams, the converter's chunk and sample counts, the bytes the PCM took across
to the host.  Then the host conversion the device one replaces: the same 16 native streams converted one after the other by a numpy polyphase
filter in f32 with the library's table (all taps of one output vectorised over the stream) and quantised, median ms per stream and for 16.
Usage: python scripts/bench_pcm_out.py [--model-dir DIR] [--rounds 2] [--frames 64]"""
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
ARMS = [("native", None), ("16000_s16", (16000, 1)), ("48000_s16", (48000, 1))]
N = 16


def _run(eng, prompts, frames, fmt):
    s0, c0 = eng.pcm_out_stats(), eng.stats()["codec_calls"]
    eng.set_output_format(*(fmt if fmt else (None,)))
    t0 = time.perf_counter()
    ids = [eng.submit(p, max_steps=frames, seed=100 + i, mask_eos=True, want_pcm=True, **SAMPLING) for i, p in enumerate(prompts)]
    eng.set_output_format(None)
    while not all(eng.poll(r)["state"] in ENDED for r in ids):
        assert time.perf_counter() - t0 < 300.0, "requests did not end"
        eng.sched_step()
    ms = (time.perf_counter() - t0) * 1e3
    out = [eng.result(r, want_pcm=True) for r in ids]
    s1 = eng.pcm_out_stats()
    return ms, out, s1["chunks_converted"] - s0["chunks_converted"], s1["samples_out"] - s0["samples_out"], eng.stats()["codec_calls"] - c0


def host_polyphase(x, L, M, h, s16):
    """what an integrator writes behind q3tts_fetch: f32 numpy, one vector operation per tap, clamp, round"""
    n = np.arange(x.size * L // M, dtype=np.int64)
    t = n * M
    p, j = t % L, t // L
    taps = -(-h.size // L)
    xp = np.concatenate([np.zeros(taps, np.float32), x])
    hp = np.concatenate([h, np.zeros(taps * L, np.float32)])
    y = np.zeros(n.size, np.float32)
    for k in range(taps):
        y += hp[p + k * L] * xp[j - k + taps]
    y = np.clip(y, -1.0, 1.0)
    return np.rint(y * np.float32(32767.0)).astype(np.int16) if s16 else y


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
    eng = Q.Engine(model, "q8_0", max_batch=N, max_prompt=512, max_steps=a.frames, load_codec=True)
    rng = np.random.default_rng(1)
    prompts = [eng.assets.build_core(rng.integers(0, 4000, 8 + i % 5).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(N)]
    try:
        native = None
        for _, fmt in ARMS:                                                  # warm-up: graphs captured, converter state allocated
            _run(eng, prompts, a.frames, fmt)
        res = {name: [] for name, _ in ARMS}
        for _ in range(a.rounds):
            for name, fmt in ARMS:
                ms, out, chunks, samples, calls = _run(eng, prompts, a.frames, fmt)
                res[name].append((ms, chunks, samples, calls, sum(o["pcm"].nbytes for o in out)))
                if fmt is None:
                    native = [o["pcm"] for o in out]
        passes = -(-a.frames // 4)
        for name, _ in ARMS:
            ms = [r[0] for r in res[name]]
            print(json.dumps({"measure": "engine", "arm": name, "streams": N, "frames": a.frames, "rounds": a.rounds,
                              "submit_to_done_ms": round(statistics.median(ms), 3), "min_max_ms": [round(min(ms), 3), round(max(ms), 3)],
                              "ms_per_pass_of_16": round(statistics.median(ms) / passes, 4), "codec_chunk_decodes": res[name][-1][3],
                              "chunks_converted": res[name][-1][1], "samples_out": res[name][-1][2], "pcm_bytes_to_host": res[name][-1][4]}), flush=True)
        for name, fmt in ARMS[1:]:
            L, M, _, _ = Q.pcm_out_plan(fmt[0])
            h = Q.pcm_out_filter(fmt[0])
            host_polyphase(native[0], L, M, h, True)
            per = []
            for _ in range(max(a.rounds, 2)):
                for x in native:
                    t0 = time.perf_counter()
                    host_polyphase(x, L, M, h, True)
                    per.append((time.perf_counter() - t0) * 1e3)
            print(json.dumps({"measure": "host_numpy_polyphase", "arm": name, "frames": a.frames, "ms_per_stream": round(statistics.median(per), 3),
                              "ms_for_16_streams": round(statistics.median(per) * N, 3), "ms_per_4_frame_chunk_of_16": round(statistics.median(per) * N / passes, 4)}),
                  flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
