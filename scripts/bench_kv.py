#!/usr/bin/env python3
"""F16 against Q8_0 talker KV cache on the full-size synthetic model with Q8_0 weights (q3tts_engine_create_kv): what the int8 pages cost
or save in time, and what they save in bytes.  One box, the two arms interleaved, each arm twice; no codec (the AR loop is what the KV
type touches).  Legs:
  one       ms per frame of one utterance, 1 slot, 128 frames
  b64       audio-s/s, 64 slots, bench.py's prompts (16 / 32 / 64 text ids), 128 frames each
  b256      the same at 256 slots
  long64    audio-s/s, 64 slots, prompts of about 1000 rows, 128 frames each
  bytes     KV bytes per token (q3tts_engine_stats) and bytes of the talker pool (pages x both plane pages, q3tts_kv_layout)
For information only: the share of identical code_0 over 64 greedy frames, and the RMS difference of the talker's logits after one
32-id prompt between the two types (q3tts_tf_open_kv).  --out FILE writes the table as markdown; --legs picks legs."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import q3tts as Q  # noqa: E402
import synth_models  # noqa: E402

FRAME_SEC = 1920 / 24000.0
TYPES = ("f16", "q8_0")
FRAMES = 128


def prompt(assets, spk, n_text, seed):
    return assets.build_core(np.random.default_rng(seed).integers(0, 4000, n_text).astype(np.int32), lang_id=2055, spk_emb=spk)


def pool_bytes(n_layer, n_kv, kv_type, slots, max_prompt, max_steps):
    pages = slots * ((max_prompt + max_steps + 1 + 63) // 64) + 1      # the engine's pool: whole pages per slot and the scratch page
    return pages * 2 * Q.kv_layout(n_layer, n_kv, kv_type)[1]


def leg(model_dir, spk, slots, n_texts, reps=2):
    """both arms alive, runs interleaved: [(elapsed s, frames)] per type, the engines' kv bytes per token, prompt rows"""
    eng = {t: Q.Engine(model_dir, "q8_0", max_batch=slots, max_prompt=1024, max_steps=FRAMES, load_codec=False, kv_type=t) for t in TYPES}
    out = {t: [] for t in TYPES}
    prompts = [prompt(eng["f16"].assets, spk, n_texts[i % len(n_texts)], 42 + i) for i in range(slots)]
    for t in TYPES:                                                    # warm-up: graphs captured, pages touched
        eng[t].generate_batch(prompts, max_steps=8, temperature=0.0, seed=42, mask_eos=True)
    for _ in range(reps):
        for t in TYPES:
            t0 = time.perf_counter()
            res = eng[t].generate_batch(prompts, max_steps=FRAMES, temperature=0.0, seed=42, mask_eos=True)
            out[t].append((time.perf_counter() - t0, sum(r["codes"].shape[0] for r in res)))
    bpt = {t: eng[t].stats()["kv_bytes_per_token"] for t in TYPES}
    for e in eng.values():
        e.close()
    return out, bpt, max(p.shape[0] for p in prompts)


def agreement(model_dir, spk):
    eng = {t: Q.Engine(model_dir, "q8_0", max_batch=1, max_steps=64, load_codec=False, kv_type=t) for t in TYPES}
    p = prompt(eng["f16"].assets, spk, 32, 42)
    c = {t: eng[t].generate_batch([p], max_steps=64, temperature=0.0, seed=42, mask_eos=True)[0]["codes"][:, 0] for t in TYPES}
    for e in eng.values():
        e.close()
    pos = np.stack([np.arange(p.shape[0])] * 3 + [np.zeros(p.shape[0], np.int64)], 1).astype(np.int32)
    lg = {}
    for t in TYPES:
        tf = Q.TfContext(os.path.join(model_dir, "gguf_q8_0", "qwen3_tts_talker.gguf"), n_ctx=4096, max_tok=64, kv_type=t)
        lg[t] = tf.eval(p, pos, 0, 2160)[1][-1].astype(np.float64)
        tf.close()
    return float((c["f16"] == c["q8_0"]).mean()), float(np.sqrt(np.mean((lg["f16"] - lg["q8_0"]) ** 2))), float(np.sqrt(np.mean(lg["f16"] ** 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL") or synth_models.model_dir("full"))
    ap.add_argument("--legs", default="one,b64,b256,long64,info")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    synth_models.full("q8_0", a.model_dir)
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    shapes = {"one": (1, (32,)), "b64": (64, (16, 32, 64)), "b256": (256, (16, 32, 64)), "long64": (64, (985,))}
    rows, res = [], {}
    for name in a.legs.split(","):
        if name not in shapes:
            continue
        slots, n_texts = shapes[name]
        out, bpt, prows = leg(a.model_dir, spk, slots, n_texts)
        res[name] = dict(runs={t: out[t] for t in TYPES}, kv_bytes_per_token=bpt, prompt_rows=prows)
        for t in TYPES:
            runs = out[t]
            if name == "one":
                vals, unit = [1e3 * s / f for s, f in runs], "ms per frame (wall, prefill included)"
            else:
                vals, unit = [f * FRAME_SEC / s for s, f in runs], "audio-s/s"
            pb = pool_bytes(28, 8, t, slots, 1024, FRAMES)
            rows.append("| %s | %s | %d | %d | %s | %s | %d | %.2f |" % (name, t, slots, prows, " / ".join("%.3f" % v for v in vals), unit, int(bpt[t]), pb / 2 ** 30))
            print(rows[-1], flush=True)
    info = ""
    if "info" in a.legs.split(","):
        share, rms, ref = agreement(a.model_dir, spk)
        info = ("For information only (seeded synthetic weights): greedy code_0 identical in %.1f %% of 64 frames; RMS difference of the talker's "
                "2160 logits after a 32-id prompt %.4g against an RMS of %.4g.\n" % (100 * share, rms, ref))
        print(info, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("| leg | KV type | slots | prompt rows (max) | run 1 / run 2 | unit | KV bytes per token | pool GiB |\n|---|---|---|---|---|---|---|---|\n")
            f.write("\n".join(rows) + "\n\n" + info)
        json.dump(res, open(a.out + ".json", "w"))


if __name__ == "__main__":
    main()
