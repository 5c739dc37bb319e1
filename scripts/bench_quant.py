"""Cost of the seven quantised weight formats on the full-size synthetic model: q8_0, q5_k_m, q4_k_m, q3_k_m, iq4_xs, q4_0, q5_0 (or the --quants chosen), codes only (no codec), one GPU, one process.
The quantisations are interleaved and each is run `--rounds` times (default 2), so the spread between two runs of one quantisation stands next
to the differences between quantisations.  Per run:
  single    one utterance, greedy, EOS masked, `--frames` frames after a warm-up utterance: ms per frame (host clock around generate_batch, which
            ends in a device synchronise)
  batch     64 slots, 64 utterances of `--frames` frames after a warm-up batch: audio-seconds per second (a frame is 80 ms of audio)
  weight_bytes   the talker's packed layer matrices as the engine holds them, mean per layer (the Q6_K share differs between layers)
Prints one JSON line per run and writes the table to profiles/q5_0_cost.md (--out), which holds nothing else: the comparison with the parent
commit is kept in profiles/q5_0_parent_ab.md.  (profiles/q4_k_m_cost.md, profiles/q3_k_m_cost.md, profiles/iq4_xs_cost.md and profiles/q4_0_cost.md are this
script's tables from before it had the q3_k_m, the iq4_xs, the q4_0 and the q5_0 arm.)
Usage: python scripts/bench_quant.py [--model-dir DIR] [--rounds 2] [--frames 64] [--quants q8_0,q4_k_m,...] [--out profiles/q5_0_cost.md]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
ALL_QUANTS = ["q8_0", "q5_k_m", "q4_k_m", "q3_k_m", "iq4_xs", "q4_0", "q5_0"]
NAMES = {"iq4_xs": "IQ4_XS", "q4_0": "Q4_0", "q5_0": "Q5_0"}


def _leg(Q, model, quant, batch, frames, spk, n_layer):
    eng = Q.Engine(model, quant, max_batch=batch, max_steps=frames + 8, load_codec=False)
    try:
        rng = np.random.default_rng(3)
        prompts = [eng.assets.build_core(rng.integers(0, 4000, 12 + i % 7).astype(np.int32), lang_id=2055, spk_emb=spk) for i in range(batch)]
        eng.generate_batch(prompts, max_steps=8, temperature=0.0, mask_eos=True)   # warm-up: code objects loaded, graphs of this width captured
        t0 = time.perf_counter()
        res = eng.generate_batch(prompts, max_steps=frames, temperature=0.0, mask_eos=True)
        dt = time.perf_counter() - t0
        assert all(r["codes"].shape[0] == frames for r in res)
        return dt, eng.stats()["talker_weight_bytes"] / n_layer
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model-dir", default=os.environ.get("Q3_BENCH_MODEL"))
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--quants", default=",".join(ALL_QUANTS), help="the arms, in the order they are interleaved")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "q5_0_cost.md"))
    a = ap.parse_args()
    QUANTS = a.quants.split(",")
    assert "q8_0" in QUANTS and all(q in ALL_QUANTS for q in QUANTS), "--quants: q8_0 and any of " + " ".join(ALL_QUANTS)
    import q3tts as Q
    import synth_models
    if Q.device_count() < 1:
        raise SystemExit("bench_quant.py needs a HIP device")
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    import ggml_ref
    models = {q: synth_models.full(q, a.model_dir) for q in QUANTS}
    nl = ggml_ref.read_gguf(os.path.join(models["q8_0"], "gguf_q8_0", "qwen3_tts_talker.gguf"))[0]["qwen3-tts-talker.block_count"]   # one architecture, every encoding
    n_layer = {q: nl for q in QUANTS}
    runs = {q: [] for q in QUANTS}
    for rnd in range(a.rounds):
        for q in QUANTS:   # interleaved: q8_0, q5_k_m, ..., q5_0, q8_0, ...
            t1, wb = _leg(Q, models[q], q, 1, a.frames, spk, n_layer[q])
            t64, _ = _leg(Q, models[q], q, 64, a.frames, spk, n_layer[q])
            row = dict(quant=q, round=rnd, ms_per_frame=round(t1 * 1e3 / a.frames, 4), audio_s_per_s_64=round(64 * a.frames * 0.08 / t64, 1),
                       weight_bytes_per_layer=int(wb))
            runs[q].append(row)
            print(json.dumps(row), flush=True)
    lines = ["# " + ", ".join(NAMES.get(q, q.upper()) for q in QUANTS) + " on the full-size synthetic model", "",
             "`python scripts/bench_quant.py --rounds %d --frames %d --quants %s`: one MI355X, one process, codes only, the quantisations interleaved." % (a.rounds, a.frames, a.quants),
             "Spread = largest minus smallest of a quantisation's own runs.", "",
             "| quant | ms / frame, 1 utterance (runs) | spread | audio-s / s, 64 slots (runs) | spread | talker weight bytes / layer |", "|---|---|---|---|---|---|"]
    for q in QUANTS:
        ms = [r["ms_per_frame"] for r in runs[q]]; au = [r["audio_s_per_s_64"] for r in runs[q]]
        lines.append("| %s | %s | %.4f | %s | %.1f | %d |" % (q, ", ".join("%.4f" % v for v in ms), max(ms) - min(ms), ", ".join("%.1f" % v for v in au),
                                                            max(au) - min(au), runs[q][0]["weight_bytes_per_layer"]))
    mean = lambda q, key: sum(r[key] for r in runs[q]) / len(runs[q])
    if "q4_k_m" in QUANTS and "q5_k_m" in QUANTS:
        m4, m5 = [r["ms_per_frame"] for r in runs["q4_k_m"]], [r["ms_per_frame"] for r in runs["q5_k_m"]]
        sp5 = max(m5) - min(m5)
        over = sum(m4) / len(m4) - sum(m5) / len(m5)
        lines += ["", "Expectation: q4_k_m's single-utterance ms / frame is not above q5_k_m's by more than the spread between the q5_k_m runs (%.4f ms)." % sp5,
                  "Measured: mean q4_k_m %.4f, mean q5_k_m %.4f: %s." % (sum(m4) / len(m4), sum(m5) / len(m5), "met" if over <= sp5 else "NOT met (q4_k_m is %.4f ms above)" % over)]
    for q, base in [(q, b) for q in ("q3_k_m", "iq4_xs", "q4_0", "q5_0") for b in ("q4_k_m", "iq4_xs", "q4_0", "q5_k_m") if q != b and q in QUANTS and b in QUANTS and (b == "q4_k_m" or q == "q4_0" and b == "iq4_xs" or q == "q5_0" and b != "iq4_xs")]:
        lines += ["", "No threshold was set for %s in advance.  Against %s: %.4f against %.4f ms / frame, %.1f against %.1f audio-s / s at 64 slots, %.1f against %.1f MB per talker layer."
                  % (q, base, mean(q, "ms_per_frame"), mean(base, "ms_per_frame"), mean(q, "audio_s_per_s_64"), mean(base, "audio_s_per_s_64"),
                     runs[q][0]["weight_bytes_per_layer"] / 1e6, runs[base][0]["weight_bytes_per_layer"] / 1e6)]
    lines.append("")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("\n".join(lines))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
