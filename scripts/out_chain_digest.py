#!/usr/bin/env python3
"""One SHA-1 per case over what requests are given when their PCM passes through the codec's output stages inside the engine: every request's
codes, its delivered bytes, its delivered sample count and its loudness rows.  scripts/output_stage_digest.py drives the stage launchers
through their test entry points; this one drives what sits between CodecDecoder and the launchers -- which stage runs, what it is handed,
the lazy making of the stages, their reset when a stream is taken again, the flush, the converter history of a primed stream -- so a refactor
of that layer is judged by running the script against the build before and the build after.

Tiny synthetic model, Q8_0, 4-slot engines with their codec, temperature 0, at most 6 frames a request, the scheduler stepped by hand.  One
process, a few seconds a case.

  python scripts/out_chain_digest.py [--lib PATH/libq3tts.so] [--out FILE.json]

The stage counters are printed beside each digest and are not hashed.  tests/golden/out_chain_digests.json holds what one build printed;
tests/test_gpu_out_chain_bits.py asserts it of the current one."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32, S16 = 0, 1
WAIT_MS = 120000.0


def model():
    import synth_models
    return synth_models.ensure(synth_models.model_dir("smoke_tiny"), [["--preset", "tiny", "--quant", "q8_0"]])


def speaker():
    with open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")) as f:
        return np.array(json.load(f)["spk_emb"], np.float32)


def settle(eng, done, limit=4000):
    for _ in range(limit):
        if done():
            return
        eng.sched_step()
    raise AssertionError("the scheduler did not get there")


def drain(eng, limit=4000):
    for _ in range(limit):
        if not eng.sched_step():
            return
    raise AssertionError("the scheduler did not go idle")


class Wave:
    """requests submitted side by side, each with its own output settings; collect() steps until all have ended and hashes them in order"""

    def __init__(self, q, eng, sha):
        self.q, self.eng, self.sha, self.rids = q, eng, sha, []

    def settings(self, fmt=None, rate=100, pitch=100, vol=0, loud=False):
        e = self.eng
        e.set_output_format(*(fmt or (None,)))
        e.set_speech_rate(rate); e.set_pitch(pitch); e.set_volume(vol); e.set_loudness(loud)

    def add(self, submit, **kw):
        self.settings(**kw)
        rid = submit()
        self.settings()
        assert self.eng.request_metered(rid) == bool(kw.get("loud"))
        self.rids.append((rid, bool(kw.get("loud"))))
        return rid

    def collect(self):
        e = self.eng
        ended = (self.q.REQ_DONE, self.q.REQ_CANCELLED, self.q.REQ_FAILED)
        settle(e, lambda: all(e.poll(r)["state"] in ended for r, _ in self.rids))
        for rid, loud in self.rids:
            rows = e.fetch_loudness(rid) if loud else np.zeros((0, 2))
            r = e.result(rid, want_pcm=True)
            assert r["state"] == self.q.REQ_DONE, r["state"]
            pcm = np.ascontiguousarray(r["pcm"])
            assert pcm.size == r["n_pcm"]
            for a in (np.ascontiguousarray(r["codes"]), pcm, np.array([r["n_pcm"]], np.int64), np.ascontiguousarray(rows, np.float64)):
                self.sha.update(("%s%s;" % (a.dtype.str, a.shape)).encode())
                self.sha.update(a.tobytes())
        self.rids = []
        drain(e)


def stats(eng):
    return dict(pcm_out=eng.pcm_out_stats(), tsm=eng.tsm_stats(), pitch=eng.pitch_stats(), volume=eng.volume_stats(), loudness=eng.loudness_stats())


def cases(q, model_dir):
    """yields (name, digest, the engine's stage counters behind the case)"""
    spk = speaker()
    rng = np.random.default_rng(11)
    texts = [rng.integers(0, 4000, n).astype(np.int32) for n in (8, 9, 7, 10, 6, 11)]
    given = rng.integers(0, 2048, (6, 16)).astype(np.int32)
    pre_codes, ref_codes, ref_text = (rng.integers(0, 2048, (6, 16)).astype(np.int32), rng.integers(0, 2048, (70, 16)).astype(np.int32),
                                      rng.integers(0, 4000, 5).astype(np.int32))
    engine = lambda: q.Engine(model_dir, "q8_0", max_batch=4, max_prompt=256, max_steps=24, load_codec=True)

    def gen(eng, i, n):   # one greedy request of exactly n frames
        prompt = eng.assets.build_core(texts[i % len(texts)], lang_id=2055, spk_emb=spk)
        return lambda: eng.submit(prompt, max_steps=n, temperature=0.0, seed=40 + i, mask_eos=True, want_pcm=True)

    eng = engine()
    try:
        sha = hashlib.sha1(); w = Wave(q, eng, sha)
        w.add(gen(eng, 0, 6), fmt=(16000, S16), vol=60, loud=True)
        w.add(gen(eng, 1, 5), rate=125, vol=-60)
        w.add(gen(eng, 2, 6), fmt=(24000, S16), pitch=80, loud=True)
        w.add(gen(eng, 3, 6))
        w.collect()
        yield "mixed-wave", sha.hexdigest(), stats(eng)

        sha = hashlib.sha1(); w = Wave(q, eng, sha)
        for i, n in enumerate((6, 5, 4, 6)):
            w.add(gen(eng, i, n))
        w.collect()
        yield "native-wave", sha.hexdigest(), stats(eng)

        sha = hashlib.sha1(); w = Wave(q, eng, sha)
        waves = ((dict(pitch=80), dict(rate=50)),
                 (dict(loud=True), dict(fmt=(48000, S16))),
                 (dict(fmt=(24000, S16), rate=200, vol=200), dict(pitch=200)))
        for k, wave in enumerate(waves):
            for i, kw in enumerate(wave):
                w.add(gen(eng, 2 * k + i, 6 - i), **kw)
            w.collect()
        yield "slot-reuse", sha.hexdigest(), stats(eng)

        sha = hashlib.sha1(); w = Wave(q, eng, sha)
        w.add(lambda: eng.submit_decode(given), rate=80)
        w.collect()
        yield "decode-given", sha.hexdigest(), stats(eng)
    finally:
        eng.close()

    eng = engine()
    try:
        sha = hashlib.sha1(); w = Wave(q, eng, sha)
        for i, kw in enumerate((dict(vol=60, loud=True), dict(fmt=(16000, S16)), dict(pitch=80), dict(rate=125))):
            w.add(gen(eng, i, 6 - i % 2), **kw)
            w.collect()
        yield "lazy-order", sha.hexdigest(), stats(eng)
    finally:
        eng.close()

    eng = engine()
    try:
        sha = hashlib.sha1(); w = Wave(q, eng, sha)
        vid = eng.register_voice(spk, ref_codes, ref_text)
        pid = eng.preamble_create(pre_codes)
        assert eng.preamble_wait(pid, WAIT_MS) and eng.preamble_poll(pid) == (q.PREAMBLE_READY, 6)
        eng.voice_set_preamble(vid, pid)
        rid = w.add(lambda: eng.submit_text(vid, texts[0], max_steps=6, temperature=0.0, seed=50, mask_eos=True, want_pcm=True), fmt=(22050, S16))
        assert eng.request_preamble(rid) == pid
        w.collect()
        yield "preamble-converted", sha.hexdigest(), stats(eng)
    finally:
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build's libq3tts.so to run the cases against")
    ap.add_argument("--out", help="also write the digests to this JSON file")
    a = ap.parse_args()
    import q3tts as q
    if a.lib:
        q.LIB_PATH = os.path.abspath(a.lib)
    got = {}
    for name, d, st in cases(q, model()):
        print("%s  %s  %s" % (d, name, json.dumps(st, sort_keys=True)), flush=True)
        got[name] = d
    if a.out:
        with open(a.out, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")


if __name__ == "__main__":
    main()
