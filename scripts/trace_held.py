"""One pass over everything a held object ([EXT] codec preambles, prompt stems) goes through, for comparing two commits: tiny synthetic model,
Q8_0, one 4-slot engine with its codec, fixed seeds, every request waited for through q3tts_wait.
  1  a preamble of 6 frames and the stem of a clone voice's prompt head are created and waited for
  2  the preamble is set at engine level, the stem on the voice
  3  two requests of the text form (they take the voice's stem; one sampled with PCM, one greedy without) and one raw-prompt request with
     PCM (primed with the engine-level preamble)
  4  a candidate set of two, sampled, with PCM (both primed)
  5  both creators release, both settings are unset: the preamble and the stem recycle, the scheduler frees the stem's store
  6  one more plain request with PCM
Prints one JSON line: the SHA-1 over every request's codes and PCM bytes in order, q3tts_engine_preamble_stats and q3tts_engine_stem_stats
after step 4 and at the end.  --settings: the requests with PCM also carry the per-request output settings, so that every output stage runs --
16000 Hz s16 with +6 dB (step 3, text form), rate 125 with -6 dB (step 3, raw prompt), pitch 80 s16 with +20 dB (step 4) and 24000 Hz s16 at rate
125 and pitch 80 with +6 dB (step 6).  Meant to run under a kernel trace, a fresh process per commit:
    rocprofv3 --kernel-trace --stats -- python scripts/trace_held.py
Usage: python scripts/trace_held.py [--settings]"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
WAIT_MS = 120000.0
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)


def main():
    import q3tts as Q
    settings = "--settings" in sys.argv[1:]
    import synth_models
    model = synth_models.ensure(synth_models.model_dir("smoke_tiny"), [["--preset", "tiny", "--quant", "q8_0"]])
    spk = np.array(json.load(open(os.path.join(ROOT, "tests", "golden", "speakers", "vivian.json")))["spk_emb"], np.float32)
    rng = np.random.default_rng(5)
    ref_codes, ref_text = rng.integers(0, 2048, (70, 16)).astype(np.int32), rng.integers(0, 4000, 5).astype(np.int32)
    texts = [rng.integers(0, 4000, n).astype(np.int32) for n in (7, 11)]
    pre_codes = rng.integers(0, 2048, (6, 16)).astype(np.int32)
    eng = Q.Engine(model, "q8_0", max_batch=4, max_prompt=256, max_steps=24, load_codec=True)
    sha = hashlib.sha1()

    def out(fmt=None, rate=100, pitch=100, vol=0):   # what requests submitted from now on deliver; nothing without --settings
        if settings:
            eng.set_output_format(*(fmt or (None,)))
            eng.set_speech_rate(rate)
            eng.set_pitch(pitch)
            eng.set_volume(vol)

    def collect(rids, want_pcm):
        for rid, pcm in zip(rids, want_pcm):
            assert eng.wait(rid, WAIT_MS), "a request did not end"
            r = eng.result(rid, want_pcm=pcm)
            assert r["state"] == Q.REQ_DONE
            sha.update(np.ascontiguousarray(r["codes"]).tobytes())
            if pcm:
                sha.update(np.ascontiguousarray(r["pcm"]).tobytes())

    try:
        prompts = [eng.assets.build_core(rng.integers(0, 4000, n).astype(np.int32), lang_id=2055, spk_emb=spk) for n in (9, 14, 6)]
        vid = eng.register_voice(spk, ref_codes, ref_text)
        pid, sid = eng.preamble_create(pre_codes), eng.voice_stem_create(vid)                                    # 1
        assert eng.preamble_wait(pid, WAIT_MS) and eng.preamble_poll(pid) == (Q.PREAMBLE_READY, 6)
        assert eng.stem_wait(sid, WAIT_MS) and eng.stem_poll(sid)[0] == Q.STEM_READY
        n_stem = eng.stem_poll(sid)[1]
        eng.set_preamble(pid)                                                                                     # 2
        eng.voice_set_stem(vid, sid)
        out((16000, Q.PCM_S16), vol=60)
        rids = [eng.submit_text(vid, texts[0], max_steps=9, seed=3, mask_eos=True, want_pcm=True, **SAMPLED),     # 3
                eng.submit_text(vid, texts[1], max_steps=7, seed=4, mask_eos=True)]
        out(rate=125, vol=-60)
        rids.append(eng.submit(prompts[0], max_steps=10, seed=5, mask_eos=True, want_pcm=True))
        assert [eng.request_stem(r) for r in rids] == [(sid, n_stem), (sid, n_stem), (-1, 0)]
        assert [eng.request_preamble(r) for r in rids] == [-1, -1, pid]
        collect(rids, (True, False, True))
        out((24000, Q.PCM_S16), pitch=80, vol=200)
        rids = eng.submit_candidates(prompts[1], [901, 902], max_steps=8, mask_eos=True, want_pcm=True, **SAMPLED)  # 4
        assert [eng.request_preamble(r) for r in rids] == [pid, pid]
        collect(rids, (True, True))
        mid = dict(preamble=eng.preamble_stats(), stem=eng.stem_stats())
        eng.preamble_release(pid)                                                                                 # 5
        eng.stem_release(sid)
        assert eng.preamble_poll(pid)[0] == Q.PREAMBLE_READY and eng.stem_poll(sid)[0] == Q.STEM_READY           # the settings still hold them
        eng.set_preamble(None)
        eng.voice_set_stem(vid, None)
        for poll, gone in ((eng.preamble_poll, pid), (eng.stem_poll, sid)):
            try:
                poll(gone)
                raise AssertionError("a recycled object still answers")
            except Q.Q3Error:
                pass
        eng.sched_step()                                                                                          # the scheduler frees the store
        out((24000, Q.PCM_S16), rate=125, pitch=80, vol=60)
        rid = eng.submit(prompts[2], max_steps=8, seed=6, mask_eos=True, want_pcm=True)                           # 6
        assert eng.request_preamble(rid) == -1 and eng.request_stem(rid) == (-1, 0)
        collect([rid], (True,))
        end = dict(preamble=eng.preamble_stats(), stem=eng.stem_stats())
        assert end["stem"]["device_bytes"] == 0, end
        print(json.dumps({"sha1": sha.hexdigest(), "stem_rows": n_stem, "after_step_4": mid, "at_the_end": end}), flush=True)
    finally:
        eng.close()


if __name__ == "__main__":
    main()
