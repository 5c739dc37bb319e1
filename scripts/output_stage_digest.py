#!/usr/bin/env python3
"""One SHA-1 per case over every byte the three output-stage test entry points return: outputs with their guards, traces with their guards,
the counts and the history stores.  The cases go through op_pcm_convert, op_tsm and op_pitch alone, on the signals of tests/tsm_ref.py, so the
script runs unchanged against any build that has those entry points: a refactor of the stages is judged by running it against the build
before and the build after.  At most 9 frames a case, one process, a few seconds.

  python scripts/output_stage_digest.py [--lib PATH/libq3tts.so] [--out FILE.json] [--volume-out FILE.json]

tests/golden/output_stage_digests.json holds what one build printed; tests/test_gpu_output_stage_bits.py asserts it of the current one.
volume_cases() does the same for op_volume, recorded apart (tests/golden/output_stage_volume_digests.json) by a later build."""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FRAME, F32, S16 = 1920, 0, 1
STREAMED = (1, 4, 3, 1)


def signals():
    import tsm_ref as R
    return np.stack([R.speech_like(9, 21), R.noise(9, 22), R.periodic(75, 9, 23)[1]])   # sched_signals() of tests/test_gpu_tsm.py


def sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        a = np.ascontiguousarray(a)
        h.update(("%s%s;" % (a.dtype.str, a.shape)).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def store(q, n_streams, width, seed):
    """a guarded state store whose every slot holds somebody's history"""
    core = np.random.default_rng(seed).uniform(-1, 1, n_streams * width).astype(np.float32)
    g = np.full(q.GLUE_GUARD, -3e38, np.float32)
    return np.concatenate([g, core, g])


def permuted(sched):
    """three streams on slots 3, 0, 4 of a 5-slot store; position 1 starts a new utterance at the third chunk"""
    slots = np.tile(np.array([3, 0, 4], np.int32), (len(sched), 1))
    reset = np.zeros((len(sched), 3), np.int32)
    reset[2, 1] = 1
    return slots, reset


def cases(q):
    """yields (name, digest); every case is one call of one entry point"""
    x = signals()
    ident = lambda sched: np.tile(np.arange(3, dtype=np.int32), (len(sched), 1))
    chunks = lambda sched: [f * FRAME for f in sched]

    def tsm(name, sched, rates, encs, flush, **kw):
        outs, traces, wholes, twholes, n_out, hist = q.op_tsm(x, chunks(sched), kw.pop("slots", ident(sched)), kw.pop("n_streams", 3), rates, encs,
                                                               flush=flush, slack=8, **kw)
        return name, sha(*wholes, *twholes, n_out, hist)

    def pitch(name, sched, pairs, encs, flush, **kw):
        r = q.op_pitch(x, chunks(sched), kw.pop("slots", ident(sched)), kw.pop("n_streams", 3), [p[0] for p in pairs], [p[1] for p in pairs], encs,
                       flush=flush, slack=8, **kw)
        return name, sha(*r[2], *r[3], r[4], r[5], r[6])

    for sched in ((9,), STREAMED):
        for flush in (False, True):
            yield tsm("tsm/%s/%s" % ("-".join(map(str, sched)), "flushed" if flush else "streaming"), sched, [50, 125, 200], [F32, S16, F32], flush)
    yield tsm("tsm/with-native", STREAMED, [100, 75, 160], [S16, S16, F32], True)
    slots, reset = permuted(STREAMED)
    yield tsm("tsm/permuted-reset", STREAMED, [80, 150, 50], [S16, F32, F32], True, slots=slots, n_streams=5, reset_before=reset,
              hist=store(q, 5, q.TSM_HIST, 31))

    groups = (((100, 50), (100, 80), (100, 107)), ((100, 199), (100, 200), (125, 80)), ((80, 125), (100, 107), (100, 199)))
    for i, (pairs, encs) in enumerate(zip(groups, ([F32, S16, F32], [S16, F32, S16], [S16, F32, F32]))):
        for flush in (False, True):
            yield pitch("pitch/group%d/%s" % (i, "flushed" if flush else "streaming"), STREAMED, pairs, encs, flush)
    yield pitch("pitch/pitched-rated-native", STREAMED, ((100, 80), (125, 100), (100, 100)), [S16, S16, F32], True)
    yield pitch("pitch/permuted-reset", STREAMED, ((125, 80), (100, 107), (160, 100)), [F32, S16, F32], True, slots=slots, n_streams=5,
                reset_before=reset, hist=store(q, 5, q.TSM_HIST, 32), zhist=store(q, 5, q.PITCH_HIST, 33))

    def convert(name, sched, fmts, **kw):
        G = len(fmts)
        xs = x[np.arange(G) % 3]
        sl = kw.pop("slots", np.tile(np.arange(G, dtype=np.int32), (len(sched), 1)))
        outs, wholes, n_out, hist = q.op_pcm_convert(xs[:, : sum(sched) * FRAME], chunks(sched), sl, kw.pop("n_streams", G), fmts, slack=8, **kw)
        return name, sha(*wholes, n_out, hist)

    yield convert("pcm/every-format", (1, 2, 1), [(r, e) for r in q.PCM_RATES for e in (F32, S16) if q.pcm_format_ok(r, e)])
    slots3, reset3 = permuted((1, 2, 1))
    yield convert("pcm/permuted-reset", (1, 2, 1), [(22050, S16), (8000, F32), (48000, S16)], slots=slots3, n_streams=5, reset_before=reset3,
                  hist=store(q, 5, 2 * q.PCM_HIST, 34))


def volume_cases(q):
    """the same for op_volume, traces on: tests/golden/output_stage_volume_digests.json"""
    x = signals()

    def volume(name, sched, vols, **kw):
        slots = kw.pop("slots", np.tile(np.arange(3, dtype=np.int32), (len(sched), 1)))
        outs, traces, wholes, twholes, n_out, hist = q.op_volume(x, [f * FRAME for f in sched], slots, kw.pop("n_streams", 3), vols, trace=True,
                                                                 slack=8, **kw)
        return name, sha(*wholes, *twholes, n_out, hist)

    for sched in ((9,), STREAMED):
        yield volume("volume/%s" % "-".join(map(str, sched)), sched, [120, -60, 200])
    yield volume("volume/with-unity", STREAMED, [0, 200, 0])
    slots, reset = permuted(STREAMED)
    yield volume("volume/permuted-reset", STREAMED, [120, -60, 200], slots=slots, n_streams=5, reset_before=reset, hist=store(q, 5, q.VOL_HIST, 35))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", help="another build's libq3tts.so to run the cases against")
    ap.add_argument("--out", help="also write the digests to this JSON file")
    ap.add_argument("--volume-out", help="also write the op_volume digests to this JSON file")
    a = ap.parse_args()
    import q3tts as q
    if a.lib:
        q.LIB_PATH = os.path.abspath(a.lib)
    for gen, path in ((cases, a.out), (volume_cases, a.volume_out)):
        got = {}
        for name, d in gen(q):
            print("%s  %s" % (d, name), flush=True)
            got[name] = d
        if path:
            with open(path, "w") as f:
                json.dump(got, f, indent=1, sort_keys=True)
                f.write("\n")


if __name__ == "__main__":
    main()
