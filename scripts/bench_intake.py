"""Cost of [EXT] reference audio intake (q3tts_intake): one 10 s 44.1 kHz stereo s16 clip, and a batch of 32 such clips, from the call to
the floats on the host -- upload of the raw bytes, one launch of k_intake, download -- best of --rounds after one warm-up call (which builds
and uploads the ratio's table).  Against the host conversion it stands in for: the same decode and channel-0 downmix in numpy and
scipy.signal.resample_poly with the same taps (window = h / L), float32 in and out, one clip after the other.  Also the mean downmix, and the
largest deviation of the device result from the scipy one.  Writes profiles/intake_cost.md.  Nothing here is a pass / fail number.
Usage: python scripts/bench_intake.py [--rounds 5] [--out profiles/intake_cost.md]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
RATE, SECONDS, BATCH = 44100, 10, 32


def best_ms(fn, rounds):
    fn()   # warm-up
    best = float("inf")
    for _ in range(rounds):
        t0 = time.perf_counter()
        fn()
        best = min(best, (time.perf_counter() - t0) * 1e3)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "intake_cost.md"))
    a = ap.parse_args()
    import q3tts as Q
    import intake_ref as R
    from scipy import signal
    if Q.device_count() < 1:
        raise SystemExit("bench_intake.py needs a HIP device")
    rng = np.random.default_rng(1)
    n = RATE * SECONDS
    t = np.arange(n) / RATE
    clips = []
    for i in range(BATCH):   # speech-like level: two tones and noise per channel, different per clip
        lr = np.stack([0.3 * np.sin(2 * np.pi * (110 + 7 * i) * t) + 0.05 * rng.standard_normal(n), 0.3 * np.sin(2 * np.pi * (220 + 5 * i) * t) + 0.05 * rng.standard_normal(n)], 1)
        clips.append(np.ascontiguousarray(R.encode(lr, R.S16)).view(np.int16))
    L, M, N, taps = Q.intake_plan(RATE)
    h = Q.intake_filter(RATE)
    win = h.astype(np.float32) / np.float32(L)

    def device(k, mix):
        return Q.intake([(c, RATE, 2, Q.INTAKE_S16, mix) for c in clips[:k]])

    def host(k):
        out = []
        for c in clips[:k]:
            x = (c.reshape(-1, 2)[:, 0].astype(np.float32) / np.float32(32768.0))
            out.append(signal.resample_poly(x, L, M, window=win))
        return out

    rows = []
    for k in (1, BATCH):
        rows.append((k, best_ms(lambda: device(k, Q.INTAKE_FIRST), a.rounds), best_ms(lambda: device(k, Q.INTAKE_MEAN), a.rounds), best_ms(lambda: host(k), a.rounds)))
    dev, ref = device(BATCH, Q.INTAKE_FIRST), host(BATCH)
    assert all(d.size == r.size == R.n_out(RATE, n) for d, r in zip(dev, ref))
    dev_err = max(float(np.abs(d.astype(np.float64) - r.astype(np.float64)).max()) for d, r in zip(dev, ref))
    # the definition's figures (tests/test_intake_ref_cpu.py asserts them): the 1 kHz tone per rate and the 18 kHz tone in a 48 kHz clip
    tone = []
    for rate in R.RATES:
        m = rate * 50 // 1000
        y, _ = R.resample(np.sin(2 * np.pi * 1000.0 * np.arange(m) / rate).astype(np.float32), rate)
        tone.append((rate, float(np.abs(y - np.sin(2 * np.pi * 1000.0 * np.arange(y.size) / 24000.0))[240:-240].max())))
    y, _ = R.resample(np.sin(2 * np.pi * 18000.0 * np.arange(4800) / 48000.0).astype(np.float32), 48000)
    alias_db = float(-20 * np.log10(np.abs(y)[240:-240].max()))
    in_mb, out_mb = n * 4 / 1e6, R.n_out(RATE, n) * 4 / 1e6
    lines = [
        "# Reference audio intake: what the on-device conversion costs", "",
        "`scripts/bench_intake.py --rounds %d` on one MI355X.  A clip is %d s of %d Hz stereo s16 (%.2f MB of raw samples in, %d floats = %.2f MB out;"
        % (a.rounds, SECONDS, RATE, in_mb, R.n_out(RATE, n), out_mb),
        "ratio %d / %d, %d taps, %d terms per output, tile %d).  Time is from the `q3tts.intake` call to the floats on the host: synchronous upload,"
        % (L, M, N, taps, Q.intake_tile(RATE)),
        "one launch of `k_intake`, synchronous download, from pageable memory both ways.  Best of %d after one warm-up call.  The host arm is numpy's"
        % a.rounds,
        "decode of channel 0 and `scipy.signal.resample_poly(x, %d, %d, window=h / %d)` in float32 with the library's own taps, one clip after the other,"
        % (L, M, L),
        "on the same machine's CPU.  Nobody had measured this kernel before, the issue sets no time target, and nothing here is a pass / fail number.", "",
        "| clips per call | device, channel 0 (ms) | device, mean (ms) | scipy on the host (ms) |", "|---|---|---|---|"]
    for k, d0, d1, hs in rows:
        lines.append("| %d | %.2f | %.2f | %.2f |" % (k, d0, d1, hs))
    lines += ["", "Largest deviation of the device's samples from scipy's float32 ones over the %d clips: %.3g (signal peak about 0.5)." % (BATCH, dev_err), "",
              "## The definition's own figures", "",
              "From `tests/intake_ref.py` (float64 over the f32 table), asserted by `tests/test_intake_ref_cpu.py`.  A 1 kHz tone at each rate against",
              "the analytic 24 kHz tone, 50 ms, 10 ms in from both ends (cap 1e-4):", "",
              "| rate | " + " | ".join(str(r) for r, _ in tone) + " |", "|---|" + "---|" * len(tone),
              "| max error | " + " | ".join("%.2g" % e for _, e in tone) + " |", "",
              "An 18 kHz tone in a 48 kHz clip, which would alias to 6 kHz: attenuated by %.1f dB (the test asserts this value less 6 dB)." % alias_db, ""]
    open(a.out, "w").write("\n".join(lines))
    print("\n".join(lines))


if __name__ == "__main__":
    main()
