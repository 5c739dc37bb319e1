"""Inputs of the mel tests (tests/test_mel_ref_cpu.py, tests/test_gpu_mel.py): every case has a fixed seed and at most 24000 samples.

Lengths: 0, 1, 2, 255 give no frame; 256, 257 one; 383, 384, 385 straddle `i < n` in the left pad and the saturating index of the right
pad; 511, 512, 513 go from one frame to two; 639, 640, 641 have every pad sample inside the clip; 24000 is a second of audio (93 frames).
White noise runs at every length, every other signal at three or more.

Amplitudes.  The reference's own bound (mel_ref.py) must place at most 1 % of a case's outputs in the straddle class.  Two signals are
leakage-free once a frame lies wholly inside the clip, and there the 4u sum |xs| term of the bin bound alone decides the class of every empty
bin: the 0.5 tone on bin 100 leaves 4 of 128 outputs per inner frame straddling (the filters next to the main lobe), and DC 1.0 leaves 127 of
128.  So those two keep their amplitude at the three short lengths, where the pads break the periodicity and every output is far above the
floor, and run again at 0.25 (tone, 24000 samples) and 1 / 32 (DC, 384 and 639 samples), where the empty bins sit in the floor class.
faint_noise (sigma 2e-5) puts the magnitudes near 4e-4, where the 1e-9 under the root is 1 % of the output and yet above the floor."""
import numpy as np

LENGTHS = (0, 1, 2, 255, 256, 257, 383, 384, 385, 511, 512, 513, 639, 640, 641, 24000)
BIN_HZ = 24000.0 / 1024.0


def _noise(n, seed, sigma):
    return (sigma * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def _tone(n, bins, amp=0.5):
    return (amp * np.sin(2 * np.pi * bins * BIN_HZ * np.arange(n) / 24000.0 + 0.3)).astype(np.float32)


def _impulse(n, at):
    a = np.zeros(n, np.float32)
    a[at] = 1.0
    return a


def _square(n):
    return np.where((np.arange(n) // 37) % 2 == 0, 1.0, -1.0).astype(np.float32)   # half period 37 samples: 324 Hz and odd harmonics


def _burst(n, seed):
    a = np.zeros(n, np.float32)
    a[n - 300:] = _noise(300, seed, 0.1)
    return a


def _build():
    c = []
    for i, n in enumerate(LENGTHS):
        c.append(("noise_%d" % n, _noise(n, 100 + i, 0.1)))
    for n in (257, 512, 641):
        c.append(("tone_bin100_%d" % n, _tone(n, 100.0)))
    c.append(("tone_bin100_quarter_24000", _tone(24000, 100.0, 0.25)))
    for n in (256, 513, 640):
        c.append(("tone_bin100p5_%d" % n, _tone(n, 100.5)))
    for n in (256, 385, 640):
        for tag, at in (("0", 0), ("1", 1), ("nm2", n - 2), ("nm1", n - 1), ("mid", n // 2)):
            c.append(("impulse_%s_%d" % (tag, n), _impulse(n, at)))
    for n in (2, 256, 257):
        c.append(("dc_%d" % n, np.ones(n, np.float32)))
    for n in (384, 639):
        c.append(("dc_32nd_%d" % n, np.full(n, 1.0 / 32.0, np.float32)))
    for n in (383, 512, 640):
        c.append(("square_%d" % n, _square(n)))
    for i, n in enumerate((257, 511, 641)):
        c.append(("tiny_noise_%d" % n, _noise(n, 200 + i, 1e-6)))
    c.append(("faint_noise_512", _noise(512, 210, 2e-5)))
    for n in (1, 255, 256, 640):
        c.append(("silence_%d" % n, np.zeros(n, np.float32)))
    for i, n in enumerate((513, 640, 24000)):
        c.append(("burst_%d" % n, _burst(n, 300 + i)))
    return c


CASES = _build()
NAMES = [n for n, _ in CASES]
AUDIO = dict(CASES)
