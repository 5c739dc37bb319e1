"""The float64 restatement of the whole codec decoder (tests/codec_f64_ref.py) and the C oracle pinned to each other at the float32 noise
floor, frame by frame; what the standing whole-signal bar (RMS < 1e-4) lets through and the per-frame bounds of
test_gpu_codec_pcm_f64.py do not; and the priming rule of the reference.  Tiny codec, no GPU."""
import os
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import codec_f64_ref as R

SPF = R.SPF
FRAME_RMS_BAR = 5e-7      # about 4 x the largest per-frame RMS measured (1.22e-7, 24 frames, seed 7)
SAMPLE_BAR = 3e-6         # about 5 x the largest per-sample error measured (5.36e-7)
PCM_RMS_TOL = 1e-4        # the standing whole-signal bar of the GPU tests


@pytest.fixture(scope="module")
def path(tiny_model):
    return os.path.join(tiny_model, "onnx", "q3tts_codec.gguf")


@pytest.fixture(scope="module")
def floor(path, oracle):
    """seed -> (codes, oracle PCM, float64 PCM), 24 frames each; computed once and left unchanged"""
    c = oracle.Codec(path)
    out = {}
    for seed in (7, 8):
        codes = np.random.default_rng(seed).integers(0, 2048, (24, 16))
        c.reset()
        t0 = time.time(); orc = c.decode(codes).copy(); t1 = time.time()
        ref = R.torch_codec(path, codes, torch.float64); t2 = time.time()
        print("seed %d: oracle %.2f s, float64 torch %.2f s" % (seed, t1 - t0, t2 - t1))
        assert ref.dtype == np.float64 and orc.dtype == np.float32 and ref.shape == orc.shape == (24 * SPF,)
        for a in (codes, orc, ref):
            a.setflags(write=False)
        out[seed] = (codes, orc, ref)
    c.close()
    return out


@pytest.mark.parametrize("seed", (7, 8))
def test_oracle_against_float64_per_frame(floor, seed):
    codes, orc, ref = floor[seed]
    E, M = R.frame_errors(orc, ref)
    assert E.shape == M.shape == (24,)
    whole = float(np.sqrt(np.mean((orc - ref) ** 2)))
    print("seed %d: whole rms %.3g, per-frame rms %.3g .. %.3g, max abs %.3g, signal rms %.3g"
          % (seed, whole, E.min(), E.max(), M.max(), np.sqrt(np.mean(ref ** 2))))
    assert np.isfinite(ref).all() and 0.02 < ref.std() < 0.6
    assert E.max() <= FRAME_RMS_BAR and M.max() <= SAMPLE_BAR


def test_float32_path_agrees_with_float64_at_the_floor(path, floor):
    """the dtype parameter changes the precision and nothing else (torch's float32 sums are blocked differently from the oracle's: a few
    times its error)"""
    codes, _, ref = floor[7]
    f32 = R.torch_codec(path, codes)
    assert f32.dtype == np.float32
    E, M = R.frame_errors(f32, ref)
    print("float32 torch against float64: per-frame rms up to %.3g, max abs %.3g" % (E.max(), M.max()))
    assert E.max() <= 2e-6 and M.max() <= 3e-5      # the bars test_codec_mel_oracle.py holds this float32 restatement to, per frame here


def _bounds(floor):
    _, orc, ref = floor[7]
    E, M = R.frame_errors(orc, ref)
    return R.K_RMS * E.max(), R.K_MAX * M.max()


def test_the_whole_signal_bar_passes_what_the_per_frame_bounds_catch(floor):
    """two faults of the kind a streaming decoder makes, applied to the oracle's own output: both stay below 1e-4 whole-signal RMS, and
    each breaks a per-frame bound of test_gpu_codec_pcm_f64.py (K_RMS x the oracle's worst frame RMS, K_MAX x its worst sample) by more
    than 100 times"""
    assert R.K_RMS <= R.K_CAP and R.K_MAX <= R.K_CAP
    _, orc, ref = floor[7]
    rms_bound, max_bound = _bounds(floor)
    # a wrong halo at a chunk boundary: the last seven samples of the third 4-frame chunk off by 1e-3
    halo = orc.astype(np.float64)
    halo[12 * SPF - 7: 12 * SPF] += 1e-3
    # a history slot shifted by one at one chunk: one whole frame off by +-3e-4
    frame = orc.astype(np.float64)
    frame[9 * SPF: 10 * SPF] += 3e-4 * np.where(np.arange(SPF) % 2, -1.0, 1.0)
    for what, bad, f in (("halo", halo, 11), ("frame", frame, 9)):
        whole = float(np.sqrt(np.mean((bad - ref) ** 2)))
        E, M = R.frame_errors(bad, ref)
        print("%s: whole rms %.3g; frame %d rms %.3g = %.0f x bound, max %.3g = %.0f x bound"
              % (what, whole, f, E[f], E[f] / rms_bound, M[f], M[f] / max_bound))
        assert whole < PCM_RMS_TOL
        assert int(np.argmax(E)) == f and int(np.argmax(M)) == f
        assert max(E[f] / rms_bound, M[f] / max_bound) > 100
        ok = np.arange(24) != f                                           # and every other frame still passes
        assert (E[ok] <= rms_bound).all() and (M[ok] <= max_bound).all()


def test_prime_is_the_concatenation_cut(path, floor):
    codes = floor[7][0]
    rng = np.random.default_rng(9)
    p8, p3 = rng.integers(0, 2048, (8, 16)), rng.integers(0, 2048, (3, 16))
    whole = R.torch_codec(path, np.concatenate([p8, codes[:6]]), torch.float64)
    one = R.torch_codec(path, codes[:6], torch.float64, prime=p8)
    assert one.shape == (6 * SPF,) and np.array_equal(one, whole[8 * SPF:])
    cold = R.torch_codec(path, codes[:6], torch.float64)
    same = lambda a, b: a.shape == b.shape and np.abs(a - b).max() <= 1e-12  # other shapes reassociate torch's sums: float64 rounding
    assert same(cold, floor[7][2][: 6 * SPF])                             # causal: the first frames of a longer decode
    assert np.sqrt(np.mean((one[:SPF] - cold[:SPF]) ** 2)) >= 0.05        # priming is audible in the first frame
    # a list: primed and cold streams of different lengths, each as if decoded alone
    many = R.torch_codec(path, [codes[:6], codes[:6], codes[6:17], codes[:14]], torch.float64, prime=[p8, None, p3, None])
    assert [m.shape[0] for m in many] == [6 * SPF, 6 * SPF, 11 * SPF, 14 * SPF]   # 14 = 8 + 6 = 3 + 11: three streams share one pass
    assert same(many[0], one) and same(many[1], cold)
    assert same(many[2], R.torch_codec(path, np.concatenate([p3, codes[6:17]]), torch.float64)[3 * SPF:])
    assert same(many[3], floor[7][2][: 14 * SPF])


def test_frame_errors():
    ref = np.zeros(3 * SPF)
    got = ref.copy()
    got[SPF: 2 * SPF] = 2.0
    got[2 * SPF + 5] = -3.0
    E, M = R.frame_errors(got.astype(np.float32), ref)
    assert E.dtype == np.float64 and np.allclose(E, [0.0, 2.0, 3.0 / np.sqrt(SPF)]) and np.array_equal(M, [0.0, 2.0, 3.0])
    with pytest.raises(AssertionError):
        R.frame_errors(got[:-1], ref[:-1])
