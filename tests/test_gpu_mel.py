"""k_mel (csrc/mel.hip) against the float64 definition of tests/mel_ref.py on every case of tests/mel_cases.py.

Per output the comparison is mel_ref's step (4): above the floor |got - ln v| <= d_v / (v - d_v) + 2u |ln v|, below it logf(1e-5f) to 1 ulp,
and in between (at most 1 % of a case, asserted on the CPU) got lies between the two ends.  d_v follows the kernel's own sums
(mel_ref.kernel_bin_bound): there is no tolerance here that is not a formula of that docstring.  MEL_F64_REPORT=<path> appends one line per
case with the largest error / bound and the straddle share (profiles/voice_front_end_f64.md)."""
import ctypes as C
import os

import numpy as np
import pytest

import mel_cases
import mel_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tables(gpu):
    return gpu.mel_tables()


def _raw(gpu, audio, rows):
    """the C entry on a NaN-poisoned buffer of `rows` rows -> (status, buffer)"""
    audio = np.ascontiguousarray(audio, np.float32)
    src = audio if audio.size else np.zeros(1, np.float32)
    out = np.full((rows, 128), np.nan, np.float32)
    rc = gpu.lib().q3tts_mel(src.ctypes.data_as(C.c_void_p), audio.size, out.ctypes.data_as(C.c_void_p))
    return rc, out


@pytest.mark.parametrize("name", mel_cases.NAMES)
def test_mel_against_float64(name, gpu, tables):
    a = mel_cases.AUDIO[name]
    nf = R.frames(a.size)
    got = gpu.mel(a)
    assert got.shape == (nf, 128) and got.dtype == np.float32
    rc, buf = _raw(gpu, a, nf + 2)
    assert rc == 0
    assert np.all(np.isnan(buf[nf:]))                      # rows past the frame count stay poisoned
    assert np.array_equal(buf[:nf], got)                   # and the same audio gives the same bits twice
    v, _, dv = R.mel64(a, *tables)
    assert v.shape == got.shape
    if nf == 0:
        return
    assert np.all(np.isfinite(got))
    e = R.above_excess(got, v, dv)
    above, floor, straddle = R.classify(v, dv)
    share = straddle.mean()
    ulps = np.abs(got[floor].astype(np.float64) - float(R.LN_FLOOR32)).max() / R.ULP_LN_FLOOR if floor.any() else 0.0
    print("%s: error / bound %.3g above the floor (%d outputs), floor class %d outputs within %.0f ulp, straddle share %.4f"
          % (name, e, above.sum(), floor.sum(), ulps, share))
    rep = os.environ.get("MEL_F64_REPORT")
    if rep:
        with open(rep, "a") as f:
            f.write("%s %d %d %d %.4g %d %.0f %.4f\n" % (name, a.size, nf, above.sum(), e, floor.sum(), ulps, share))
    lo, hi = R.limits(v, dv)
    assert np.all(got >= lo) and np.all(got <= hi), "error / bound %.3g" % e


@pytest.mark.parametrize("n", [0, 255])
def test_no_frame_is_ok_and_writes_nothing(n, gpu):
    a = mel_cases.AUDIO["noise_255"][:n]
    assert gpu.mel_frames(n) == 0 and gpu.mel(a).shape == (0, 128)
    rc, buf = _raw(gpu, a, 2)
    assert rc == 0 and np.all(np.isnan(buf))
    assert gpu.mel(np.zeros(100, np.float32)).shape == (0, 128)


def test_bad_arguments_are_errors(gpu):
    L = gpu.lib()
    a = np.zeros(512, np.float32)
    out = np.full((4, 128), np.nan, np.float32)
    pa, po = a.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert L.q3tts_mel(pa, -1, po) != 0 and b"bad arguments" in L.q3tts_last_error()
    assert L.q3tts_mel(None, 512, po) != 0
    assert L.q3tts_mel(pa, 512, None) != 0
    assert np.all(np.isnan(out))
    assert L.q3tts_mel_tables(None, None) != 0


def test_encode_speaker_refuses_a_clip_without_a_frame(gpu, tiny_model, tmp_path):
    """TtsEngine::encode_speaker (host/tts_engine.cpp) sizes its buffer with q3tts_mel_frames: a clip below 256 samples used to count as one frame
    of zeros and reach the encoder; now it raises "audio too short".  The speaker encoder here is a two-node graph (mean over frames, Gemm)."""
    import subprocess
    import onnx_writer as W
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "qwen3-tts-rust_amd")
    mdir = tmp_path / "model"
    (mdir / "onnx").mkdir(parents=True)
    for e in os.listdir(tiny_model):
        if e != "onnx":
            os.symlink(os.path.join(tiny_model, e), str(mdir / e))
    for e in os.listdir(os.path.join(tiny_model, "onnx")):
        os.symlink(os.path.join(tiny_model, "onnx", e), str(mdir / "onnx" / e))
    fc = (np.random.default_rng(5).standard_normal((2048, 128)) * 0.1).astype(np.float32)
    nodes = [W.node("ReduceMean", ["mels"], ["mu"], attrs=[W.attr_ints("axes", [1]), W.attr_int("keepdims", 0)]),
             W.node("Gemm", ["mu", "fc"], ["spk_emb"], attrs=[W.attr_int("transB", 1)])]
    with open(str(mdir / "onnx" / "qwen3_tts_speaker_encoder.onnx"), "wb") as f:
        f.write(W.model(nodes, [W.tensor("fc", fc)], [W.value_info("mels", W.F32, [1, "n", 128])], [W.value_info("spk_emb", W.F32, [1, 2048])], opset=13))
    exe = str(tmp_path / "short_clip_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(root, "tests", "host", "short_clip_main.cpp"), "-L" + pkg, "-lq3tts_host", "-lq3tts",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe, str(mdir)], capture_output=True, text=True, cwd=str(tmp_path), timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-500:], r.stderr[-2000:])
