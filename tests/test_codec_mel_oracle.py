"""Codec decoder oracle: chunked streaming == one full pass, and the whole stack == an independent torch.nn.functional
re-implementation of the same architecture (conv1d / conv_transpose1d / layer_norm / gelu / softmax).
Mel front end: oracle vs a numpy restatement of /root/reference/src/models/onnx.rs:167-320."""
import os
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from codec_f64_ref import torch_codec   # the restatement lives in tests/codec_f64_ref.py; float32 here, as always


def test_codec_streaming_equals_full_and_matches_torch(tiny_model, oracle):
    path = os.path.join(tiny_model, "onnx", "q3tts_codec.gguf")
    c = oracle.Codec(path)
    assert c.spf == 1920
    rng = np.random.default_rng(7)
    codes = rng.integers(0, 2048, (21, 16))   # 21 frames > window(8)+chunking: exercises the sliding KV history
    c.reset(); full = c.decode(codes).copy()
    for chunks in ([4, 4, 4, 4, 4, 1], [1] * 21, [7, 14], [20, 1]):
        c.reset()
        parts, o = [], 0
        for i, n in enumerate(chunks):
            parts.append(c.decode(codes[o:o + n], i == len(chunks) - 1).copy()); o += n
        assert np.array_equal(np.concatenate(parts), full), chunks
    with torch.no_grad():
        ref = torch_codec(path, torch.from_numpy(codes))
    assert ref.shape == full.shape
    assert np.sqrt(np.mean((ref - full) ** 2)) < 2e-6 and np.abs(ref - full).max() < 3e-5
    assert 0.02 < full.std() < 0.6 and np.abs(full).max() <= 1.0
    c.close()


def numpy_mel(audio):
    """onnx.rs:167-320 restated with numpy (float64 FFT)."""
    sr, n_fft, hop, n_mels = 24000.0, 1024, 256, 128
    f32 = np.float32

    def hz_to_mel(f):
        f_sp = f32(200.0) / f32(3.0); min_log_hz = f32(1000.0); min_log_mel = min_log_hz / f_sp
        logstep = np.log(f32(6.4)) / f32(27.0)
        return min_log_mel + np.log(f / min_log_hz) / logstep if f >= min_log_hz else f / f_sp

    def mel_to_hz(m):
        f_sp = f32(200.0) / f32(3.0); min_log_hz = f32(1000.0); min_log_mel = min_log_hz / f_sp
        logstep = np.log(f32(6.4)) / f32(27.0)
        return min_log_hz * np.exp(logstep * (m - min_log_mel)) if m >= min_log_mel else f_sp * m
    mmin, mmax = hz_to_mel(f32(0)), hz_to_mel(f32(12000))
    edges = [mel_to_hz(f32(mmin + (mmax - mmin) * f32(i) / f32(n_mels + 1))) for i in range(n_mels + 2)]
    freqs = np.arange(n_fft // 2 + 1, dtype=np.float32) * f32(sr) / f32(n_fft)
    fb = np.zeros((n_mels, n_fft // 2 + 1), np.float32)
    for m in range(n_mels):
        fl, fc, fr = edges[m], edges[m + 1], edges[m + 2]
        up = (freqs - fl) / (fc - fl); dn = (fr - freqs) / (fr - fc)
        w = np.where((freqs >= fl) & (freqs <= fc), up, np.where((freqs > fc) & (freqs <= fr), dn, 0))
        fb[m] = w * (f32(2.0) / (fr - fl))
    pad = (n_fft - hop) // 2
    n = len(audio)
    head = [audio[i] if i < n else 0.0 for i in range(pad, 0, -1)]
    tail = [audio[max(n - 1 - i, 0)] if n > 0 else 0.0 for i in range(1, pad + 1)]
    x = np.concatenate([head, audio, tail]).astype(np.float32)
    hann = (0.5 * (1 - np.cos(2 * np.pi * np.arange(n_fft) / n_fft))).astype(np.float32)
    out = []
    for f in range((max(len(x) - n_fft, 0)) // hop + 1):
        if f * hop + n_fft > len(x):
            break
        spec = np.fft.rfft((x[f * hop:f * hop + n_fft] * hann).astype(np.float64))
        mag = np.sqrt(np.abs(spec) ** 2 + 1e-9)
        out.append(np.log(np.maximum(fb.astype(np.float64) @ mag, 1e-5)))
    return np.array(out, np.float32)


def test_mel_matches_transformers_audio_utils(oracle):
    """Independent pin of row a16: the installed `transformers.audio_utils` builds the same Slaney-scale, Slaney-normalised 128-filter
    bank (0-12 kHz, 513 bins) and a Hann/1024/256 power-1 spectrogram; the oracle's mel of a chirp must agree with it.  Framing differs
    only in the padding rule (reference: reflect pad 384 by hand, onnx.rs:255-271), so the clip is pre-padded the reference's way."""
    from transformers.audio_utils import mel_filter_bank, spectrogram, window_function
    rng = np.random.default_rng(5)
    t = np.arange(24000) / 24000.0
    audio = (0.4 * np.sin(2 * np.pi * (300 + 2500 * t) * t) + 0.02 * rng.standard_normal(t.size)).astype(np.float32)
    pad = 384
    padded = np.concatenate([audio[pad:0:-1], audio, audio[-2:-pad - 2:-1]]).astype(np.float64)
    fb = mel_filter_bank(num_frequency_bins=513, num_mel_filters=128, min_frequency=0.0, max_frequency=12000.0, sampling_rate=24000,
                         norm="slaney", mel_scale="slaney")
    spec = spectrogram(padded, window_function(1024, "hann", periodic=True), frame_length=1024, hop_length=256, fft_length=1024, power=1.0,
                       center=False, mel_filters=fb, mel_floor=1e-5, log_mel="log")
    ref = spec.T.astype(np.float32)                       # [frames][128]
    got = oracle.mel(audio)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() < 5e-3                 # |FFT| gets +1e-9 under the root in the reference; f32 vs f64 pipelines


def test_mel_matches_numpy_restatement(oracle):
    rng = np.random.default_rng(11)
    t = np.arange(24000 * 2) / 24000.0
    chirp = (0.4 * np.sin(2 * np.pi * (200 + 3000 * t) * t) + 0.05 * rng.standard_normal(t.size)).astype(np.float32)
    for audio in (chirp, chirp[:5000], chirp[:300], np.zeros(1500, np.float32)):   # incl. clip shorter than the 384 pad
        got = oracle.mel(audio)
        ref = numpy_mel(audio)
        assert got.shape == ref.shape and got.shape[1] == 128
        assert np.abs(got - ref).max() < 2e-3
    assert oracle.mel(chirp).shape[0] == (len(chirp) + 768 - 1024) // 256 + 1
