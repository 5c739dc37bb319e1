"""[EXT] reference audio intake on the GPU: k_intake through q3tts_intake, against the float64 restatement of tests/intake_ref.py.  The
restatement is fed the library's own f32 table, so only the kernel's arithmetic is judged: a result must lie within the restatement's
per-sample running-error bound, and where the definition leaves one term per sum, or none, it must be the bits.  Every output buffer is
over-allocated and checked behind its last sample."""
import functools
import os
import subprocess

import numpy as np
import pytest

import intake_ref as R
import onnx_writer as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NON_NATIVE = [r for r in R.RATES if r != R.NATIVE]
FILL, SLACK = 0x5A, 8
CHANNELS = (1, 2, 3, 8)
F32, I64 = 1, 7


@functools.lru_cache(maxsize=None)
def h32_of(gpu_mod, rate):
    return gpu_mod.intake_filter(rate) if rate != R.NATIVE else None


def make_clip(rng, rate, fmt, channels, mix, n):
    """(the tuple q3.intake takes, the same for the restatement)"""
    raw = R.random_raw(rng, fmt, n, channels)
    raw.setflags(write=False)
    return (raw, rate, channels, fmt, mix)


def run(gpu, clips, **kw):
    """one q3tts_intake; checks what every case must hold: counts and the untouched slack behind every output"""
    outs, wholes, n_out = gpu.intake(clips, slack=SLACK, fill=FILL, **kw)
    for o, w, n, c in zip(outs, wholes, n_out, clips):
        frames = np.asarray(c[0]).nbytes // (R.SAMPLE_BYTES[c[3]] * c[2])
        assert n == o.size == R.n_out(c[1], frames) == gpu.intake_samples(c[1], frames)
        assert np.all(w.view(np.uint8)[4 * n:] == FILL) and w.size == n + SLACK, "a write behind the clip's samples"
    return outs


def check(gpu, clips, outs, what=""):
    """every output against the restatement, within its bound (24000 Hz: the bits)"""
    worst = 0.0
    for c, o in zip(clips, outs):
        raw, rate, ch, fmt, mix = c
        y, bound = R.intake(raw, rate, ch, fmt, mix, h32_of(gpu, rate))
        assert o.dtype == np.float32 and o.size == y.size
        if rate == R.NATIVE:
            assert np.array_equal(o.view(np.uint32), y.astype(np.float32).view(np.uint32))
            continue
        err = np.abs(o.astype(np.float64) - y)
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
        assert np.all(err <= bound), (what, rate, ch, fmt, mix, o.size, float(err.max()))
    print("%s: worst err / bound %.3g over %d clips" % (what, worst, len(clips)))


def edge_frames(gpu, rate):
    """frame counts whose sample counts sit at the places where the kernel's paths change: one output, one short of a full sum, around one and
    two tiles of this ratio's tile; and n L mod M of 0 and of 1.  Upsampling ratios cannot reach every count: the nearest on either side"""
    L, M, N, taps = R.plan(rate)
    tile = gpu.intake_tile(rate)
    ns = set()
    for target in (1, max(taps - 1, 1), tile - 1, tile, tile + 1, 2 * tile + 1):
        ns.update((max(target * M // L, 1), -(-target * M // L)))
    ns.add(5 * M)                                                        # n L mod M == 0
    if M > 1:
        ns.add(next(n for n in range(3 * M + 1, 4 * M + 1) if n * L % M == 1))
    counts = {R.n_out(rate, n) for n in ns}
    if L <= M:   # every count is reachable when downsampling
        assert {1, max(taps - 1, 1), tile - 1, tile, tile + 1, 2 * tile + 1} <= counts
    return sorted(ns)


@pytest.mark.parametrize("rate", R.RATES)
def test_every_rate_at_the_tile_edges(gpu, rate):
    rng = np.random.default_rng(rate)
    clips = [make_clip(rng, rate, R.FORMATS[i % 5], CHANNELS[i % 4], i % 2, n) for i, n in enumerate(edge_frames(gpu, rate))]
    check(gpu, clips, run(gpu, clips), "%d Hz" % rate)


@pytest.mark.parametrize("rate", [16000, 44100, 24000, 191400])
def test_every_format_channel_count_and_downmix(gpu, rate):
    """40 clips in one launch; 191400 Hz is a ratio (40 / 319) whose tile the host has to shrink to fit"""
    rng = np.random.default_rng(7)
    n = 1500 * rate // 24000 + 3
    clips = [make_clip(rng, rate, fmt, ch, mix, n + 2 * i) for i, (fmt, ch, mix) in enumerate((f, c, m) for f in R.FORMATS for c in CHANNELS for m in (R.FIRST, R.MEAN))]
    outs = run(gpu, clips)
    check(gpu, clips, outs, "%d Hz, formats" % rate)
    # the downmix happens in front of the filter: a clip equals, bit for bit, the mono f32 clip of its decoded and downmixed frames
    pick = [3, 17, 38]
    mono = [(R.downmix(R.decode(clips[i][0], clips[i][3], clips[i][2]), clips[i][4]), rate, 1, R.F32, R.FIRST) for i in pick]
    for i, o in zip(pick, run(gpu, mono)):
        assert np.array_equal(o.view(np.uint32), outs[i].view(np.uint32)), i


@pytest.mark.parametrize("rate", NON_NATIVE)
def test_an_impulse_returns_the_prototype_taps(gpu, rate):
    """one nonzero term per sum: h[c + m M - i L] * 1.0 + 0, exact"""
    L, M, N, taps = R.plan(rate)
    h, c = h32_of(gpu, rate), R.Z * max(L, M)
    n = 3 * max(M // L, 1) * 40 + 11
    clips, at = [], (0, n - 1, n // 2)
    for i in at:
        x = np.zeros(n, np.float32)
        x[i] = 1.0
        clips.append((x, rate, 1, R.F32, R.FIRST))
    for i, o in zip(at, run(gpu, clips)):
        idx = c + np.arange(o.size, dtype=np.int64) * M - i * L
        want = np.where((idx >= 0) & (idx < N), h[np.clip(idx, 0, N - 1)], np.float32(0.0)).astype(np.float32)
        assert np.count_nonzero(want) >= 16 and np.array_equal(o, want), (rate, i)


def test_24000_hz_is_the_decode_and_downmix_bit_for_bit(gpu):
    """what the engine's own reader (read_wav_for_voice: s16 v / 32768, s32 (float)v / 2147483648, f32 as it is, channel 0) makes of the clip"""
    rng = np.random.default_rng(24)
    clips = [make_clip(rng, 24000, fmt, ch, mix, 2051) for fmt in R.FORMATS for ch in (1, 2) for mix in (R.FIRST, R.MEAN)]
    special = np.array([0.0, -0.0, 1e-45, -1e-45, 3e38, -3e38, 1.0, -1.0], np.float32)   # zeros, subnormals and large values pass as they are
    clips.append((special, 24000, 1, R.F32, R.FIRST))
    outs = run(gpu, clips)
    for c, o in zip(clips, outs):
        raw, rate, ch, fmt, mix = c
        x = R.decode(raw, fmt, ch)
        if mix == R.FIRST:
            b = np.ascontiguousarray(raw).view(np.uint8)
            own = {R.S16: lambda: b.view("<i2").astype(np.float32) / np.float32(32768.0), R.S32: lambda: b.view("<i4").astype(np.float32) / np.float32(2147483648.0),
                   R.F32: lambda: b.view("<f4")}.get(fmt)
            if own:
                assert np.array_equal(o.view(np.uint32), own()[::ch].astype(np.float32).view(np.uint32))
        assert np.array_equal(o.view(np.uint32), R.downmix(x, mix).view(np.uint32)), (fmt, ch, mix)


def mixed_batch():
    rng = np.random.default_rng(99)
    spec = [(44100, R.S16, 2, R.MEAN, 5000), (8000, R.U8, 1, R.FIRST, 90), (192000, R.S24, 3, R.MEAN, 30011), (24000, R.F32, 2, R.FIRST, 777),
            (11025, R.S32, 8, R.MEAN, 1), (48000, R.F32, 1, R.FIRST, 4099), (176400, R.S16, 2, R.FIRST, 17000)]
    return [make_clip(rng, r, f, c, m, n) for r, f, c, m, n in spec]


def test_a_clip_does_not_depend_on_its_batch(gpu):
    clips = mixed_batch()
    whole = run(gpu, clips)
    check(gpu, clips, whole, "mixed batch")
    again = run(gpu, clips)
    for a, b in zip(whole, again):                                       # two calls: identical bits
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    order = [4, 6, 0, 2, 5, 1, 3]
    for k, o in zip(order, run(gpu, [clips[k] for k in order])):         # any position
        assert np.array_equal(o.view(np.uint32), whole[k].view(np.uint32)), k
    for k in (0, 2, 4, 6):                                               # alone
        assert np.array_equal(run(gpu, [clips[k]])[0].view(np.uint32), whole[k].view(np.uint32)), k
    full = [clips[i % len(clips)] for i in range(R.MAX_CLIPS)]           # and 64 clips are taken
    for i, o in enumerate(run(gpu, full)):
        assert np.array_equal(o.view(np.uint32), whole[i % len(clips)].view(np.uint32)), i


@pytest.mark.parametrize("rate", [11025, 191400])
def test_a_120_s_clip_last_tile(gpu, rate):
    """m M + c and i L at their largest: 2 880 000 outputs; only the last tile is compared"""
    L, M, N, taps = R.plan(rate)
    n = R.MAX_OUT * M // L
    assert R.n_out(rate, n) == R.MAX_OUT and R.n_out(rate, n + 1) > R.MAX_OUT
    clip = make_clip(np.random.default_rng(120), rate, R.U8, 1, R.FIRST, n)
    (o,) = run(gpu, [clip])
    tile = gpu.intake_tile(rate)
    m0 = (R.MAX_OUT - 1) // tile * tile - tile                            # the last two tiles
    y, bound = R.intake(clip[0], rate, 1, R.U8, R.FIRST, h32_of(gpu, rate), m0=m0, count=R.MAX_OUT - m0)
    err = np.abs(o[m0:].astype(np.float64) - y)
    assert np.all(err <= bound) and np.abs(o[m0:]).max() > 0.1, float(err.max())


REFUSALS = {
    "bad rate": (lambda c: (c[0], 24001) + c[2:], "rate"),
    "no channels": (lambda c: (c[0], c[1], 0) + c[3:], "channel"),
    "nine channels": (lambda c: (c[0], c[1], 9) + c[3:], "channel"),
    "bad format": (lambda c: c[:3] + (5, c[4]), "format"),
    "bad downmix": (lambda c: c[:4] + (2,), "downmix"),
    "no frames": (lambda c: c[:5] + (0,), "empty"),
    "too long": (lambda c: (np.zeros(R.MAX_OUT // 3 + 1, np.uint8), 8000, 1, R.U8, R.FIRST), "120 s"),
}


@pytest.mark.parametrize("what", sorted(REFUSALS) + ["capacity short", "65 clips", "no clips"])
def test_refusals_leave_the_outputs_untouched(gpu, what):
    clips, kw, word = mixed_batch()[:3], {}, "clip 1"
    if what in REFUSALS:
        clips[1], word2 = REFUSALS[what][0](clips[1]), REFUSALS[what][1]
    elif what == "capacity short":
        kw["caps"] = [R.n_out(c[1], c[0].nbytes // (R.SAMPLE_BYTES[c[3]] * c[2])) - (i == 1) for i, c in enumerate(clips)]
        word2 = "fewer"
    else:
        clips, word, word2 = (clips * 22)[:65] if what == "65 clips" else [], "clip count", "64"
    with pytest.raises(gpu.Q3Error) as ei:
        gpu.intake(clips, slack=SLACK, fill=FILL, **kw)
    ex = ei.value
    assert "intake" in str(ex) and word in str(ex) and word2 in str(ex), str(ex)
    assert len(ex.wholes) == len(clips) and all(np.all(w.view(np.uint8) == FILL) for w in ex.wholes) and np.all(ex.n_out == -1)


@pytest.mark.parametrize("rate", [44100, 24000, 8000])
def test_a_non_finite_sample_fails_the_call_and_names_the_clip(gpu, rate):
    L, M, N, taps = R.plan(rate)
    tile = gpu.intake_tile(rate)
    n = (2 * tile + 100) * M // L
    rng = np.random.default_rng(3)
    good = [make_clip(rng, 16000, R.S16, 2, R.MEAN, 3000), make_clip(rng, 48000, R.F32, 1, R.FIRST, 3000)]
    base = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    for at in (0, n - 1, tile * M // L, -(-tile * M // L)):               # the first and the last frame, both sides of the first tile boundary
        for bad, ch, mix in ((np.nan, 0, R.FIRST), (np.inf, 1, R.MEAN), (-np.inf, 0, R.MEAN)):
            x = base.copy()
            x[at, ch] = bad
            with pytest.raises(gpu.Q3Error) as ei:
                gpu.intake(good + [(x, rate, 2, R.F32, mix)], slack=SLACK, fill=FILL)
            ex = ei.value
            assert "clip 2" in str(ex) and "non-finite" in str(ex), str(ex)
            assert all(np.all(w.view(np.uint8) == FILL) for w in ex.wholes) and np.all(ex.n_out == -1)
    x = base.copy()
    x[5, 1] = np.nan                                                     # channel 1 is not read when channel 0 is taken
    outs = run(gpu, good + [(x, rate, 2, R.F32, R.FIRST)])
    assert np.isfinite(outs[2]).all()
    big = np.full((64, 2), 3e38, np.float32)                             # a mean that overflows is not finite either
    with pytest.raises(gpu.Q3Error, match="clip 0"):
        gpu.intake([(big, rate, 2, R.F32, R.MEAN)])


def test_wav_intake_reads_a_file_of_any_form(gpu, tmp_path):
    rng = np.random.default_rng(8)
    for k, (fmt, ch, rate, ext) in enumerate(((R.S24, 2, 44100, False), (R.U8, 1, 8000, False), (R.F32, 3, 96000, True), (R.S32, 2, 24000, True))):
        raw = R.random_raw(rng, fmt, 2000 + k, ch)
        path = str(tmp_path / ("clip%d.wav" % k))
        open(path, "wb").write(R.wav_bytes(raw, fmt, ch, rate, extensible=ext, junk=b"odd" if k & 1 else None))
        for mix in (R.FIRST, R.MEAN):
            y, info = gpu.wav_intake(path, mix)
            assert (info["sample_format"], info["channels"], info["sample_rate"], info["n_frames"]) == (fmt, ch, rate, 2000 + k)
            (want,) = gpu.intake([(raw, rate, ch, fmt, mix)])
            assert np.array_equal(y.view(np.uint32), want.view(np.uint32))
    bad = str(tmp_path / "bad.wav")
    open(bad, "wb").write(R.wav_bytes(raw, R.S16, 2, 48000)[:30])
    with pytest.raises(gpu.Q3Error, match="WAV error"):
        gpu.wav_intake(bad)
    with pytest.raises(gpu.Q3Error, match="cannot open"):
        gpu.wav_intake(str(tmp_path / "missing.wav"))


def _encoder_graphs(mdir, rng):
    """the voice-clone encoders as small test-written graphs with the reference's tensor names: input_values [1, T] -> audio_codes [1, F, 16]
    (two strided convolutions, then 16 quantisers = argmax over 16 slices of a projection) and mels [1, n, 128] -> spk_emb [1, 2048] (a
    convolution, mean and deviation pooling, a linear layer)"""
    D, NQ, CB, C = 12, 16, 8, 16
    Pc = {"w1": (rng.standard_normal((8, 1, 9)) * 0.3).astype(np.float32), "b1": (rng.standard_normal(8) * 0.1).astype(np.float32),
          "w2": (rng.standard_normal((D, 8, 16)) * 0.1).astype(np.float32), "b2": (rng.standard_normal(D) * 0.1).astype(np.float32),
          "proj": (rng.standard_normal((D, NQ * CB)) * 0.5).astype(np.float32)}
    cn = [W.node("Unsqueeze", ["input_values", "ax1"], ["x"]),
          W.node("Conv", ["x", "w1", "b1"], ["h1"], attrs=[W.attr_ints("strides", [8]), W.attr_ints("pads", [4, 4])]), W.node("Elu", ["h1"], ["h1e"]),
          W.node("Conv", ["h1e", "w2", "b2"], ["h2"], attrs=[W.attr_ints("strides", [16]), W.attr_ints("pads", [8, 7])]), W.node("Tanh", ["h2"], ["h2t"]),
          W.node("Transpose", ["h2t"], ["t"], attrs=[W.attr_ints("perm", [0, 2, 1])]), W.node("MatMul", ["t", "proj"], ["lg"]),
          W.node("Shape", ["lg"], ["lgs"]), W.node("Slice", ["lgs", "c0", "c2"], ["bf"]), W.node("Concat", ["bf", "qc"], ["ns"], attrs=[W.attr_int("axis", 0)]),
          W.node("Reshape", ["lg", "ns"], ["lg4"]), W.node("ArgMax", ["lg4"], ["audio_codes"], attrs=[W.attr_int("axis", 3), W.attr_int("keepdims", 0)])]
    ci = [W.tensor(k, v) for k, v in Pc.items()] + [W.tensor("ax1", np.asarray([1], np.int64)), W.tensor("c0", np.asarray([0], np.int64)),
                                                   W.tensor("c2", np.asarray([2], np.int64)), W.tensor("qc", np.asarray([NQ, CB], np.int64))]
    Ps = {"w0": (rng.standard_normal((C, 128, 3)) * 0.05).astype(np.float32), "b0": (rng.standard_normal(C) * 0.1).astype(np.float32),
          "fc": (rng.standard_normal((2048, 2 * C)) * 0.1).astype(np.float32), "fcb": (rng.standard_normal(2048) * 0.1).astype(np.float32)}
    sn = [W.node("Transpose", ["mels"], ["x"], attrs=[W.attr_ints("perm", [0, 2, 1])]), W.node("Conv", ["x", "w0", "b0"], ["h"], attrs=[W.attr_ints("pads", [1, 1])]),
          W.node("Relu", ["h"], ["hr"]), W.node("ReduceMean", ["hr"], ["mu"], attrs=[W.attr_ints("axes", [2]), W.attr_int("keepdims", 0)]),
          W.node("Mul", ["hr", "hr"], ["h2"]), W.node("ReduceMean", ["h2"], ["m2"], attrs=[W.attr_ints("axes", [2]), W.attr_int("keepdims", 0)]),
          W.node("Mul", ["mu", "mu"], ["mumu"]), W.node("Sub", ["m2", "mumu"], ["var"]), W.node("Relu", ["var"], ["varp"]), W.node("Sqrt", ["varp"], ["sd"]),
          W.node("Concat", ["mu", "sd"], ["st"], attrs=[W.attr_int("axis", 1)]), W.node("Gemm", ["st", "fc", "fcb"], ["spk_emb"], attrs=[W.attr_int("transB", 1)])]
    si = [W.tensor(k, v) for k, v in Ps.items()]
    open(os.path.join(mdir, "onnx", "qwen3_tts_codec_encoder.onnx"), "wb").write(
        W.model(cn, ci, [W.value_info("input_values", F32, [1, "T"])], [W.value_info("audio_codes", I64, [1, "F", 16])], opset=13))
    open(os.path.join(mdir, "onnx", "qwen3_tts_speaker_encoder.onnx"), "wb").write(
        W.model(sn, si, [W.value_info("mels", F32, [1, "n", 128])], [W.value_info("spk_emb", F32, [1, 2048])], opset=13))


def test_create_voice_file_and_generate_through_the_intake(gpu, tiny_model, tmp_path):
    """end to end through the C++ mirror of the reference API (tests/host/intake_main.cpp)"""
    rng = np.random.default_rng(12)
    mdir = tmp_path / "model"
    (mdir / "onnx").mkdir(parents=True)
    for e in os.listdir(tiny_model):
        if e != "onnx":
            os.symlink(os.path.join(tiny_model, e), str(mdir / e))
    for e in os.listdir(os.path.join(tiny_model, "onnx")):
        os.symlink(os.path.join(tiny_model, "onnx", e), str(mdir / "onnx" / e))
    _encoder_graphs(str(mdir), rng)
    t = np.arange(48000) / 48000.0
    left = np.sin(2 * np.pi * 220 * t) * 0.4 + rng.standard_normal(t.size) * 0.05
    right = np.sin(2 * np.pi * 330 * t) * 0.3 + rng.standard_normal(t.size) * 0.05
    stereo = R.encode(np.stack([left, right], 1), R.S16)
    clip48, first24, mean24, ref2 = [str(tmp_path / n) for n in ("clip48k.wav", "first24k.wav", "mean24k.wav", "ref2_44k.wav")]
    open(clip48, "wb").write(R.wav_bytes(stereo, R.S16, 2, 48000))
    open(ref2, "wb").write(R.wav_bytes(R.encode(left[:22050], R.S24), R.S24, 1, 44100, extensible=True))
    for path, mix in ((first24, R.FIRST), (mean24, R.MEAN)):
        y, info = gpu.wav_intake(clip48, mix)
        assert y.size == 24000 and info["sample_rate"] == 48000 and info["channels"] == 2
        open(path, "wb").write(R.wav_bytes(y, R.F32, 1, 24000))
    assert open(first24, "rb").read() != open(mean24, "rb").read()
    pkg = os.path.join(ROOT, "qwen3-tts-rust_amd")
    exe = str(tmp_path / "intake_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "host", "intake_main.cpp"), "-L" + pkg, "-lq3tts_host", "-lq3tts",
                           "-Wl,-rpath," + pkg])
    r = subprocess.run([exe, str(mdir), clip48, first24, mean24, ref2], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and r.stdout.strip().endswith("OK"), (r.stdout[-500:], r.stderr[-2000:])
    assert "MODE 0 CODES" in r.stdout and "MODE 1 CODES" in r.stdout
    assert os.path.exists(str(tmp_path / "ref2_44k.intake.cache")) and not os.path.exists(str(tmp_path / "ref2_44k.cache"))
