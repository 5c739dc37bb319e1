"""Full-size ("Q3TTS-1.7B-synth", BASELINE.json configs[1..3] shapes) checks on the GPU: a short oracle comparison plus
size-independent properties (determinism, batch invariance, code ranges, chunk-count bookkeeping)."""
import os
import subprocess
import numpy as np
import pytest

import synth_models

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def full_model(synth_tool):
    return synth_models.full("q8_0")


def test_fullsize_parity_and_properties(gpu, oracle, full_model, vivian):
    ge = gpu.Engine(full_model, "q8_0", max_batch=2, max_steps=64, load_codec=True)
    rng = np.random.default_rng(42)
    prompt = ge.assets.build_core(rng.integers(0, 4000, 32).astype(np.int32), lang_id=2055, spk_emb=vivian)
    assert prompt.shape == (43, 2048)
    r = ge.generate_batch([prompt], max_steps=24, mask_eos=True, want_pcm=True)[0]
    assert r["codes"].shape == (24, 16) and r["codes"][:, 0].max() < 2160 and r["codes"][:, 1:].max() < 2048 and r["codes"].min() >= 0
    assert r["pcm"].size == 24 * 1920 and np.isfinite(r["pcm"]).all() and np.abs(r["pcm"]).max() <= 1.0
    # oracle on the host for the first frames (~0.3 s/frame + 43-token prefill)
    oe = oracle.Engine(os.path.join(full_model, "gguf_q8_0"), None, 8)
    oc, _ = oe.generate(prompt, max_steps=6, mask_eos=True)
    oe.close()
    assert np.array_equal(oc, r["codes"][:6])
    # determinism + batch invariance at full size
    r2 = ge.generate_batch([prompt, prompt], max_steps=24, mask_eos=True)
    assert np.array_equal(r2[0]["codes"], r["codes"]) and np.array_equal(r2[1]["codes"], r["codes"])
    # streaming codec == the codec oracle on the generated codes (first 5 frames: ~1 s of CPU)
    oc2 = oracle.Codec(os.path.join(full_model, "onnx", "q3tts_codec.gguf")); oc2.reset()
    ref = oc2.decode(np.clip(r["codes"][:5], 0, 2047)).copy(); oc2.close()
    assert np.sqrt(np.mean((ref - r["pcm"][: ref.size]) ** 2)) < 1e-4
    ge.close()


def test_fullsize_long_context_crosses_kv_pages_vs_oracle(gpu, oracle, full_model, vivian):
    """VERDICT r2 weak 2 ("full-size oracle comparisons are short: context < 60 positions"): two utterances step together through a 2-slot engine until
    their contexts cross KV page boundaries DURING decode -- 43 prompt rows + 40 frames (positions 43..82: the 64-position page boundary at frame 21) and
    75 prompt rows + 56 frames (75..130: the prompt itself spans two pages, the 128 boundary falls at frame 53) -- and every one of the 96 frames x 16
    codes is compared with the oracle run alone on the host (bit-exact).  Exercises the paged attention kernels over 2 and 3 pages, the page-table rows
    of both slots, ragged retirement and the talker's second 256-position attention chunk being absent (n < 256) at full head count."""
    ge = gpu.Engine(full_model, "q8_0", max_batch=2, max_steps=64, load_codec=False)
    prompts, steps = [], (40, 56)
    for i, n_text in enumerate((32, 64)):
        rng = np.random.default_rng(900 + i)
        prompts.append(ge.assets.build_core(rng.integers(0, 4000, n_text).astype(np.int32), lang_id=2055, spk_emb=vivian))
    assert [p.shape[0] for p in prompts] == [43, 75]
    res = ge.generate_batch(prompts, max_steps=list(steps), mask_eos=True)
    ge.close()
    oe = oracle.Engine(os.path.join(full_model, "gguf_q8_0"), None, 32)
    for p, m, r in zip(prompts, steps, res):
        oc, _ = oe.generate(p, max_steps=m, mask_eos=True)
        assert r["codes"].shape == (m, 16)
        bad = np.nonzero((oc != r["codes"]).any(axis=1))[0]
        assert bad.size == 0, "first differing frame %d of %d (prompt rows %d)" % (int(bad[0]), m, p.shape[0])
    oe.close()


def test_fullsize_batched_c3_shapes_vs_oracle_singles(gpu, oracle, full_model, vivian):
    """BASELINE config C3 as bench.py runs it: 64 slots of the full Q3TTS-1.7B-synth model step together (the 64-wide frame graph, every
    batched kernel form at K = 2048 / 6144 (talker) and K = 1024 / 3072 (predictor), the multi-sequence prefill over the bench's
    27 / 43 / 75-row prompts on the async lane, 4 codec groups over 2 lanes, two codec chunks per stream), ragged lengths so continuous
    batching retires slots at different frames.  Three of the 64 requests are compared with the oracle run ALONE on the host (tokens
    bit-exact), one with the oracle codec (PCM 1e-4 RMS), and one request alone must give the tokens and PCM it gave inside the batch."""
    ge = gpu.Engine(full_model, "q8_0", max_batch=64, max_steps=16, load_codec=True)
    prompts = []
    for i in range(64):
        rng = np.random.default_rng(500 + i)
        prompts.append(ge.assets.build_core(rng.integers(0, 4000, (16, 32, 64)[i % 3]).astype(np.int32), lang_id=2055, spk_emb=vivian))
    assert [p.shape[0] for p in prompts[:3]] == [27, 43, 75]
    ms = [8 + (i % 4) for i in range(64)]            # ragged lengths (8..11 frames: two codec chunks + a partial one per stream)
    res = ge.generate_batch(prompts, max_steps=ms, mask_eos=True, want_pcm=True)
    st = ge.stats()
    assert st["slot_frames"] / max(st["graph_frames"], 1) >= 48, "the 64-wide frame graph was not exercised"
    for r, m in zip(res, ms):
        assert r["codes"].shape == (m, 16) and r["codes"].min() >= 0 and r["codes"][:, 0].max() < 2160 and r["codes"][:, 1:].max() < 2048
        assert r["pcm"].size == m * 1920 and np.isfinite(r["pcm"]).all()
    oe = oracle.Engine(os.path.join(full_model, "gguf_q8_0"), None, 16)
    for i in (0, 13, 62):                             # one prompt of each length (27 / 43 / 75 rows)
        oc, _ = oe.generate(prompts[i], max_steps=3, mask_eos=True)
        assert np.array_equal(oc, res[i]["codes"][:3]), i
    oe.close()
    oc2 = oracle.Codec(os.path.join(full_model, "onnx", "q3tts_codec.gguf")); oc2.reset()
    ref = oc2.decode(np.clip(res[40]["codes"][:5], 0, 2047)).copy(); oc2.close()
    assert np.sqrt(np.mean((ref - res[40]["pcm"][: ref.size]) ** 2)) < 1e-4
    # batch invariance at full size: the same request alone gives the same tokens and the same PCM (1e-6: the codec's batched GEMMs tile by rows)
    solo = ge.generate_batch([prompts[7]], max_steps=ms[7], mask_eos=True, want_pcm=True)[0]
    assert np.array_equal(solo["codes"], res[7]["codes"])
    assert np.sqrt(np.mean((solo["pcm"] - res[7]["pcm"]) ** 2)) < 1e-5
    ge.close()


@pytest.fixture(scope="module")
def full_model_bf16(synth_tool, full_model):
    return synth_models.full("bf16", full_model)


def test_fullsize_c5_bf16_clone_batch32_vs_oracle(gpu, oracle, full_model_bf16, vivian):
    """BASELINE config C5 at its real dimensions (engine.rs:243-302 clone path): bf16 weights, 32 slots, 133-row voice-clone prompts (62 reference
    frames + 24 reference-text ids + 32 text ids) over 4 registered voices.  The 32 x 133 = 4 256-row prefill runs k_gemm_float_mfma's >= 96-token
    form at K = 2048 / 6144 and the 32-token steps its narrow form at K = 1024 / 3072.  Three requests (three different voices) against the
    oracle run alone on the host for 3 frames, bit-exact; the same request alone == inside the batch."""
    ge = gpu.Engine(full_model_bf16, "bf16", max_batch=32, max_prompt=256, max_steps=16, load_codec=False)
    voices = []
    for v in range(4):
        vr = np.random.default_rng(1000 + v)
        voices.append(dict(spk=(vivian * (1.0 - 0.1 * v) + 0.01 * vr.standard_normal(2048)).astype(np.float32),
                           codes=vr.integers(0, 2048, 62 * 16).astype(np.int32), text=vr.integers(0, 4000, 24).astype(np.int32)))
    vids = [ge.register_voice(v["spk"], v["codes"], v["text"]) for v in voices]
    texts = [np.random.default_rng(42 + i).integers(0, 4000, 32).astype(np.int32) for i in range(32)]
    prompts = [ge.assets.build_clone(texts[i], voices[i % 4]["codes"], voices[i % 4]["text"], voices[i % 4]["spk"]) for i in range(32)]
    assert prompts[0].shape == (133, 2048)
    ms = [4 + (i % 3) for i in range(32)]
    ids = [ge.submit_text(vids[i % 4], texts[i], lang_id=2055, max_steps=ms[i], temperature=0.0, seed=42) for i in range(32)]
    while ge.sched_step():
        pass
    res = [ge.result(rid) for rid in ids]
    st = ge.stats()
    assert st["slot_frames"] / max(st["graph_frames"], 1) >= 24, "the 32-wide frame graph was not exercised"
    for r, m in zip(res, ms):
        assert r["codes"].shape == (m, 16) and r["codes"].min() >= 0 and r["codes"][:, 0].max() < 2160 and r["codes"][:, 1:].max() < 2048
    oe = oracle.Engine(os.path.join(full_model_bf16, "gguf_bf16"), None, 16)
    for i in (0, 13, 30):                             # voices 0, 1, 2
        oc, _ = oe.generate(prompts[i], max_steps=3, mask_eos=True)
        assert np.array_equal(oc, res[i]["codes"][:3]), i
    oe.close()
    solo = ge.generate_batch([prompts[7]], max_steps=ms[7], mask_eos=True)[0]
    assert np.array_equal(solo["codes"], res[7]["codes"])
    ge.close()


def test_fullsize_codec_group16_vs_oracle(gpu, oracle, full_model):
    """q3tts_decoder_decode_group at full codec size: 16 streams with different histories, two 4-frame chunks each in one pass per
    chunk (the batched extended-buffer GEMMs at G*T rows, split-f16 kernels above 32 rows) vs the oracle stream by stream (1e-4 RMS)."""
    path = os.path.join(full_model, "onnx", "q3tts_codec.gguf")
    gd = gpu.Decoder(path, n_streams=17, max_frames=4, max_group=16)
    rng = np.random.default_rng(21)
    codes = rng.integers(0, 2048, (16, 8, 16))
    streams = [(5 * i + 3) % 17 for i in range(16)]
    assert len(set(streams)) == 16
    for s in streams:
        gd.reset(s)
    got = np.concatenate([gd.decode_group(streams, codes[:, o:o + 4]) for o in (0, 4)], axis=1)
    assert np.isfinite(got).all()
    oc = oracle.Codec(path)
    for i in (0, 6, 15):                              # ~1.5 s of host time per stream
        oc.reset()
        ref = oc.decode(codes[i]).copy()
        assert ref.shape == got[i].shape
        assert np.sqrt(np.mean((ref - got[i]) ** 2)) < 1e-4, i
    oc.close(); gd.close()


def test_fullsize_codec_fallback_epilogues_match_the_16_byte_ones(gpu, full_model, tmp_path):
    """The split-f16 GEMMs finish their tiles through LDS with 16-byte accesses (k_conv_gemm_h3<.., EPL = 1>, k_conv_gemm_h<.., 1>, k_splitk_reduce4) whenever
    strides and pointers allow -- always, for this decoder -- so the four-byte fallback instantiations would otherwise never run.  A child process with
    Q3_CODEC_H3_EPL=0 Q3_CODEC_EPL4=0 decodes the same 16-stream pass; same arithmetic per element, so the waveforms must be IDENTICAL (also checks the
    pre-split operand form, Q3_CODEC_PRESPLIT=1, against the default within the 1e-6 its re-association allows)."""
    import sys
    path = os.path.join(full_model, "onnx", "q3tts_codec.gguf")
    rng = np.random.default_rng(77)
    codes = rng.integers(0, 2048, (16, 4, 16))
    np.save(os.path.join(str(tmp_path), "codes.npy"), codes)
    child = (
        "import sys, numpy as np\n"
        "sys.path.insert(0, %r)\n"
        "import q3tts as Q\n"
        "codes = np.load(sys.argv[1])\n"
        "gd = Q.Decoder(%r, n_streams=16, max_frames=4, max_group=16)\n"
        "[gd.reset(s) for s in range(16)]\n"
        "np.save(sys.argv[2], gd.decode_group(list(range(16)), codes)); gd.close()\n"
    ) % (os.path.join(ROOT, "qwen3-tts-rust_amd", "python"), path)
    outs = {}
    for name, env in (("default", {}), ("scalar", {"Q3_CODEC_H3_EPL": "0", "Q3_CODEC_EPL4": "0"}), ("presplit", {"Q3_CODEC_PRESPLIT": "1"})):
        out = os.path.join(str(tmp_path), name + ".npy")
        e = dict(os.environ); e.update(env)
        r = subprocess.run([sys.executable, "-c", child, os.path.join(str(tmp_path), "codes.npy"), out], env=e, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs[name] = np.load(out)
    assert outs["default"].shape == (16, 4 * 1920) and np.isfinite(outs["default"]).all() and np.abs(outs["default"]).max() > 1e-3
    assert np.array_equal(outs["default"], outs["scalar"])
    assert np.sqrt(np.mean((outs["default"] - outs["presplit"]) ** 2)) < 1e-6


@pytest.fixture(scope="module")
def full_model_q5(synth_tool, full_model):
    return synth_models.full("q5_k_m", full_model)


def test_fullsize_q5_k_m_packed_planes_vs_oracle(gpu, oracle, full_model_q5, vivian):
    """Q5_K_M at the real dimensions (BASELINE configs[0] quantisation): the K-quant rows stay packed in HBM (nibble + bit planes) and every
    kernel body that unpacks them -- fused B = 1 path (k_gemv_q8_norm / k_gateup_swiglu / k_gemv_kq for Q5_K, Q6_K and the mixed q,k,v
    matrix) at K = 2048 / 6144 (talker) and 1024 / 3072 (predictor, two super-segments), then a 20-slot batch through the matrix-core K-quant GEMM and a 12-slot batch through the z-tiled GEMV --
    must reproduce the oracle's Q5_K / Q6_K block arithmetic bit for bit."""
    ge = gpu.Engine(full_model_q5, "q5_k_m", max_batch=20, max_steps=16, load_codec=False)
    b5 = ge.bytes_per_step(1, 16)
    prompts = []
    for i in range(20):
        rng = np.random.default_rng(900 + i)
        prompts.append(ge.assets.build_core(rng.integers(0, 4000, 3 + (i % 2)).astype(np.int32), lang_id=2055, spk_emb=vivian))
    single = ge.generate_batch([prompts[0]], max_steps=4, mask_eos=True)[0]["codes"]
    oe = oracle.Engine(os.path.join(full_model_q5, "gguf_q5_k_m"), None, 8)
    oc, _ = oe.generate(prompts[0], max_steps=4, mask_eos=True)
    assert np.array_equal(oc, single)
    res = ge.generate_batch(prompts, max_steps=3, mask_eos=True)   # 20 slots: the K-quant matrix-core GEMM (k_gemm_kq_mfma) at K = 1024 ... 6144
    assert np.array_equal(res[0]["codes"], single[:3])
    for i in (5, 17):
        oci, _ = oe.generate(prompts[i], max_steps=3, mask_eos=True)
        assert np.array_equal(oci, res[i]["codes"]), i
    oe.close()
    res12 = ge.generate_batch(prompts[:12], max_steps=3, mask_eos=True)   # 12 slots: the z-tiled GEMV form of the same arithmetic
    for i in range(12):
        assert np.array_equal(res12[i]["codes"], res[i]["codes"]), i
    ge.close()
    # packed planes: 0.75 / 0.875 B per weight with scales and metadata against Q8_0's 1.0625 (int8 planes were 1.19)
    g8 = gpu.Engine(full_model_q5, "q8_0", max_batch=1, max_steps=16, load_codec=False)
    b8 = g8.bytes_per_step(1, 16)
    g8.close()
    assert b5 < 0.85 * b8, (b5, b8)


def test_fullsize_ggml_mode_engine_matches_oracle(gpu, oracle, full_model, vivian):
    """Q3_SPEC=ggml at the real dimensions (K = 2048 / 6144 talker, 1024 / 3072 predictor; 28 + 5 layers): the device's ggml-arithmetic path
    (csrc/ggml_mode.hip) against oracle/q3o_ggml.c, codec tokens bit for bit -- SURVEY 8f row f-1, /root/reference/src/models/llama/mod.rs:442-451."""
    old = os.environ.get("Q3_SPEC")
    try:
        os.environ["Q3_SPEC"] = "ggml"
        oracle.set_arith_mode(1)
        ge = gpu.Engine(full_model, "q8_0", max_batch=2, max_steps=16, load_codec=False)
        rng = np.random.default_rng(321)
        prompts = [ge.assets.build_core(rng.integers(0, 4000, 3 + i).astype(np.int32), lang_id=2055, spk_emb=vivian) for i in range(2)]
        res = ge.generate_batch(prompts, max_steps=[3, 2], mask_eos=True)
        ge.close()
        oe = oracle.Engine(os.path.join(full_model, "gguf_q8_0"), None, 16)
        for p, r, m in zip(prompts, res, (3, 2)):
            oc, _ = oe.generate(p, max_steps=m, mask_eos=True)
            assert np.array_equal(oc, r["codes"])
        oe.close()
    finally:
        oracle.set_arith_mode(0)
        if old is None:
            os.environ.pop("Q3_SPEC", None)
        else:
            os.environ["Q3_SPEC"] = old
