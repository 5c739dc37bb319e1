"""[EXT] streaming-text talker input, CPU half: q3tts_prompt_build_streaming against the reference-layout builders (through the
q3tts_assets_* rows), the Python restatement (tests/text_stream_ref.py) against gen_loop_ref at n_trail = 0, and the feedback kernel's
streaming variant against a scratch-free gfx950 code object.  No GPU is used."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gen_loop_ref
import text_stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TEXT_BOS, TEXT_EOS, CODEC_PAD, CODEC_BOS = 151672, 151673, 2148, 2149


@pytest.fixture(scope="module")
def assets(q3, tiny_model):
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    yield a
    a.close()


def _check_layout(a, full, stream, trail, text):
    n = len(text)
    assert stream.shape[0] == full.shape[0] - (n + 1)     # n text rows + [EOS + PAD] of the reference layout, and its [marker + BOS] row
    k = stream.shape[0] - 1                               # the prefix ends with [text(BOS) + E0(PAD)]
    assert np.array_equal(stream[:k], full[:k])
    bos_pad = a.text_embedding(TEXT_BOS) + a.codec_embedding(0, CODEC_PAD)
    assert np.array_equal(stream[k - 1], bos_pad)
    assert np.array_equal(stream[k], a.text_embedding(int(text[0])) + a.codec_embedding(0, CODEC_BOS))
    assert list(trail) == [int(t) for t in text[1:]] + [TEXT_EOS]


@pytest.mark.parametrize("n_text", [1, 2, 9])
def test_streaming_prompt_preset_voice(assets, vivian, n_text):
    rng = np.random.default_rng(n_text)
    text = rng.integers(0, 4000, n_text).astype(np.int32)
    text[-1] = 5000                                       # out of the 4096-row table: the fallback row in the prompt / trail
    for kw in (dict(lang_id=2055, spk_emb=vivian), dict(lang_id=None, spk_id=3000), dict(lang_id=2058, spk_emb=vivian, instr_ids=[7, 8, 9])):
        full = assets.build_core(text, **kw)
        stream, trail = assets.prompt_build_streaming(text, **kw)
        _check_layout(assets, full, stream, trail, text)


def test_streaming_prompt_clone_voice(assets, vivian):
    rng = np.random.default_rng(4)
    text = rng.integers(0, 4000, 6).astype(np.int32)
    ref_codes = rng.integers(0, 2048, (5, 16)).astype(np.int32)
    ref_text = rng.integers(0, 4000, 4).astype(np.int32)
    for ins in (None, [11, 12]):
        full = assets.build_clone(text, ref_codes, ref_text, vivian, lang_id=2055, instr_ids=ins)
        stream, trail = assets.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian, instr_ids=ins, ref_codes=ref_codes, ref_text_ids=ref_text)
        _check_layout(assets, full, stream, trail, text)


def test_streaming_prompt_rejects_empty_text(q3, assets, vivian):
    with pytest.raises(q3.Q3Error, match="n_text >= 1"):
        assets.prompt_build_streaming(np.zeros(0, np.int32), spk_emb=vivian)


@pytest.fixture(scope="module")
def tiny_oracle(oracle, tiny_model, q3):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    pad = a.tts_pad()
    for tok in (0, 17, 4095, 4096, 5000, TEXT_EOS, -3):     # the restatement's text rows are the product host's, fallback included
        assert np.array_equal(oe.assets.text_embedding(tok).view(np.uint32), a.text_embedding(tok).view(np.uint32)), tok
    a.close()
    yield oe, pad
    oe.close()


@pytest.mark.parametrize("temperature", [0.0, 0.7])
def test_restatement_without_trail_is_gen_loop_ref(tiny_oracle, vivian, temperature):
    oe, pad = tiny_oracle
    prompt = oe.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    for kw in ({}, dict(repetition_penalty=1.3, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)):
        want = gen_loop_ref.generate(oe, pad, prompt, 14, temperature, 40, 0.9, 9, True, **kw)
        got = text_stream_ref.generate(oe, pad, prompt, 14, (), temperature, 40, 0.9, 9, True, **kw)
        assert np.array_equal(got, want)


def test_restatement_trail_changes_the_trajectory(q3, tiny_oracle, vivian, tiny_model):
    oe, pad = tiny_oracle
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    text = np.arange(100, 108, dtype=np.int32)
    prompt, trail = a.prompt_build_streaming(text, lang_id=2055, spk_emb=vivian)
    a.close()
    base = text_stream_ref.generate(oe, pad, prompt, 12, ())
    got = text_stream_ref.generate(oe, pad, prompt, 12, trail)
    assert base.shape == got.shape == (12, 16)
    assert np.array_equal(got[0], base[0])                # frame 0's codes come from the prefill and its first predictor pass
    assert not np.array_equal(got, base)
    # the trailing row of frame f enters the feedback of frame f: a trail that differs only from row 3 on leaves frames 0..3 alone
    alt = list(trail[:3]) + [int(t) + 1 for t in trail[3:]]
    got2 = text_stream_ref.generate(oe, pad, prompt, 12, alt)
    assert np.array_equal(got2[:4], got[:4]) and not np.array_equal(got2, got)


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_feedback_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "fused.s"
    flags = ["-mllvm", "-amdgpu-kernarg-preload-count=16", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S", "-x", "hip"]
    subprocess.run([HIPCC] + flags + [os.path.join(ROOT, "qwen3-tts-rust_amd", "csrc", "kernels_fused.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "k_feedback_keys" in name:
            seen[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert len(seen) == 2 and set(seen.values()) == {0}, seen
    assert any("Lb1E" in n for n in seen) and any("Lb0E" in n for n in seen), seen
