"""[EXT] generation controls (q3tts_gen_options), CPU half: the Python restatement of the oracle loop (tests/gen_loop_ref.py) is anchored
to q3oracle.Engine.generate, its penalty formula to transformers' RepetitionPenaltyLogitsProcessor, the ctypes mirror to the C header, and
the sampler kernels to a scratch-free gfx950 code object.  No GPU is used."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gen_loop_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def tiny_oracle(oracle, tiny_model, q3):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    pad = a.tts_pad()
    a.close()
    yield oe, pad
    oe.close()


@pytest.mark.parametrize("temperature,top_k,top_p", [(0.0, 40, 0.9), (0.7, 40, 0.9)])
@pytest.mark.parametrize("mask_eos", [True, False])
def test_restatement_matches_oracle_engine_at_defaults(tiny_oracle, vivian, temperature, top_k, top_p, mask_eos):
    oe, pad = tiny_oracle
    rng = np.random.default_rng(21)
    for n_text, steps, seed in ((6, 9, 5), (23, 14, 77)):
        prompt = oe.assets.build_core(rng.integers(0, 4000, n_text).astype(np.int32), lang_id=2055, spk_emb=vivian)
        oc, _ = oe.generate(prompt, max_steps=steps, temperature=temperature, top_k=top_k, top_p=top_p, seed=seed, mask_eos=mask_eos)
        rc = gen_loop_ref.generate(oe, pad, prompt, steps, temperature, top_k, top_p, seed, mask_eos)
        assert np.array_equal(oc, rc), (n_text, steps)


def test_restatement_options_change_the_trajectory(tiny_oracle, vivian):
    """the new controls are live in the restatement (a no-op there would make every GPU comparison vacuous)"""
    oe, pad = tiny_oracle
    prompt = oe.assets.build_core(np.arange(100, 108, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    base = gen_loop_ref.generate(oe, pad, prompt, 24)
    pen = gen_loop_ref.generate(oe, pad, prompt, 24, repetition_penalty=1.3)     # greedy: code_0 1139 repeats at frame 13 without it
    pred = gen_loop_ref.generate(oe, pad, prompt, 24, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
    assert not np.array_equal(base, pen) and not np.array_equal(base, pred)
    # the teacher-forced replay reproduces the oracle's own PCM for its own codes
    oc, opcm = oe.generate(prompt, max_steps=12, want_pcm=True)
    assert np.array_equal(gen_loop_ref.replay_pcm(oe, prompt, oc), opcm)


def test_penalty_matches_transformers_processor():
    torch = pytest.importorskip("torch")
    tlp = pytest.importorskip("transformers.generation.logits_process")
    rng = np.random.default_rng(5)
    for p in (1.05, 1.3, 0.8, 2.0):
        lg = (rng.standard_normal(2160) * 4).astype(np.float32)
        lg[[3, 9, 17]] = 0.0
        lg[[5]] = -0.0
        lg[[11]] = np.inf
        lg[[13]] = -np.inf
        lg[100:110] = rng.standard_normal(10).astype(np.float32) * 1e-30   # subnormal range
        hist = [3, 5, 9, 11, 13, 17, 3, 3, 42, 42, 2047, 100, 101, 105] + list(rng.integers(0, 2160, 200))
        ref = tlp.RepetitionPenaltyLogitsProcessor(p)(torch.tensor([hist]), torch.from_numpy(lg.copy())[None])[0].numpy()
        got = gen_loop_ref.penalise(lg, hist, p)
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), p


def test_gen_options_layout_and_defaults(q3, tmp_path):
    src = tmp_path / "lay.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "q3tts.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu\\n", sizeof(q3tts_gen_options), offsetof(q3tts_gen_options, repetition_penalty),'
                   ' offsetof(q3tts_gen_options, predictor_temperature), offsetof(q3tts_gen_options, predictor_top_k),'
                   ' offsetof(q3tts_gen_options, predictor_top_p)); return 0; }\n')
    exe = tmp_path / "lay"
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    G = q3.GenOptions
    assert got == [q3.C.sizeof(G)] + [getattr(G, f).offset for f, _ in G._fields_]
    o = G(0.0, 5.0, 7, 0.1)
    q3.lib().q3tts_gen_options_default(q3.C.byref(o))
    assert (o.repetition_penalty, o.predictor_temperature, o.predictor_top_k, o.predictor_top_p) == (1.0, 0.0, 0, 1.0)
    assert {f: getattr(o, f) for f, _ in G._fields_} == q3.GEN_DEFAULTS
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    assert int(re.search(r"#define Q3_PRED_SEED_XOR (0x[0-9A-Fa-f]+)ull", spec).group(1), 16) == gen_loop_ref.PRED_SEED_XOR


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_sampler_kernels_use_no_scratch(tmp_path):
    out = tmp_path / "sampler.s"
    flags = ["-mllvm", "-amdgpu-kernarg-preload-count=16", "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math",
             "-fhip-fp32-correctly-rounded-divide-sqrt", "--cuda-device-only", "-S", "-x", "hip"]
    subprocess.run([HIPCC] + flags + [os.path.join(ROOT, "qwen3-tts-rust_amd", "csrc", "sampler.hip"), "-o", str(out)], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    text = out.read_text()
    meta = text[text.index("amdhsa.kernels"):]
    seen = {}
    for blk in meta.split("  - .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        seen[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert seen.get("_ZN2q313k_sample_predENS_10SampleArgsE") == 0, seen
    assert seen.get("_ZN2q38k_sampleENS_10SampleArgsE") == 0, seen
