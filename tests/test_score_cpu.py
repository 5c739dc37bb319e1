"""[EXT] scoring given frames, CPU half (include/q3tts_spec.h "scoring"): the entry points are declared, exported, listed and fail cleanly
without an engine or a device; every refusal of include/q3tts.h is reached through the pure rule of csrc/sched_logic.h (built with plain g++ and
host sanitizers, like the other rule drivers); the same driver checks which rows of a prefill chunk get the talker head for a score request
that spans one, two and three chunks; and tests/score_ref.py -- the reference of tests/test_gpu_score.py -- gives exactly the rows of
tests/logprob_ref.py::generate for the codes that run produced (the same f32 logits, the same float64 formula).  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import logprob_ref as LR
import score_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("q3tts_submit_score", "q3tts_group_submit_score", "q3tts_engine_score_width", "q3tts_op_score_rows", "q3tts_op_score_inputs")
SAMPLE_END, CODEC_EOS = 2160, 2150


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_names_are_declared_exported_and_listed(q3):
    txt = _header("q3tts.h")
    tail = (r"\s*const\s+float\s*\*\s*prompt\s*,\s*int32_t\s+n_prompt\s*,\s*const\s+int32_t\s*\*\s*trail_ids\s*,\s*int32_t\s+n_trail\s*,"
            r"\s*const\s+int32_t\s*\*\s*codes\s*,\s*int32_t\s+n\s*,\s*int64_t\s*\*\s*req_id\s*\)\s*;")
    assert re.search(r"\bint\s+q3tts_submit_score\s*\(\s*q3tts_engine\s*\*\s*\w+\s*," + tail, txt)
    assert re.search(r"\bint\s+q3tts_group_submit_score\s*\(\s*q3tts_group\s*\*\s*\w+\s*,\s*int32_t\s+engine_index\s*," + tail, txt)
    assert re.search(r"\bint32_t\s+q3tts_engine_score_width\s*\(\s*q3tts_engine\s*\*\s*\w+\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_op_score_rows\s*\(\s*const\s+float\s*\*\s*tlogits\s*,\s*int32_t\s+t_stride\s*,\s*const\s+float\s*\*\s*plogits\s*,"
                     r"\s*const\s+int32_t\s*\*\s*codes\s*,\s*int32_t\s+F\s*,\s*float\s*\*\s*out\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_op_score_inputs\s*\(\s*const\s+float\s*\*\s*hidden_proj\s*,\s*const\s+float\s*\*\s*const\s*\*\s*tabs\s*,"
                     r"\s*const\s+int64_t\s*\*\s*tab_rows\s*,\s*int32_t\s+dP\s*,\s*const\s+int32_t\s*\*\s*codes\s*,\s*int32_t\s+F\s*,\s*float\s*\*\s*out\s*\)\s*;", txt)
    for n in NEW:
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n) and getattr(q3.lib(), n).argtypes, n
    raw = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    sec = raw[raw.index("scoring given frames [EXT]"):]
    assert "n_prompt - 1 + f" in sec and "teacher-forced" in sec and "1e-5 * max(1, |lp64|)" in sec


def test_python_surface(q3):
    assert callable(q3.Engine.submit_score) and callable(q3.Engine.score_width) and callable(q3.group_submit_score)
    assert callable(q3.op_score_rows) and callable(q3.op_score_inputs)


def test_entry_points_fail_cleanly_without_an_engine_or_a_device(q3):
    L = q3.lib()
    prompt, codes, rid = np.zeros((3, 2048), np.float32), np.zeros((2, 16), np.int32), C.c_int64(-5)
    assert L.q3tts_submit_score(None, q3._p(prompt), 3, None, 0, q3._p(codes), 2, C.byref(rid)) < 0 and L.q3tts_last_error()
    assert L.q3tts_group_submit_score(None, -1, q3._p(prompt), 3, None, 0, q3._p(codes), 2, C.byref(rid)) < 0 and L.q3tts_last_error()
    assert rid.value == -5
    assert L.q3tts_engine_score_width(None) == -1
    tl, pl, out = np.zeros((2, 2176), np.float32), np.zeros((15, 2, 2048), np.float32), np.full((2, 17), 7.0, np.float32)
    hp, tab, rows, outi = np.zeros((2, 16), np.float32), np.zeros((4, 16), np.float32), np.full(15, 4, np.int64), np.full((32, 16), 7.0, np.float32)
    ptrs = (C.c_void_p * 15)(*[tab.ctypes.data] * 15)
    if q3.device_count() == 0:
        assert L.q3tts_op_score_rows(q3._p(tl), 2176, q3._p(pl), q3._p(codes), 2, q3._p(out)) < 0 and b"no HIP device" in L.q3tts_last_error()
        assert L.q3tts_op_score_inputs(q3._p(hp), ptrs, q3._p(rows), 16, q3._p(codes), 2, q3._p(outi)) < 0 and b"no HIP device" in L.q3tts_last_error()
        with pytest.raises(q3.Q3Error, match="no HIP device"):
            q3.op_score_rows(tl, pl, codes)
    for args in ((None, 2176, q3._p(pl), q3._p(codes), 2, q3._p(out)), (q3._p(tl), 2176, None, q3._p(codes), 2, q3._p(out)),
                 (q3._p(tl), 2176, q3._p(pl), None, 2, q3._p(out)), (q3._p(tl), 2176, q3._p(pl), q3._p(codes), 0, q3._p(out)),
                 (q3._p(tl), 2159, q3._p(pl), q3._p(codes), 2, q3._p(out)), (q3._p(tl), 2176, q3._p(pl), q3._p(codes), 2, None)):
        assert L.q3tts_op_score_rows(*args) < 0 and L.q3tts_last_error()
    for args in ((None, ptrs, q3._p(rows), 16, q3._p(codes), 2, q3._p(outi)), (q3._p(hp), None, q3._p(rows), 16, q3._p(codes), 2, q3._p(outi)),
                 (q3._p(hp), ptrs, None, 16, q3._p(codes), 2, q3._p(outi)), (q3._p(hp), ptrs, q3._p(rows), 18, q3._p(codes), 2, q3._p(outi)),
                 (q3._p(hp), ptrs, q3._p(rows), 16, None, 2, q3._p(outi)), (q3._p(hp), ptrs, q3._p(rows), 16, q3._p(codes), 0, q3._p(outi))):
        assert L.q3tts_op_score_inputs(*args) < 0 and L.q3tts_last_error()
    assert np.all(out == 7.0) and np.all(outi == 7.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("score_logic") / "score_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "score_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _refusal(driver, n_prompt=5, max_prompt=32, n_trail=0, n=2, max_steps=8, kv_rows=64, ggml=0, codes=None, null_prompt=0, null_trail=0, null_codes=0):
    codes = np.arange(1, 1 + 16 * max(n, 0), dtype=np.int64) % 2048 if codes is None else np.asarray(codes).reshape(-1)
    return driver("refusal %d %d %d %d %d %d %d %d %d %d %d %s\n" % (null_prompt, n_prompt, max_prompt, null_trail, n_trail, null_codes, n, max_steps,
                                                                    kv_rows, ggml, codes.size, " ".join(str(int(c)) for c in codes)))[0]


def test_every_refusal(driver):
    assert _refusal(driver) == "ok"
    assert _refusal(driver, n=8) == "ok"                                 # n = max_steps: nothing is generated, so the whole budget may be given
    assert _refusal(driver, n=1, n_prompt=1) == "ok"
    assert _refusal(driver, n_trail=32, n=2) == "ok"                     # a trail may be longer or shorter than the frames
    assert "n must be >= 1" in _refusal(driver, n=0)
    assert "n must be >= 1" in _refusal(driver, n=-3)
    assert "max_steps" in _refusal(driver, n=9)
    assert "codes missing" in _refusal(driver, null_codes=1)
    assert "prompt missing" in _refusal(driver, null_prompt=1)
    assert "prompt length" in _refusal(driver, n_prompt=0)
    assert "prompt length" in _refusal(driver, n_prompt=33)
    assert "n_trail" in _refusal(driver, n_trail=-1)
    assert "n_trail" in _refusal(driver, n_trail=33)
    assert "trailing ids missing" in _refusal(driver, n_trail=2, null_trail=1)
    assert _refusal(driver, n_trail=0, null_trail=1) == "ok"
    assert _refusal(driver, n_prompt=32, n=8, kv_rows=40) == "ok"         # exactly the capacity
    assert "KV capacity" in _refusal(driver, n_prompt=32, n=8, kv_rows=39)
    assert "Q3_SPEC=ggml" in _refusal(driver, ggml=1)
    good = np.arange(32) % 2048
    for at, bad, why in ((0, -1, "code_0"), (16, SAMPLE_END, "code_0"), (16, CODEC_EOS, "EOS"), (1, -1, "residual"), (31, 2048, "residual"), (15, 4000, "residual")):
        c = good.copy()
        c[at] = bad
        assert why in _refusal(driver, codes=c), (at, bad)
    c = good.copy()
    c[0], c[16], c[15], c[17] = SAMPLE_END - 1, 0, 2047, 0                # the edges of both ranges are fine (2150 aside)
    assert _refusal(driver, codes=c) == "ok"


def test_chunk_rows_that_get_the_head(driver):
    # one chunk: 5 prompt rows and 4 frames -> rows 4..7 of an 8-row stream (the last frame's feedback row is not prefilled)
    assert driver("runs 16 1\n5 4 1\n") == ["chunk 8: 0:4:0:4"]
    # a single frame: the last prompt row alone
    assert driver("runs 16 1\n5 1 1\n") == ["chunk 5: 0:4:0:1"]
    # two chunks, the boundary inside the frames: 6 + 7 - 1 = 12 rows in chunks of 8
    assert driver("runs 8 1\n6 7 1\n") == ["chunk 8: 0:5:0:3", "chunk 4: 0:0:3:4"]
    # two chunks, the boundary right behind the last prompt row's predecessor: the first chunk ends with frame 0's row
    assert driver("runs 6 1\n6 3 1\n") == ["chunk 6: 0:5:0:1", "chunk 2: 0:0:1:2"]
    # three chunks with the prompt alone in the first
    assert driver("runs 4 1\n5 6 1\n") == ["chunk 4:", "chunk 4: 0:0:0:4", "chunk 2: 0:0:4:2"]
    # beside other requests: a generation request (3 rows), a resumed one (3 + 2 rows) and two score requests share the chunks
    assert driver("runs 8 4\n3 0 0\n2 3 1\n3 2 0\n2 12 1\n") == ["chunk 8: 1:4:0:3", "chunk 8: 3:5:0:3", "chunk 8: 3:0:3:8", "chunk 1: 3:0:11:1"]


@pytest.fixture(scope="module")
def tiny_oracle(oracle, tiny_model, q3):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), None, 4)
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    yield oe, a.tts_pad()
    a.close()
    oe.close()


@pytest.mark.parametrize("name,kw,seed", [("greedy", {}, 42),
                                          ("sampled", dict(temperature=0.9, top_k=50, top_p=1.0, repetition_penalty=1.05, predictor_temperature=0.9,
                                                           predictor_top_k=50, predictor_top_p=0.8), 44)])
def test_score_of_generated_codes_is_the_generation_record(tiny_oracle, vivian, name, kw, seed):
    oe, pad = tiny_oracle
    rng = np.random.default_rng(seed)
    prompt = oe.assets.build_core(rng.integers(0, 4000, 7).astype(np.int32), lang_id=2055, spk_emb=vivian)
    codes, lp = LR.generate(oe, pad, prompt, 6, seed=seed, mask_eos=True, **kw)
    assert codes.shape == (6, 16)
    got = SR.score(oe, pad, prompt, codes)
    assert np.array_equal(got, lp)                                       # exactly: the same f32 logits through the same float64 formula
    assert np.array_equal(SR.score(oe, pad, prompt, codes[:3]), lp[:3])  # a row depends on the frames before it alone


def test_off_policy_codes_give_finite_rows(tiny_oracle, vivian):
    oe, pad = tiny_oracle
    rng = np.random.default_rng(7)
    prompt = oe.assets.build_core(rng.integers(0, 4000, 6).astype(np.int32), lang_id=2055, spk_emb=vivian)
    codes = rng.integers(0, 2048, (5, 16)).astype(np.int32)
    lp = SR.score(oe, pad, prompt, codes, trail=[17, 400])
    assert lp.shape == (5, 17) and np.all(np.isfinite(lp)) and np.all(lp <= 0.0)
    plain = SR.score(oe, pad, prompt, codes)
    assert np.array_equal(lp[0], plain[0]) and not np.array_equal(lp[1:], plain[1:])   # the ids enter with frame 0's feedback row
