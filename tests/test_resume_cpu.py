"""[EXT] resume (q3tts_submit_resume), CPU half: the declarations and the Python surface are there, the entry points fail cleanly without an
engine or a device, every refusal of include/q3tts.h is reached through the pure rule of csrc/sched_logic.h (built with plain g++, like the
cancel rules), the prefill packer routes a prefix behind its prompt, the numpy restatement of the feedback row (tests/resume_ref.py) equals
the host assets' own arithmetic, and resume() composed from the oracle restatements equals the uninterrupted restatement at every split
point -- greedy, sampled and sampled with the generation options, with and without trailing text.  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import gen_loop_ref
import resume_ref
import text_stream_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPSTREAM = dict(repetition_penalty=1.05, predictor_temperature=0.9, predictor_top_k=50, predictor_top_p=0.8)
SAMPLED = dict(temperature=0.9, top_k=50, top_p=1.0)
SAMPLE_END, CODEC_EOS = 2160, 2150


def test_names_are_declared_exported_and_listed(q3):
    raw = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    tail = (r"const\s+q3tts_request\s*\*\s*\w+\s*,\s*int32_t\s+want_pcm\s*,\s*const\s+q3tts_gen_options\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*trail_ids\s*,"
            r"\s*int32_t\s+n_trail\s*,\s*int32_t\s+open\s*,\s*const\s+int32_t\s*\*\s*prefix_codes\s*,\s*int32_t\s+n_prefix\s*,\s*int64_t\s*\*\s*req_id\s*\)\s*;")
    assert re.search(r"\bint\s+q3tts_submit_resume\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*" + tail, txt)
    assert re.search(r"\bint\s+q3tts_group_submit_resume\s*\(\s*q3tts_group\s*\*\s*\w+\s*,\s*int32_t\s+engine_index\s*,\s*" + tail, txt)
    assert re.search(r"\bint\s+q3tts_op_feedback_rows\s*\(\s*const\s+q3tts_assets\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*codes\s*,\s*int32_t\s+n\s*,"
                     r"\s*const\s+int32_t\s*\*\s*trail_ids\s*,\s*int32_t\s+n_trail\s*,\s*float\s*\*\s*rows\s*\)\s*;", txt)
    for n in ("q3tts_submit_resume", "q3tts_group_submit_resume", "q3tts_op_feedback_rows"):
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n) and getattr(q3.lib(), n).argtypes, n
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    assert re.search(r"resume \[EXT\] \(q3tts_submit_resume", spec)


def test_python_surface(q3):
    import inspect
    assert inspect.signature(q3.Engine.submit).parameters["prefix_codes"].default is None
    assert callable(q3.op_feedback_rows)


def test_fails_cleanly_without_an_engine_or_a_device(q3, tiny_model):
    L = q3.lib()
    r, rid = q3.Request(), C.c_int64(-7)
    codes = np.zeros(16, np.int32)
    assert L.q3tts_submit_resume(None, C.byref(r), 0, None, None, 0, 0, q3._p(codes), 1, C.byref(rid)) < 0 and L.q3tts_last_error()
    assert L.q3tts_group_submit_resume(None, -1, C.byref(r), 0, None, None, 0, 0, q3._p(codes), 1, C.byref(rid)) < 0 and L.q3tts_last_error()
    assert rid.value == -7
    rows = np.zeros((1, 2048), np.float32)
    assert L.q3tts_op_feedback_rows(None, q3._p(codes), 1, None, 0, q3._p(rows)) < 0 and L.q3tts_last_error()
    if q3.device_count() > 0:
        return   # on the GPU box the no-device path cannot be observed
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    try:
        assert L.q3tts_op_feedback_rows(a.h, q3._p(codes), 1, None, 0, q3._p(rows)) < 0
        assert b"no HIP device" in L.q3tts_last_error()
        with pytest.raises(q3.Q3Error):
            q3.op_feedback_rows(a, codes)
    finally:
        a.close()


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("resume_logic") / "resume_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "resume_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _refusal(driver, n_prompt=10, max_steps=40, n_prefix=3, null_codes=0, open_=0, n_trail=0, kv_rows=1088, codes=None):
    if codes is None:
        codes = np.tile(np.arange(16, dtype=np.int32) + 5, (max(n_prefix, 0), 1))
    codes = np.asarray(codes, np.int32).reshape(-1)
    return driver("refusal %d %d %d %d %d %d %d %d %s\n" % (n_prompt, max_steps, n_prefix, null_codes, open_, n_trail, kv_rows, codes.size,
                                                           " ".join(str(int(c)) for c in codes)))[0]


def test_every_refusal(driver):
    good = np.tile(np.arange(16, dtype=np.int32) + 5, (3, 1))
    assert _refusal(driver) == "ok"
    assert _refusal(driver, n_prefix=0, null_codes=1) == "ok"                       # the plain submission
    assert _refusal(driver, n_prefix=39) == "ok" and _refusal(driver, n_prefix=1, max_steps=2) == "ok"
    assert "n_prefix must be >= 0" in _refusal(driver, n_prefix=-1)
    assert "below max_steps" in _refusal(driver, n_prefix=40) and "below max_steps" in _refusal(driver, n_prefix=41)
    assert "below max_steps" in _refusal(driver, n_prefix=1, max_steps=1) and "below max_steps" in _refusal(driver, n_prefix=1, max_steps=0)
    assert "codes missing" in _refusal(driver, null_codes=1)
    for bad in (-1, SAMPLE_END, SAMPLE_END + 5, 1 << 30):
        c = good.copy(); c[1, 0] = bad
        assert "code_0 lies outside" in _refusal(driver, codes=c), bad
    c = good.copy(); c[2, 0] = CODEC_EOS
    assert "EOS" in _refusal(driver, codes=c)
    for ok0 in (0, 2047, 2048, CODEC_EOS - 1, CODEC_EOS + 1, SAMPLE_END - 1):           # the talker's whole sampling range but EOS
        c = good.copy(); c[0, 0] = ok0
        assert _refusal(driver, codes=c) == "ok", ok0
    for q in (1, 7, 15):
        for bad in (-1, 2048, 2150):
            c = good.copy(); c[2, q] = bad
            assert "residual code" in _refusal(driver, codes=c), (q, bad)
        for edge in (0, 2047):
            c = good.copy(); c[0, q] = edge
            assert _refusal(driver, codes=c) == "ok"
    assert "open trail" in _refusal(driver, open_=1, n_trail=2)
    assert _refusal(driver, open_=1, n_trail=3) == "ok" and _refusal(driver, open_=0, n_trail=2) == "ok"   # a closed trail may be shorter
    # positions 0 .. n_prompt + n_prefix (the first generated frame's row) must fit the slot's pages
    assert _refusal(driver, n_prompt=60, n_prefix=3, kv_rows=64) == "ok"
    assert "KV capacity" in _refusal(driver, n_prompt=61, n_prefix=3, kv_rows=64)
    assert "KV capacity" in _refusal(driver, n_prompt=1024, n_prefix=39, max_steps=512, kv_rows=1024)


def test_packer_routes_the_prefix_behind_its_prompt(driver):
    # request 0: 3 prompt rows + 4 prefix frames on slot 2; request 1: 2 prompt rows, no prefix, slot 0; request 2: 1 + 2 on slot 1; chunks of 5
    out = driver("pack 5 3  3 2 4  2 0 0  1 1 2\n")
    assert out == [
        "chunk 5", "seq 2 2 2 2 2", "slot 0 1 2 3 4", "pos 0 0 0 0 1 1 1 0 2 2 2 0 3 3 3 0 4 4 4 0", "lasts", "fb 0:3:0:2", "staged 0+3",
        "stage 0 1 2 -1 -1",
        "chunk 5", "seq 2 2 0 0 1", "slot 5 6 0 1 0", "pos 5 5 5 0 6 6 6 0 0 0 0 0 1 1 1 0 0 0 0 0", "lasts 0:1 1:3", "fb 0:0:2:2", "staged 2+3",
        "stage -1 -1 100 101 200",
        "chunk 2", "seq 1 1", "slot 1 2", "pos 1 1 1 0 2 2 2 0", "lasts 2:1", "fb 2:0:0:2", "staged",
        "stage -1 -1 -1 -1 -1"]
    # without a prefix the chunk is what it was
    assert driver("pack 4 2  3 1 0  2 0 0\n")[:8] == ["chunk 4", "seq 1 1 1 0", "slot 0 1 2 0", "pos 0 0 0 0 1 1 1 0 2 2 2 0 0 0 0 0", "lasts 0:2", "fb",
                                                   "staged 0+4", "stage 0 1 2 100"]
    # the slot of a resumed request starts at frame k, position n_prompt + k in the three running streams
    assert driver("load 17 5\nload 9 0\n") == ["5 22 22 22 22 0", "0 9 9 9 9 0"]


@pytest.fixture(scope="module")
def tiny_oracle(oracle, tiny_model, q3):
    oe = oracle.Engine(os.path.join(tiny_model, "gguf_q8_0"), os.path.join(tiny_model, "onnx", "q3tts_codec.gguf"), 4)
    a = q3.Assets(os.path.join(tiny_model, "gguf_q8_0", "qwen3_assets.gguf"))
    yield oe, a, a.tts_pad()
    a.close()
    oe.close()


def test_feedback_row_restatement(tiny_oracle):
    oe, a, pad = tiny_oracle
    # the fallback row, against the host assets' own loop; the table's last row is not the fallback
    for tok in (resume_ref.SYNTH_TEXT_ROWS, 151673, 2 ** 31 - 1, -1, -5, 987654):
        assert np.array_equal(resume_ref.fallback_row(tok), a.text_embedding(tok)), tok
        assert set(np.unique(resume_ref.fallback_row(tok))) <= {-1.0, 0.0}
    assert not np.array_equal(a.text_embedding(resume_ref.SYNTH_TEXT_ROWS - 1), resume_ref.fallback_row(resume_ref.SYNTH_TEXT_ROWS - 1))
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 2048, (4, 16)).astype(np.int32)
    codes[1, 3], codes[2, 0], codes[3, 5] = 2047, 2159, -4
    rows = resume_ref.feedback_rows(a, pad, codes, [17, 151673])
    for f in range(4):                                                   # spelt out once more, element-wise in float32
        acc = np.zeros(2048, np.float32)
        for q in range(16):
            acc += a.codec_embedding(q, int(codes[f, q]))
        acc += a.text_embedding([17, 151673][f]) if f < 2 else pad
        assert rows.dtype == np.float32 and np.array_equal(rows[f], acc), f
    # left to right is the definition: another order rounds differently somewhere in these rows
    rev = np.zeros(2048, np.float32)
    for q in reversed(range(16)):
        rev += a.codec_embedding(q, int(codes[0, q]))
    assert not np.array_equal(rev + a.text_embedding(17), rows[0])
    # the oracle's assets agree with the product's host assets on every addend
    assert np.array_equal(resume_ref.feedback_rows(oe.assets, pad, codes, [17, 151673]), rows)


CASES = [("greedy", {}, 11), ("sampled", SAMPLED, 12), ("options", dict(SAMPLED, **UPSTREAM), 13), ("greedy_penalty", dict(repetition_penalty=1.3), 14)]


@pytest.mark.parametrize("name,kw,seed", CASES, ids=[c[0] for c in CASES])
def test_resume_restatement_equals_the_uninterrupted_one(tiny_oracle, vivian, name, kw, seed):
    oe, a, pad = tiny_oracle
    rng = np.random.default_rng(seed)
    prompt = oe.assets.build_core(rng.integers(0, 4000, 7).astype(np.int32), lang_id=2055, spk_emb=vivian)
    steps = 10
    want = gen_loop_ref.generate(oe, pad, prompt, steps, seed=seed, mask_eos=True, **kw)
    assert want.shape == (steps, 16)
    assert np.array_equal(resume_ref.resume(oe, pad, prompt, steps, want[:0], seed=seed, **kw), want)          # k = 0 is the loop itself
    for k in (1, 4, 9):
        got = resume_ref.resume(oe, pad, prompt, steps, want[:k], seed=seed, **kw)
        assert np.array_equal(got, want), (name, k)
    if kw.get("temperature", 0) > 0:                                     # the draw offsets are live: another prefix length is another stream position
        other = resume_ref.resume(oe, pad, prompt, steps, want[:4], seed=seed + 1, **kw)
        assert np.array_equal(other[:4], want[:4]) and not np.array_equal(other, want)


def test_resume_restatement_with_trailing_text(tiny_oracle, vivian):
    oe, a, pad = tiny_oracle
    kw = dict(SAMPLED, **UPSTREAM)
    prompt = oe.assets.build_core(np.arange(300, 306, dtype=np.int32), lang_id=2055, spk_emb=vivian)
    for trail in ([40, 41, 42, 43, 44, 45, 46, 151673], [40, 41, 151673]):     # longer and shorter than the split points
        want = text_stream_ref.generate(oe, pad, prompt, 9, trail, seed=21, mask_eos=True, **kw)
        for k in (2, 5):
            assert np.array_equal(resume_ref.resume(oe, pad, prompt, 9, want[:k], trail, seed=21, **kw), want), (len(trail), k)
