"""[EXT] codec preambles, CPU half (include/q3tts_spec.h "codec preambles"): the entry points are declared, exported, listed and fail cleanly
without an engine, a decoder or a device; every refusal of q3tts_preamble_create is reached through the pure rule of csrc/sched_logic.h,
together with the reference-count rule (who holds a preamble, when its snapshot's slot may be recycled), what a setter refuses and which
preamble a request is primed with.  The rules are built with plain g++ and the host sanitizers, like the other rule drivers.  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINE = ("q3tts_preamble_create", "q3tts_preamble_poll", "q3tts_preamble_wait", "q3tts_preamble_release", "q3tts_voice_set_preamble",
          "q3tts_engine_set_preamble", "q3tts_request_preamble", "q3tts_engine_preamble_stats")
GROUP = ("q3tts_group_preamble_create", "q3tts_group_preamble_wait", "q3tts_group_preamble_release", "q3tts_group_voice_set_preamble",
         "q3tts_group_set_preamble", "q3tts_group_request_preamble")
DECODER = ("q3tts_decoder_snapshot_create", "q3tts_decoder_snapshot_restore", "q3tts_decoder_snapshot_free", "q3tts_decoder_snapshot_bytes")
SAMPLE_END, CODEC_EOS, MAX_POS = 2160, 2150, 65536   # Q3_SAMPLE_END, Q3_CODEC_EOS, Q3TTS_CODEC_MAX_FRAMES
BUILDING, READY, FAILED = 0, 1, -1


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def test_names_are_declared_exported_and_listed(q3):
    txt = _header("q3tts.h")
    for n in ENGINE + GROUP + DECODER:
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % n, txt), n
        assert n in q3.SYMBOLS and hasattr(q3.lib(), n) and getattr(q3.lib(), n).argtypes, n
    assert re.search(r"\bint\s+q3tts_preamble_create\s*\(\s*q3tts_engine\s*\*\s*\w+\s*,\s*const\s+int32_t\s*\*\s*codes\s*,\s*int32_t\s+n\s*,"
                     r"\s*int32_t\s*\*\s*preamble_id\s*\)\s*;", txt)
    assert re.search(r"\bint\s+q3tts_decoder_snapshot_restore\s*\(\s*q3tts_decoder\s*\*\s*\w+\s*,\s*int32_t\s+snapshot\s*,\s*int32_t\s+stream\s*\)\s*;", txt)
    spec = open(os.path.join(ROOT, "include", "q3tts_spec.h")).read()
    sec = spec[spec.index("codec preambles [EXT]"):]
    for word in ("P1", "P2", "P3", "P4", "Q3_PCM_HIST", "m * 1920", "READY"):
        assert word in sec, word
    stripped = _header("q3tts_spec.h")
    assert re.search(r"#define\s+Q3TTS_MAX_PREAMBLES\s+64\b", stripped)
    for name, val in (("BUILDING", "0"), ("READY", "1"), ("FAILED", "-1")):
        assert re.search(r"#define\s+Q3TTS_PREAMBLE_%s\s+%s\b" % (name, re.escape(val)), stripped), name
    assert (q3.MAX_PREAMBLES, q3.PREAMBLE_BUILDING, q3.PREAMBLE_READY, q3.PREAMBLE_FAILED) == (64, BUILDING, READY, FAILED)


def test_python_surface(q3):
    for n in ("preamble_create", "preamble_poll", "preamble_wait", "preamble_release", "voice_set_preamble", "set_preamble",
              "request_preamble", "preamble_stats", "prime_voice"):
        assert callable(getattr(q3.Engine, n)), n
    for n in ("snapshot_create", "snapshot_restore", "snapshot_free", "snapshot_bytes"):
        assert callable(getattr(q3.Decoder, n)), n
    for n in ("group_preamble_create", "group_preamble_wait", "group_preamble_release", "group_voice_set_preamble", "group_set_preamble",
              "group_request_preamble"):
        assert callable(getattr(q3, n)), n


def test_entry_points_fail_cleanly_without_an_engine_or_a_device(q3):
    L = q3.lib()
    codes, pid, st = np.full((4, 16), 7, np.int32), C.c_int32(-5), C.c_int32(-9)
    for fn in (L.q3tts_preamble_create, L.q3tts_group_preamble_create):
        assert fn(None, q3._p(codes), 4, C.byref(pid)) < 0 and L.q3tts_last_error() and pid.value == -5
    assert L.q3tts_preamble_poll(None, 0, C.byref(st), None) < 0 and L.q3tts_last_error() and st.value == -9
    for fn in (L.q3tts_preamble_wait, L.q3tts_group_preamble_wait):
        assert fn(None, 0, 0.0) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_preamble_release, L.q3tts_group_preamble_release, L.q3tts_engine_set_preamble, L.q3tts_group_set_preamble):
        assert fn(None, 0) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_voice_set_preamble, L.q3tts_group_voice_set_preamble):
        assert fn(None, 0, 0) < 0 and L.q3tts_last_error()
    for fn in (L.q3tts_request_preamble, L.q3tts_group_request_preamble):
        assert fn(None, 1, C.byref(pid)) < 0 and L.q3tts_last_error() and pid.value == -5
    a = C.c_int64(-7)
    assert L.q3tts_engine_preamble_stats(None, C.byref(a), None, None) < 0 and L.q3tts_last_error() and a.value == -7
    assert L.q3tts_decoder_snapshot_create(None, 0, C.byref(pid)) < 0 and L.q3tts_last_error() and pid.value == -5
    assert L.q3tts_decoder_snapshot_restore(None, 0, 0) < 0 and L.q3tts_last_error()
    assert L.q3tts_decoder_snapshot_free(None, 0) < 0 and L.q3tts_last_error()
    assert L.q3tts_decoder_snapshot_bytes(None) < 0
    with pytest.raises(q3.Q3Error):
        q3.group_preamble_create(None, codes)
    with pytest.raises(q3.Q3Error):
        q3.group_set_preamble(None, None)
    if q3.device_count() == 0:   # there is no codec to build a preamble on without a device
        with pytest.raises(q3.Q3Error, match="no HIP device"):
            q3.Engine(os.path.join(ROOT, "no_such_model"), "q8_0", max_batch=1, max_steps=8)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("preamble_logic") / "preamble_logic_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                           os.path.join(ROOT, "tests", "host", "preamble_logic_main.cpp")])

    def run(text):
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        return r.stdout.splitlines()
    return run


def _refusal(driver, n=6, max_steps=16, have_codec=1, null_codes=0, at=-1, c0=5, res=7, live=0, max_pos=MAX_POS):
    return driver("refusal %d %d %d %d %d %d %d %d %d\n" % (n, max_steps, have_codec, null_codes, at, c0, res, live, max_pos))[0]


def test_every_refusal_and_the_accepting_edges(driver):
    assert _refusal(driver) == "ok"
    assert _refusal(driver, n=1) == "ok" and _refusal(driver, n=16) == "ok"
    # what a decode-only request is refused for
    assert "max_steps" in _refusal(driver, n=17)
    assert "n must be >= 1" in _refusal(driver, n=0) and "n must be >= 1" in _refusal(driver, n=-3)
    assert "load_codec" in _refusal(driver, have_codec=0)
    assert "codes missing" in _refusal(driver, null_codes=1)
    for at in (0, 3, 5):
        assert "EOS" in _refusal(driver, at=at, c0=CODEC_EOS)
        assert "code_0" in _refusal(driver, at=at, c0=SAMPLE_END) and "code_0" in _refusal(driver, at=at, c0=-1)
        assert "residual" in _refusal(driver, at=at, res=2048) and "residual" in _refusal(driver, at=at, res=-1)
        assert _refusal(driver, at=at, c0=2048, res=2047) == "ok"
    # the preamble's own: the 65th live one, and RoPE positions n + max_steps past the codec's tables
    assert _refusal(driver, live=63) == "ok"
    assert "Q3TTS_MAX_PREAMBLES" in _refusal(driver, live=64) and "Q3TTS_MAX_PREAMBLES" in _refusal(driver, live=200)
    assert _refusal(driver, n=6, max_steps=16, max_pos=22) == "ok"
    assert "positions" in _refusal(driver, n=6, max_steps=16, max_pos=21)
    # a bad frame is reported before the count: nothing of a refused preamble is counted or queued
    assert "EOS" in _refusal(driver, at=2, c0=CODEC_EOS, live=64)


def test_reference_count_rule(driver):
    assert driver("fresh\n")[0] == "1 0 %d 0" % BUILDING      # its creator holds it, it is building, it is not recyclable

    def rec(creator, holders, state):
        return int(driver("recyclable %d %d %d\n" % (creator, holders, state))[0])
    table = [
        # creator, holders, state, recyclable
        (1, 0, BUILDING, 0), (1, 0, READY, 0), (1, 3, READY, 0), (1, 0, FAILED, 0),       # the creator has not released it
        (0, 1, READY, 0), (0, 2, READY, 0), (0, 1, FAILED, 0),                            # a voice, the engine or a request still holds it
        (0, 0, BUILDING, 0), (0, 1, BUILDING, 0),                                         # released while it builds: its stream is still decoding
        (0, 0, READY, 1), (0, 0, FAILED, 1),                                              # nobody left, the build has ended
    ]
    for creator, holders, state, want in table:
        assert rec(creator, holders, state) == want, (creator, holders, state)


def test_setters_take_ready_preambles_only(driver):
    assert driver("set 1 %d\n" % READY)[0] == "ok"
    assert "building" in driver("set 1 %d\n" % BUILDING)[0]
    assert "failed" in driver("set 1 %d\n" % FAILED)[0]
    for st in (BUILDING, READY, FAILED):
        assert "unknown" in driver("set 0 %d\n" % st)[0]


def test_which_preamble_a_request_takes(driver):
    def of(want_pcm, asked, eng):
        return int(driver("of %d %d %d\n" % (want_pcm, asked, eng))[0])
    assert of(1, -2, 5) == 5 and of(1, -2, -1) == -1          # a raw-prompt form: the engine-level setting
    assert of(1, 3, 5) == 3 and of(1, -1, 5) == -1            # a text form: its voice's, never the engine's
    for asked in (-2, -1, 3):
        assert of(0, asked, 5) == -1                          # never without PCM
