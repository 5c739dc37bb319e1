"""[EXT] live text append, CPU half: the new entry points are declared and listed, fail cleanly without an engine or a device, and the two
stall kernels compile for gfx950 without scratch.  No GPU is used."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
NEW = ["q3tts_submit_trailing_open", "q3tts_trail_append", "q3tts_trail_progress", "q3tts_submit_text_streaming_open", "q3tts_text_append",
       "q3tts_group_submit_text_streaming_open", "q3tts_group_text_append", "q3tts_group_trail_append", "q3tts_group_trail_progress"]


def test_new_names_are_declared_and_listed(q3):
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "q3tts.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % n, txt), n
        assert n in q3.SYMBOLS, n
        assert hasattr(q3.lib(), n), n


def test_new_entry_points_fail_without_an_engine(q3):
    L = q3.lib()
    ids = np.arange(4, dtype=np.int32)
    rid = C.c_int64(7)
    na, nc, cl = C.c_int32(-5), C.c_int32(-5), C.c_int32(-5)
    r = q3.Request()
    sc = q3.SamplerConfig(0.0, 40, 0.9, 1, 1)
    assert L.q3tts_submit_trailing_open(None, C.byref(r), 0, None, q3._p(ids), ids.size, C.byref(rid)) < 0
    assert rid.value == 7
    assert L.q3tts_trail_append(None, 1, q3._p(ids), ids.size, 0) < 0
    assert L.q3tts_trail_append(None, 1, None, 0, 1) < 0
    assert L.q3tts_trail_progress(None, 1, C.byref(na), C.byref(nc), C.byref(cl)) < 0
    assert (na.value, nc.value, cl.value) == (-5, -5, -5)
    assert L.q3tts_submit_text_streaming_open(None, 0, q3._p(ids), ids.size, 2055, None, 0, C.byref(sc), 8, 1, 0, None, C.byref(rid)) < 0
    assert L.q3tts_text_append(None, 1, q3._p(ids), ids.size, 1) < 0
    assert L.q3tts_group_submit_text_streaming_open(None, 0, q3._p(ids), ids.size, 2055, None, 0, C.byref(sc), 8, 1, 0, None,
                                                    C.byref(rid)) < 0
    assert L.q3tts_group_text_append(None, 1, q3._p(ids), ids.size, 0) < 0
    assert L.q3tts_group_trail_append(None, 1, q3._p(ids), ids.size, 0) < 0
    assert L.q3tts_group_trail_progress(None, 1, C.byref(na), C.byref(nc), C.byref(cl)) < 0
    assert rid.value == 7 and (na.value, nc.value, cl.value) == (-5, -5, -5)
    assert q3.lib().q3tts_last_error()


def test_python_surface(q3):
    for name in ("trail_append", "text_append", "trail_progress"):
        assert callable(getattr(q3.Engine, name))
    import inspect
    assert "open_trail" in inspect.signature(q3.Engine.submit).parameters
    assert "open_text" in inspect.signature(q3.Engine.submit_text).parameters


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_stall_kernels_use_no_scratch(tmp_path):
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
        if "k_stall_save" in name or "k_advance_keys" in name:
            seen[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))
    assert any("k_stall_save" in n for n in seen), seen
    assert any("k_advance_keys_gated" in n for n in seen), seen
    assert len(seen) == 3 and set(seen.values()) == {0}, seen
