"""The packed weight layout rule (qwen3-tts-rust_amd/csrc/wlayout.h: row-group sizes and offsets, blob sections, tensor map), built with plain
g++ -- no HIP header, no GPU -- and compared with a restatement from the documented sizes: per 256-column segment of a 32-row group 1024 * 8
bytes of Q8_0 tiles, 5120 of Q5_K planes, 6144 of Q6_K planes; scales Npad * K / 32 * 2 bytes; metadata Npad * K / 256 * 16; the type and the
offset sections rounded up to 16 bytes; blob = [quants | scales | meta | types | offsets]."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_BYTES = {8: 1024 * 8, 13: 5120, 14: 6144}
SCALARS = ["Npad", "mapped", "qbytes", "sc_at", "meta_at", "ty_at", "off_at", "total", "qs_bytes", "sc_bytes", "meta_bytes", "ty_bytes", "off_bytes",
           "nparts", "p0_type", "p0_off", "p1_rg0", "p1_type", "p1_off", "p2_rg0", "p2_type", "p2_off"]
NONE = 0x7FFFFFFF  # first row group of a run the matrix does not have


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("wlayout") / "wlayout_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "host", "wlayout_main.cpp")])

    def run(tensors, N, K, force=0):
        """tensors: (type, first row, rows).  Returns the error message, or (scalars, row-group types, row-group offsets)."""
        text = "%d %d %d %d " % (N, K, force, len(tensors)) + " ".join("%d %d %d" % t for t in tensors) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = r.stdout.splitlines()
        if out[0].startswith("error "):
            return out[0][6:]
        return dict(zip(SCALARS, (int(x) for x in out[0].split()))), [int(x) for x in out[1].split()], [int(x) for x in out[2].split()]
    return run


def stacked(types_rows):
    """[(type, rows)] one under the other -> [(type, first row, rows)], N"""
    t, n = [], 0
    for ty, rows in types_rows:
        t.append((ty, n, rows)); n += rows
    return t, n


def pad16(n):
    return (n + 15) // 16 * 16


def restate(tensors, N, K, force):
    npad = (N + 31) // 32 * 32
    nrg = npad // 32
    mapped = bool(force) or any(t != 8 for t, _, _ in tensors)
    types = [8] * nrg                      # row groups no tensor covers: Q8_0-typed (zero) tiles
    if mapped:
        for t, row0, rows in tensors:
            types[row0 // 32:(row0 + rows) // 32] = [t] * (rows // 32)
    offs, q = [], 0
    for t in types:
        offs.append(q // 16); q += SEG_BYTES[t] * (K // 256)
    size = [q, npad * K // 32 * 2, npad * K // 256 * 16 if mapped else 0, pad16(nrg), pad16(4 * nrg) if mapped else 0]
    at = [sum(size[:i]) for i in range(1, 6)]
    runs = [(i, types[i], offs[i]) for i in range(nrg) if i == 0 or types[i] != types[i - 1]] if mapped else []
    nparts = len(runs)
    runs += [(NONE, 0, 0)] * (3 - nparts)   # fields of a run the matrix does not have keep their defaults
    s = dict(Npad=npad, mapped=int(mapped), qbytes=q if mapped else 0, sc_at=at[0], meta_at=at[1], ty_at=at[2], off_at=at[3], total=at[4],
             qs_bytes=size[0], sc_bytes=size[1], meta_bytes=size[2], ty_bytes=size[3], off_bytes=size[4], nparts=nparts,
             p0_type=runs[0][1], p0_off=runs[0][2], p1_rg0=runs[1][0], p1_type=runs[1][1], p1_off=runs[1][2],
             p2_rg0=runs[2][0], p2_type=runs[2][1], p2_off=runs[2][2])
    return s, types, offs


def check(plan, tensors, N, K, force=0):
    got = plan(tensors, N, K, force)
    assert not isinstance(got, str), got
    assert got == restate(tensors, N, K, force)
    return got


def test_header_is_hip_free():
    src = open(os.path.join(ROOT, "qwen3-tts-rust_amd", "csrc", "wlayout.h")).read()
    includes = re.findall(r'#include\s+[<"]([^>"]+)', src)
    assert includes and all("/" not in i and "." not in i for i in includes)  # std only


def test_one_row_group_size_rule():
    csrc = os.path.join(ROOT, "qwen3-tts-rust_amd", "csrc")
    defs = [f for f in sorted(os.listdir(csrc)) if re.search(r"size_t\s+q3_rowgroup_bytes\s*\(", open(os.path.join(csrc, f), errors="replace").read())]
    assert defs == ["wlayout.h"]


def test_uniform_q8(plan):
    s, types, offs = check(plan, [(8, 0, 40)], 40, 512)
    assert s["Npad"] == 64 and not s["mapped"] and s["nparts"] == 0 and s["qbytes"] == 0  # qbytes 0: the kernels take Npad * K
    assert s["qs_bytes"] == 64 * 512 and s["sc_bytes"] == 64 * 16 * 2 and s["meta_bytes"] == 0 and s["off_bytes"] == 0
    assert types == [8, 8] and offs == [0, 512 * 1024 // 32 // 16]
    # tensors of a uniform matrix need not start or end on a row group
    s, types, offs = check(plan, [(8, 0, 33), (8, 33, 7)], 40, 512)
    assert s["Npad"] == 64 and not s["mapped"]


def test_two_runs(plan):
    tensors, n = stacked([(13, 256), (13, 128), (14, 128)])
    s, types, offs = check(plan, tensors, n, 1024)
    assert s["mapped"] and s["nparts"] == 2 and (s["p0_type"], s["p1_type"]) == (13, 14) and s["p1_rg0"] == 12 and s["p2_rg0"] == NONE
    assert offs[:13] == [i * 4 * 5120 // 16 for i in range(13)] and offs[13] - offs[12] == 4 * 6144 // 16  # cumulative
    assert s["p0_off"] == 0 and s["p1_off"] == offs[12] and s["qbytes"] == 12 * 4 * 5120 + 4 * 4 * 6144
    assert s["ty_bytes"] == 16 and s["off_bytes"] == 64 and s["meta_bytes"] == 512 * 4 * 16


@pytest.mark.parametrize("order", [(13, 8, 14), (13, 14, 13)])
def test_three_runs(plan, order):
    tensors, n = stacked([(t, 32) for t in order])
    s, types, offs = check(plan, tensors, n, 256)
    assert s["nparts"] == 3 and types == list(order) and (s["p0_type"], s["p1_type"], s["p2_type"]) == order
    assert (s["p1_rg0"], s["p2_rg0"]) == (1, 2) and (s["p0_off"], s["p1_off"], s["p2_off"]) == tuple(offs)
    assert offs == [0, SEG_BYTES[order[0]] // 16, (SEG_BYTES[order[0]] + SEG_BYTES[order[1]]) // 16]


def test_forced_map_of_q8(plan):
    s, types, offs = check(plan, [(8, 0, 64)], 64, 512, force=1)
    assert s["mapped"] and s["nparts"] == 1 and s["p0_type"] == 8 and s["qbytes"] == 64 * 512 and s["off_bytes"] == 16
    assert s["meta_bytes"] == 64 * 2 * 16  # a mapped matrix always carries the metadata section


def test_uncovered_last_row_group(plan):
    s, types, offs = check(plan, [(13, 0, 64)], 96, 512)
    assert types == [13, 13, 8] and offs[2] == 2 * 2 * 5120 // 16 and s["qbytes"] == 2 * 2 * 5120 + 2 * 8192
    assert s["nparts"] == 2 and (s["p1_rg0"], s["p1_type"], s["p1_off"]) == (2, 8, offs[2])


def test_refusals(plan):
    four, n = stacked([(13, 32), (14, 32), (13, 32), (14, 32)])
    assert "more than 3 runs" in plan(four, n, 256)
    assert "multiple of 32" in plan([(13, 0, 48)], 48, 256)                  # a K-quant tensor of 48 rows
    assert "multiple of 32" in plan([(8, 0, 48), (14, 48, 16)], 64, 256)     # ... and a Q8_0 one next to a K-quant tensor
    assert "multiple of 32" in plan([(8, 0, 48)], 48, 256, 1)
    assert "multiple of 256" in plan([(8, 0, 32)], 32, 384)
    assert "unsupported weight type" in plan([(12, 0, 32)], 32, 256)
    assert "bad row range" in plan([(8, 0, 65)], 40, 256)
    assert "bad row range" in plan([(13, 64, 64)], 96, 256)
    # 32-bit offsets in 16-byte units: 2^36 bytes of quants is one too many
    assert "32-bit" in plan([(8, 0, 1 << 20)], 1 << 20, 1 << 16)
    assert not isinstance(plan([(8, 0, (1 << 20) - 32)], (1 << 20) - 32, 1 << 16), str)
