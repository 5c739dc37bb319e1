"""[EXT] the host-only rules of the ONNX executor (csrc/onnx_shape.h) without a GPU: the checked axis, Slice geometry against an index-by-index
walk, Conv / ConvTranspose output sizes and pads against a count of the positions that fit, the Reshape / Flatten / Squeeze / Unsqueeze rules
against the operator definitions spelled out, and the one broadcast walker (with the host evaluators built on it) against nested loops.
tests/host/onnx_shape_main.cpp restates each rule and checks the grids itself, as a stand-alone program under the host sanitizers; the counts
asserted here are the sizes of those grids, worked out again in Python."""
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("onnx_shape") / "onnx_shape_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "host", "onnx_shape_main.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return dict(l.split() for l in r.stdout.splitlines())


def test_axis_of_refuses_every_axis_outside_the_range(lines):
    """ranks 0..4, every axis in [-rank - 3, rank + 3], with and without the end allowed (Flatten)"""
    assert int(lines["axes"]) == sum((2 * r + 7) * 2 for r in range(5))


def test_slice_against_an_index_by_index_walk(lines):
    """dim 0..5, every start and end in [-dim - 2, dim + 2], steps -3..3 without 0"""
    assert int(lines["slice"]) == sum((2 * d + 5) ** 2 for d in range(6)) * 6


def test_conv_sizes_against_a_count_of_positions(lines):
    """extents 1..9, kernels 1..4, strides and dilations 1..3.  Conv: 9 explicit pad pairs + VALID + both SAME modes.  ConvTranspose, for
    output_padding 0 and 1: the 9 pad pairs + both SAME modes; then output_shape from 2 below to 1 above what the taps reach (at least 1) in 3 modes"""
    n = 0
    for i, k, s, d in itertools.product(range(1, 10), range(1, 5), range(1, 4), range(1, 4)):
        reach = (i - 1) * s + (k - 1) * d + 1
        n += 12 + 2 * 11 + 3 * (reach + 1 - max(1, reach - 2) + 1)
    assert int(lines["conv"]) == n


def test_shape_rules_against_the_definitions(lines):
    """every shape of rank 0..3 with extents 0..3: Flatten at every axis, Squeeze without axes and with every pair, Unsqueeze with every pair of
    distinct output axes, Reshape with the 0 / -1 targets of its rank, with and without allowzero"""
    n = 0
    for r in range(4):
        pairs = sum(1 for a in range(-r - 2, r + 2) for b in range(-r - 2, r + 2) if a % (r + 2) != b % (r + 2))
        n += 4 ** r * ((2 * r + 1) + 1 + (2 * r) * (2 * r + 1) // 2 + pairs + 2 * (4 + (r >= 1) + 2 * (r >= 2)))
    assert int(lines["shapes"]) == n


def test_the_broadcast_walker_against_nested_loops(lines):
    """every ordered pair of shapes of rank 0..3 with extents 1..3 that broadcast (the others are refused)"""
    shapes = [s for r in range(4) for s in itertools.product((1, 2, 3), repeat=r)]
    n = 0
    for a in shapes:
        for b in shapes:
            try:
                np.broadcast_shapes(a, b)
                n += 1
            except ValueError:
                pass
    assert int(lines["walk"]) == n
