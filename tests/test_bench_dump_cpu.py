"""bench.py --dump-outputs: what the timed region computed, written as float32 / float64 .npy files within the 64 MB budget
(no GPU: the stub engine for the bench's own flow, synthetic results for the sampling path)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_bench_dump_outputs_stub_engine(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--stub-engine", "--requests", "5",
                        "--batch", "4", "--ragged", "--dump-outputs", d], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    a = _load(d)
    assert sorted(a) == ["codes", "frames"]          # the stub engine returns no PCM
    frames = [max(1, int(12 * (0.5 + 0.5 * ((i * 7) % 11) / 10.0))) for i in range(5)]   # --steps 3 = 12 frames before the ragged cut
    assert a["frames"].dtype == np.float64 and a["frames"].tolist() == frames
    assert a["codes"].dtype == np.float32 and a["codes"].shape == (5, max(frames), 16)
    for i, n in enumerate(frames):
        assert (a["codes"][i, :n] == 0).all() and (a["codes"][i, n:] == -1).all()


def test_bench_dump_outputs_two_ranks_share_the_budget(tmp_path):
    """--gpus 2: every rank writes its own results under a rank prefix, and the directory as a whole stays within 64 MB"""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = str(tmp_path / "out")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1", "--stub-engine",
                        "--requests", "5", "--batch", "4", "--dump-outputs", d], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert sorted(os.listdir(d)) == ["rank0_codes.npy", "rank0_frames.npy", "rank1_codes.npy", "rank1_frames.npy"]
    assert sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d)) <= bench.DUMP_BYTES
    for k in (0, 1):
        assert np.load(os.path.join(d, "rank%d_codes.npy" % k)).shape == (5, 12, 16)


def test_dump_refuses_shapes_whose_codes_alone_break_the_budget(tmp_path, capsys):
    big = ["--requests", "512", "--steps", "256", "--dump-outputs", str(tmp_path), "--model-dir", str(tmp_path)]   # 32 MB of codes per rank
    assert bench.parse_args(big).dump_outputs == str(tmp_path)
    with pytest.raises(SystemExit):
        bench.parse_args(big + ["--gpus", "2"])       # 2 x 32 MB > 64 MB
    assert "exceed the 64 MB budget" in capsys.readouterr().err
    with pytest.raises(ValueError):
        bench.dump_outputs(str(tmp_path), _results(2, 8, 3), budget=1000)


def _results(n_req, n_frames, seed):
    rng = np.random.default_rng(seed)
    return [{"codes": rng.integers(0, 2048, (n_frames, 16)).astype(np.int32), "pcm": rng.standard_normal(n_frames * 1920).astype(np.float32)}
            for _ in range(n_req)]


def test_dump_outputs_whole_pcm_when_it_fits(tmp_path):
    res = _results(3, 8, 1)
    assert bench.dump_outputs(str(tmp_path), res) == ["codes", "frames", "pcm", "pcm_samples"]
    a = _load(str(tmp_path))
    assert np.array_equal(a["codes"], np.stack([r["codes"] for r in res]).astype(np.float32))
    assert np.array_equal(a["pcm"], np.concatenate([r["pcm"] for r in res])) and a["pcm_samples"].tolist() == [8 * 1920] * 3


def test_dump_outputs_samples_pcm_over_budget(tmp_path):
    res = _results(4, 64, 2)                          # 4 x 64 x 1920 x 4 B = 1.9 MB of PCM against a 1 MB budget
    full = np.concatenate([r["pcm"] for r in res])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, budget=1 << 20)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sum(os.path.getsize(str(tmp_path / "a" / f)) for f in os.listdir(str(tmp_path / "a"))) <= 1 << 20
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    idx = a["pcm_index"].astype(np.int64)
    assert np.array_equal(idx, a["pcm_index"]) and (np.diff(idx) > 0).all() and idx[-1] < full.size and idx.size > (1 << 20) // 13
    assert np.array_equal(a["pcm"], full[idx])
    assert all(np.array_equal(a[k], b[k]) for k in a)   # the sample is fixed: the same outputs give the same files
