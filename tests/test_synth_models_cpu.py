"""The synthetic-model cache (tests/synth_models.py): a private per-user root, keyed on the generator's sources, old keys pruned."""
import os
import stat
import tempfile
import time

import synth_models


def test_cache_root_is_private_and_old_generators_are_pruned(tmp_path, monkeypatch):
    monkeypatch.setattr(tempfile, "tempdir", str(tmp_path))
    root = tmp_path / ("q3tts-models-%d" % os.getuid())
    root.mkdir(mode=0o755)                               # a root left with looser permissions is tightened, not trusted as it is
    old, recent, other = root / "0123456789abcdef", root / "fedcba9876543210", root / "notes"
    for d in (old, recent, other):
        d.mkdir()
    os.utime(str(old), (time.time() - 2 * 86400,) * 2)
    d = synth_models.model_dir("tiny")
    key = synth_models._digest()[:16]
    assert d == str(root / key / "tiny") and (root / key).is_dir()
    assert stat.S_IMODE(os.lstat(str(root)).st_mode) == 0o700
    assert not old.exists() and recent.exists() and other.exists()
