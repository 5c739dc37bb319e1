"""Seeded synthetic models written by tools/q3synth for the tests, smoke() and bench.py.

The checkout itself may be read-only when they run, so the models are cached outside it, in <temp dir>/q3tts-models-<uid>/: a directory
this user owns and nobody else can write to (it is refused otherwise).  Inside it, models sit under a key made of the generator's sources,
so a model written by another version of q3synth is never read and two checkouts with the same generator share one copy; another
generator's models are removed once they have gone unused for a day.  A lock serialises the writers of one model directory, q3synth is
brought up to date before it writes, and the marker (written last) records the exact passes that filled the directory."""
import fcntl
import hashlib
import os
import shutil
import stat
import subprocess
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "q3synth")
SOURCES = ("tools/q3synth.c", "include/q3tts_spec.h")   # what tools/Makefile builds q3synth from


def _digest(extra=b""):
    h = hashlib.sha256()
    for f in SOURCES:
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(fh.read())
    h.update(extra)
    return h.hexdigest()


def _user_root():
    root = os.path.join(tempfile.gettempdir(), "q3tts-models-%d" % os.getuid())
    try:
        os.mkdir(root, 0o700)
    except FileExistsError:
        pass
    st = os.lstat(root)
    if not stat.S_ISDIR(st.st_mode) or st.st_uid != os.getuid():
        raise RuntimeError("%s is not a directory of this user; remove it or point Q3_TINY_MODEL / Q3_BENCH_MODEL elsewhere" % root)
    if st.st_mode & 0o077:
        os.chmod(root, 0o700)
    return root


def _prune(root, keep, max_age_s=86400.0):
    """removes other generators' models that have gone unused for max_age_s (model_dir() touches the key directory at every use)"""
    now = time.time()
    for d in os.listdir(root):
        p = os.path.join(root, d)
        if d != keep and len(d) == 16 and all(c in "0123456789abcdef" for c in d) and os.path.isdir(p) and not os.path.islink(p) \
                and now - os.lstat(p).st_mtime > max_age_s:
            shutil.rmtree(p, ignore_errors=True)


def model_dir(name):
    root, key = _user_root(), _digest()[:16]
    os.makedirs(os.path.join(root, key), exist_ok=True)
    os.utime(os.path.join(root, key))
    _prune(root, key)
    return os.path.join(root, key, name)


def ensure(out, passes, tag="all"):
    """Runs `q3synth --out OUT <pass>` for every pass in order unless OUT already holds their output from the current sources
    (marker OUT/.synth_<tag>).  Returns OUT."""
    marker = os.path.join(out, ".synth_" + tag)
    fp = _digest(repr([list(p) for p in passes]).encode())
    os.makedirs(out, mode=0o700, exist_ok=True)
    with open(os.path.join(out, ".lock"), "w") as lk:
        fcntl.flock(lk, fcntl.LOCK_EX)   # another process may be writing this model right now: wait for it
        if os.path.exists(marker):
            with open(marker) as fh:
                if fh.read() == fp:
                    return out
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools")])   # a stale q3synth must not fill a directory keyed on newer sources
        for p in passes:
            subprocess.check_call([TOOL, "--out", out] + list(p))
        with open(marker, "w") as fh:
            fh.write(fp)
    return out


def full(quant, out=None):
    """Q3TTS-1.7B-synth at the real dimensions (seed 1234) in one quantisation; bench.py and the full-size GPU tests share it"""
    out = out or os.environ.get("Q3_BENCH_MODEL") or model_dir("full")
    return ensure(out, [["--preset", "full", "--quant", quant, "--seed", "1234"]], tag=quant)
