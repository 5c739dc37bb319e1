"""Bit-level digests of the ONNX executor (csrc/onnx_exec.hip): every case of product_cases(), row_cases() and zoo_cases() of tests/onnx_cases.py
is run once, and the SHA-256 over dtype, shape and bytes of every output is written out with the run's launch count and the graph's operator names.

    onnx_exec_digest.py --out F            the default kernels, in this process
    onnx_exec_digest.py --out F --naive    the one-output-per-thread kernels: Q3_ONNX_NAIVE is read when the library loads, so a fresh child runs it
    onnx_exec_digest.py --golden F         both, as {"default": ..., "naive": ...}: the form of tests/golden/onnx_exec_digests.json

The fixture is recorded with the library of the commit whose behaviour is to be kept (the script and the case tables use nothing newer than
q3tts.OnnxSession / OnnxModel) and asserted by tests/test_gpu_onnx_exec_bits.py."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "qwen3-tts-rust_amd", "python"))
sys.path.insert(0, os.path.join(ROOT, "tests"))


def here():
    import q3tts
    import onnx_cases
    with tempfile.TemporaryDirectory() as tmp:
        return onnx_cases.digest_cases(q3tts, tmp)


def naive_child(out):
    env = dict(os.environ, Q3_ONNX_NAIVE="1")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", out, "--naive"], env=env, timeout=300)
    if r.returncode != 0:
        sys.exit("the Q3_ONNX_NAIVE child ended with %d" % r.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--golden")
    ap.add_argument("--naive", action="store_true")
    a = ap.parse_args()
    if a.golden:
        with tempfile.TemporaryDirectory() as tmp:
            naive_child(os.path.join(tmp, "naive.json"))
            naive = json.load(open(os.path.join(tmp, "naive.json")))
        res = {"default": here(), "naive": naive}
        out = a.golden
    elif a.naive and os.environ.get("Q3_ONNX_NAIVE") != "1":
        return naive_child(a.out)
    else:
        res, out = here(), a.out
    with open(out, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    n = res["default"] if a.golden else res
    print("%d cases -> %s" % (len(n), out))


if __name__ == "__main__":
    main()
