"""Splits the k_conv_gemm_h3 launches of a rocprofv3 --kernel-trace of scripts/dev_gpu_codec_group.py (one stream count per run) into the
decoder's launches by their order within a pass.  Each of the four decoder stages launches, in this order: convT (2 taps), then three residual
units of conv1 (7 taps, dilation 1 / 3 / 9) + conv2 (1 tap) -- 7 launches per stage, 28 per pass when every one of them is planned as H3 / H3_EPL
(16 and 32 streams: tests/test_codec_gemm_plan_cpu.py).  Prints the median duration of every position and the per-pass sums.
usage: codec_h3_tap_split.py TRACE_DIR [LABEL]"""
import csv
import glob
import statistics
import sys

src = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else src
f = (glob.glob(src + "/**/*_kernel_trace.csv", recursive=True))[0]
rows = sorted((r for r in csv.DictReader(open(f))), key=lambda r: int(r["Start_Timestamp"]))
h3 = [r for r in rows if "k_conv_gemm_h3" in r["Kernel_Name"]]
assert h3 and len(h3) % 28 == 0, "%d k_conv_gemm_h3 launches: not a multiple of 28 per pass" % len(h3)
passes = len(h3) // 28
names = ["convT", "ru0.conv1(d1)", "ru0.conv2", "ru1.conv1(d3)", "ru1.conv2", "ru2.conv1(d9)", "ru2.conv2"]
pos = [[] for _ in range(28)]
for i, r in enumerate(h3):
    pos[i % 28].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    if i >= 28:   # the same position has the same grid in every pass
        assert (r["Grid_Size_X"], r["Grid_Size_Y"]) == (h3[i % 28]["Grid_Size_X"], h3[i % 28]["Grid_Size_Y"]), "launch order changed at %d" % i
med = [statistics.median(p) for p in pos]
total = sum((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows) / passes   # (the few load-time kernels included)
print("%s: %d passes, %d kernel launches in the run, %d of them k_conv_gemm_h3 (28 per pass), %.1f us of kernel time per pass" % (
    label, passes, len(rows), len(h3), total))
k7 = k1 = kt = 0.0
for st in range(4):
    m = med[7 * st:7 * st + 7]
    s7, s1 = m[1] + m[3] + m[5], m[2] + m[4] + m[6]
    k7, k1, kt = k7 + s7, k1 + s1, kt + m[0]
    print("%s dec%d grid %sx%s: %s | k7 sum %.1f k1 sum %.1f" % (label, st, h3[7 * st + 1]["Grid_Size_X"], h3[7 * st + 1]["Grid_Size_Y"],
                                                                  "  ".join("%s %.1f" % (n, v) for n, v in zip(names, m)), s7, s1))
print("%s per pass (medians, us): k7 %.1f  k1 %.1f  convT %.1f  all h3 %.1f  = %.1f %% / %.1f %% / %.1f %% of the pass's kernel time" % (
    label, k7, k1, kt, k7 + k1 + kt, 100 * k7 / total, 100 * k1 / total, 100 * kt / total))
