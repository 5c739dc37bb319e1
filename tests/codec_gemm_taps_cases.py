"""Cases and checker for the tap-reusing main loop of k_conv_gemm_h3 (csrc/codec.hip), shared by tests/test_gpu_codec_gemm_taps.py and by its
child process, which runs this file with Q3_CODEC_H3_TAPS=0 (the tap-major loop) over the same list.

The loop stages, per 128-row tile and 32-channel chunk, the physical rows phys(m0) .. phys(m1) + (taps - 1) * dil once (phys(m) = m + (m // a_segT) *
a_skip, m1 = the tile's last row below M) and lets every tap read its rows out of that halo tile.  What can break: the row offset of a lane across
segment boundaries, the halo's end (clamped loader slots, the last row of the A buffer), rows inside the halo nobody may use, the span limit."""
import numpy as np

import codec_gemm_ref as R

HALO_ROWS = 240   # H3_HALO_ROWS in csrc/codec.hip: 240 rows x 160 B + 15 360 B of weights = 53 760 B of LDS, three workgroups per CU
F32_NAN, F16_NAN_PAIR = np.uint32(0x7FC00000), np.uint32(0x7E007E00)


def phys(m, segT, skip):
    return R.seg_rows(m, segT, skip)


def halo_span(M, taps, dil, segT, skip):
    """the largest halo of a 128-row tile (h3_halo_span in csrc/codec.hip, restated tile by tile)"""
    span = 0
    for m0 in range(0, M, 128):
        m1 = min(m0 + 128, M) - 1
        span = max(span, int(phys(m1, segT, skip) - phys(m0, segT, skip)) + (taps - 1) * dil + 1)
    return span


# (form, M, N, cin, taps, dil, a_segT, a_skip, a_split)
def _cases():
    c = []
    # segment crossings: tiles inside one segment (0), aligned to it (128), crossing one (64) or two (48) boundaries
    for M in (129, 255):
        for cin in (32, 64):
            for dil in (1, 3, 9):
                for segT in (0, 128, 64, 48):
                    for form in ("H3", "H3_EPL"):
                        c.append((form, M, 96, cin, 7, dil, segT, 6 * dil if segT else 0, False))
    # two-segment tiles whose segments are further apart than the taps reach: rows inside the halo that no output may use
    for dil in (1, 3):
        c.append(("H3_EPL", 129, 96, 64, 7, dil, 48, 6 * dil + 5, False))
        c.append(("H3", 255, 96, 32, 7, dil, 48, 6 * dil + 1, True))
    # both sides of the span limit: 128 + a_skip + 6 * 9 = 240 and 241
    for form in ("H3", "H3_EPL"):
        c.append((form, 129, 96, 32, 7, 9, 64, HALO_ROWS - 128 - 54, False))
        c.append((form, 129, 96, 32, 7, 9, 64, HALO_ROWS - 128 - 54 + 1, False))
    # other tap counts: transposed convs (2 taps, history 1), pre_conv (3 taps, 4-row segments: 31 boundaries in a tile)
    for form in ("H3", "H3_EPL"):
        c.append((form, 129, 192, 64, 2, 1, 16, 1, False))
        c.append((form, 255, 96, 32, 3, 1, 4, 2, False))
        c.append((form, 129, 96, 64, 2, 1, 0, 0, True))
    # pre-split operands
    for dil in (1, 3, 9):
        for segT in (0, 64, 48):
            c.append(("H3_EPL" if dil != 3 else "H3", 129, 96, 64, 7, dil, segT, 6 * dil if segT else 0, True))
    return c


CASES = _cases()
# one shape per form for the epilogues (EPI_NONE, EPI_RES, EPI_SNAKE)
EPI_CASES = [("H3", 255, 96, 64, 7, 3, 64, 18, False), ("H3_EPL", 129, 192, 32, 7, 9, 64, 54, False), ("H3_EPL", 129, 96, 64, 7, 1, 48, 11, True)]


def case_id(c):
    return "%s-M%d-N%d-cin%d-k%dd%d-seg%d+%d%s" % (c[:8] + ("-split" if c[8] else "",))


def expects_tap_reuse(c):
    form, M, N, cin, taps, dil, segT, skip, a_split = c
    return taps > 1 and halo_span(M, taps, dil, segT, skip) <= HALO_ROWS


class Problem:
    """A whose last row is the last row some output reads (the last tile ends exactly at the end of the buffer); every row no (row < M, tap)
    reads is poison (NaN), the padding columns as well; `clean` holds finite values in the poisoned rows instead"""

    def __init__(self, c, seed):
        self.c = c
        form, M, N, cin, taps, dil, segT, skip, a_split = c
        rng = np.random.default_rng(seed)
        base = phys(np.arange(M), segT, skip)
        a_rows = int(base[-1]) + (taps - 1) * dil + 1
        used = np.zeros(a_rows, bool)
        for j in range(taps):
            used[base + j * dil] = True
        self.unused = int((~used).sum())
        # unused rows inside some tile's halo (the loop stages them; the tap-major loop never loads them)
        inside = np.zeros(a_rows, bool)
        for m0 in range(0, M, 128):
            m1 = min(m0 + 128, M) - 1
            inside[int(base[m0]):int(base[m1]) + (taps - 1) * dil + 1] = True
        self.unused_in_halo = int((~used & inside).sum())
        lda = cin + 4
        vals = rng.standard_normal((a_rows, cin)).astype(np.float32)
        if a_split:
            A = np.zeros((a_rows, lda), np.uint32)
            A[:, :cin] = R.split_rows(vals)
            self.A_val = R.unsplit_rows(A, cin)[2]
            poison = F16_NAN_PAIR
        else:
            A = np.full((a_rows, lda), F32_NAN, np.uint32)
            A[:, :cin] = vals.view(np.uint32)
            self.A_val = vals.astype(np.float64)
            poison = F32_NAN
        self.clean = A.copy()
        A[~used, :cin] = poison
        self.A = A
        self.W = (rng.standard_normal((N, cin * taps)) / np.sqrt(cin * taps)).astype(np.float32)
        self.ref, self.absb = R.gemm_ref(self.A_val, self.W, M, cin, taps, dil, segT, skip)

    def view(self, A):
        return A if self.c[8] else A.view(np.float32)

    def run(self, q3, A=None, **kw):
        form, M, N, cin, taps, dil, segT, skip, a_split = self.c
        out, info = q3.op_codec_gemm(self.view(self.A if A is None else A), self.W, M, cin, taps, dil, a_segT=segT, a_skip=skip, a_split=a_split,
                                     form=form, **kw)
        assert info == (form, 1, -1), info
        return out.reshape(M, N)

    def query(self, q3):
        form, M, N, cin, taps, dil, segT, skip, a_split = self.c
        return q3.codec_gemm_tap_reuse(M, N, cin, taps, dil, lda=cin + 4, a_segT=segT, a_skip=skip, a_split=a_split, form=form)


def check_case(q3, c, taps_on=True):
    """runs one case; returns the Problem (for its counts).  Asserts: the query, float64 agreement, finite output, poison has no effect"""
    p = Problem(c, CASES.index(c) if c in CASES else 1000 + EPI_CASES.index(c))
    assert p.query(q3) == (taps_on and expects_tap_reuse(c)), "tap-reuse query"
    out = p.run(q3)
    assert np.all(np.isfinite(out)), "%d non-finite outputs" % int((~np.isfinite(out)).sum())
    err = np.abs(out.astype(np.float64) - p.ref)
    K = c[3] * c[4]
    bar = R.shape_bar(K) * p.absb + 2.0 ** -22 * np.abs(p.ref)
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    assert np.all(err <= bar), "row %d col %d: |err| %.3g > bar %.3g" % (worst + (err[worst], bar[worst]))
    if p.unused:
        assert np.array_equal(out.view(np.uint32), p.run(q3, p.clean).view(np.uint32)), "rows no output reads changed the result"
    return p


def _ulp(x):
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)


def check_epilogues(q3, c, taps_on=True):
    """EPI_NONE / EPI_RES / EPI_SNAKE of the device's own accumulators, as tests/test_gpu_codec_gemm.py::test_epilogues_isolated does"""
    p = check_case(q3, c, taps_on)
    M, N = c[1], c[2]
    rng = np.random.default_rng(5)
    acc = p.run(q3)
    bias = rng.standard_normal(N).astype(np.float32) * 0.5
    ea, ib = rng.uniform(0.5, 2.0, N).astype(np.float32), rng.uniform(0.25, 1.0, N).astype(np.float32)
    ldr, r_segT = N + 4, 40
    r_skip = 5 * ldr
    res_idx = R.out_index(M, N, ldr, 0, r_segT, r_skip)
    res = rng.standard_normal(res_idx.max() + 1 + ldr).astype(np.float32)
    res_rows = res[res_idx].astype(np.float64)
    v = acc.astype(np.float64) + bias.astype(np.float64)
    for epi in (R.EPI_NONE, R.EPI_RES, R.EPI_SNAKE):
        out = p.run(q3, epi=epi, bias=bias, res=res, ldr=ldr, r_segT=r_segT, r_skip=r_skip, ea=ea, ib=ib)
        ref = R.epilogue(acc, epi, bias, res_rows, None, ea, ib)
        mag = np.maximum(np.abs(ref), np.abs(v))
        if epi == R.EPI_RES:
            mag = np.maximum(mag, np.abs(res_rows))
        tol = 4 * _ulp(mag) + (2e-7 if epi == R.EPI_SNAKE else 0.0)
        err = np.abs(out.astype(np.float64) - ref)
        assert np.all(err <= tol), "epi %d: max err %.3g (tol there %.3g)" % (epi, err.max(), tol.ravel()[np.argmax(err - tol)])


def main():
    """the child process: every case with the switch as the environment sets it (the test sets Q3_CODEC_H3_TAPS=0); prints one line per failure"""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "qwen3-tts-rust_amd", "python"))
    import q3tts
    taps_on = os.environ.get("Q3_CODEC_H3_TAPS", "1") != "0"
    failed = 0
    for c in CASES + EPI_CASES:
        try:
            if c in EPI_CASES:
                check_epilogues(q3tts, c, taps_on)
            else:
                check_case(q3tts, c, taps_on)
        except AssertionError as e:
            failed += 1
            print("FAILED %s: %s" % (case_id(c), e))
    print("%d cases, %d failed, tap reuse %s" % (len(CASES) + len(EPI_CASES), failed, "on" if taps_on else "off"))
    return 1 if failed else 0


if __name__ == "__main__":
    raise SystemExit(main())
