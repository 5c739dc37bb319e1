"""Q4_K helpers for the tests: random raw rows, the Q5_K twin of a row (spec S3: a Q4_K row is the Q5_K row with bit 4 of every weight clear)
and a float64 decoder written from the public ggml block format {f16 d, f16 dmin, u8 scales[12], u8 qs[128]} (144 bytes, 256 weights)."""
import numpy as np


def rand_rows_q4k(rng, n, k, scale=1.0):
    """n rows of k weights as raw Q4_K super-blocks with RANDOM fields (every bit pattern of nibbles, scales and mins is a valid block)"""
    nsb = n * (k // 256)
    f16u = lambda lo, hi: rng.uniform(lo * scale, hi * scale, nsb).astype(np.float16).view(np.uint16).view(np.uint8).reshape(-1, 2)
    blk = rng.integers(0, 256, (nsb, 144), dtype=np.uint8)
    blk[:, 0:2] = f16u(0.0005, 0.01); blk[:, 2:4] = f16u(0.0005, 0.01)
    return blk.reshape(-1)


def widen(raw):
    """Q4_K bytes -> the Q5_K bytes of the same row: 32 zero bytes (qh) at offset 16 of every block"""
    b = np.ascontiguousarray(raw, np.uint8).reshape(-1, 144)
    return np.concatenate([b[:, :16], np.zeros((b.shape[0], 32), np.uint8), b[:, 16:]], axis=1).reshape(-1)


def dec_q4_k(raw, n, k):
    """-> (a, b), w = a - b, shape [n][k]: block j of a super-block takes the low (j even) or high (j odd) nibbles of qs[32 (j / 2) ..+32);
    its 6-bit scale and min come from scales[12] as ggml's get_scale_min_k4 unpacks them"""
    blk = np.ascontiguousarray(raw, np.uint8).reshape(n * (k // 256), 144)
    d = blk[:, 0:2].copy().view(np.float16).astype(np.float64)[:, 0]
    dmin = blk[:, 2:4].copy().view(np.float16).astype(np.float64)[:, 0]
    s = blk[:, 4:16].astype(np.int64)
    qs = blk[:, 16:144].astype(np.int64)
    a = np.zeros((blk.shape[0], 8, 32)); b = np.zeros_like(a)
    for j in range(8):
        if j < 4:
            sc, m = s[:, j] & 63, s[:, j + 4] & 63
        else:
            sc, m = (s[:, j + 4] & 0xF) | ((s[:, j - 4] >> 6) << 4), (s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4)
        q = (qs[:, 32 * (j // 2):32 * (j // 2) + 32] >> (4 * (j & 1))) & 0xF
        a[:, j] = (d * sc)[:, None] * q
        b[:, j] = (dmin * m)[:, None]
    return a.reshape(n, k), b.reshape(n, k)
