"""Q3_K helpers for the tests: random raw rows, a float64 decoder written from the block definition {u8 hmask[32], u8 qs[64], u8 scales[12],
f16 d} (110 bytes, 256 weights; spec S3 [EXT]) and the Q6_K twin of a row (the same d, scales - 32 and quants in a 210-byte Q6_K block)."""
import numpy as np


def rand_rows_q3k(rng, n, k, scale=1.0):
    """n rows of k weights as raw Q3_K super-blocks with RANDOM fields (every bit pattern of the planes and the scales is a valid block)"""
    nsb = n * (k // 256)
    blk = rng.integers(0, 256, (nsb, 110), dtype=np.uint8)
    blk[:, 108:110] = rng.uniform(0.0005 * scale, 0.01 * scale, nsb).astype(np.float16).view(np.uint16).view(np.uint8).reshape(-1, 2)
    return blk.reshape(-1)


def fields(raw):
    """-> (d [nsb] float64, s [nsb][16] = s6 - 32, q [nsb][256] in -4..3), weight e = 128 h + 32 g + l"""
    blk = np.ascontiguousarray(raw, np.uint8).reshape(-1, 110).astype(np.int64)
    hmask, qs, sc = blk[:, 0:32], blk[:, 32:96], blk[:, 96:108]
    d = np.ascontiguousarray(raw, np.uint8).reshape(-1, 110)[:, 108:110].copy().view(np.float16).astype(np.float64)[:, 0]
    q = np.zeros((blk.shape[0], 256), np.int64)
    for h in range(2):
        for g in range(4):
            low2 = (qs[:, 32 * h:32 * h + 32] >> (2 * g)) & 3
            q[:, 128 * h + 32 * g:128 * h + 32 * g + 32] = low2 - np.where((hmask >> (4 * h + g)) & 1, 0, 4)
    s6 = np.zeros((blk.shape[0], 16), np.int64)
    for j in range(4):
        s6[:, j] = (sc[:, j] & 15) | ((sc[:, 8 + j] & 3) << 4)
        s6[:, 4 + j] = (sc[:, 4 + j] & 15) | (((sc[:, 8 + j] >> 2) & 3) << 4)
        s6[:, 8 + j] = (sc[:, j] >> 4) | (((sc[:, 8 + j] >> 4) & 3) << 4)
        s6[:, 12 + j] = (sc[:, 4 + j] >> 4) | (((sc[:, 8 + j] >> 6) & 3) << 4)
    return d, s6 - 32, q


def dec_q3_k(raw, n, k):
    """-> (a, b), w = a - b with b = 0, shape [n][k]: w[e] = d * (s6[e / 16] - 32) * q[e]"""
    d, s, q = fields(raw)
    y = (d[:, None] * np.repeat(s, 16, axis=1) * q).reshape(n, k)
    return y, np.zeros_like(y)


def widen_to_q6k(raw):
    """Q3_K bytes -> the Q6_K bytes {u8 ql[128], u8 qh[64], i8 scales[16], f16 d} of the same row: quants q + 32, nothing re-quantised"""
    src = np.ascontiguousarray(raw, np.uint8).reshape(-1, 110)
    _, s, q = fields(raw)
    u = (q + 32).reshape(-1, 2, 4, 32)                       # [block][half n][group][l]: Q6_K weight 128 n + 32 group + l
    out = np.zeros((src.shape[0], 210), np.uint8)
    for n in range(2):
        out[:, 64 * n:64 * n + 32] = (u[:, n, 0] & 15) | ((u[:, n, 2] & 15) << 4)
        out[:, 64 * n + 32:64 * n + 64] = (u[:, n, 1] & 15) | ((u[:, n, 3] & 15) << 4)
        out[:, 128 + 32 * n:160 + 32 * n] = (u[:, n, 0] >> 4) | ((u[:, n, 1] >> 4) << 2) | ((u[:, n, 2] >> 4) << 4) | ((u[:, n, 3] >> 4) << 6)
    out[:, 192:208] = s.astype(np.int8).view(np.uint8)
    out[:, 208:210] = src[:, 108:110]
    return out.reshape(-1)
