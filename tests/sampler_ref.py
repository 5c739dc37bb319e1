"""Plain numpy restatement of LlamaSampler::sample (the reference's src/models/llama/mod.rs:666-776), the yardstick of the selection-kernel
tests.  TEST INFRASTRUCTURE ONLY.

  T <= 0 : the first maximum under a strict `>` from -inf, `start` when nothing beats -inf                           (:690-701)
  T  > 0 : stable sort on descending value (Python's sorted on -value: -0.0 == +0.0, equal values keep index order)   (:705-708)
           -> top-k cut (0 < top_k < len)                                                                            (:711-713)
           -> e_i = exp((l_i - l_0) / T) in f32, exp = the spec's q3_expf through the oracle's q3o_spec_expf_n        (:716-723)
           -> sum left to right in f32; divide when sum > 0                                                          (:726-731)
           -> top_p < 1: first prefix whose running f32 sum is >= top_p, kept inclusive; renormalise when > 0        (:734-753)
           -> r = f32(u32) / 2^32 (`u32::MAX as f32` rounds to 2^32); first i with r < cum_i, else candidate 0       (:761-774)

Sums are np.add.accumulate over f32, which is by definition r[i] = r[i-1] + a[i], one f32 rounding per step; np.sum adds pairwise and must
not be used (tests/test_sampler_cases_cpu.py holds accumulate against an explicit loop).  Random words are the oracle's q3o_rng_* stream
(pinned by test_chacha12_known_answer); a stream starts at any draw counter by setting the state's block counter and word index.

NaN logits are out of scope: the reference's comparator maps an unordered pair to Equal, which is no order, so the sorted sequence depends
on the sort algorithm and no contract exists to test.  +-inf, +-0.0 and subnormals are in scope.
"""
import ctypes as C

import numpy as np

import q3oracle
from gen_loop_ref import penalise  # noqa: F401  (the penalty half of the reference, re-exported)


class Rng(C.Structure):  # oracle/q3o.h q3o_rng
    _fields_ = [("key", C.c_uint32 * 8), ("counter", C.c_uint64), ("buf", C.c_uint32 * 16), ("idx", C.c_int)]


class SamplerState(C.Structure):  # oracle/q3o.h q3o_sampler
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int), ("top_p", C.c_float), ("rng", Rng)]


def _seek(rng, draw0):
    """position a seeded stream at word draw0: block draw0 / 16, word draw0 % 16"""
    rng.counter = draw0 >> 4
    rng.idx = 16
    if draw0 & 15:
        q3oracle.lib().q3o_rng_next_u32(C.byref(rng))   # generates block draw0 / 16
        rng.idx = draw0 & 15


def rng_words(seed, draw0, count):
    """words draw0 .. draw0 + count - 1 of seed_from_u64(seed)'s stream"""
    r = Rng()
    q3oracle.lib().q3o_rng_seed(C.byref(r), C.c_uint64(int(seed)))
    _seek(r, int(draw0))
    return [int(q3oracle.lib().q3o_rng_next_u32(C.byref(r))) for _ in range(count)]


def oracle_state(temperature, top_k, top_p, seed, draw0=0):
    """a q3oracle.sample state whose stream starts at word draw0"""
    buf = C.create_string_buffer(256)
    q3oracle.lib().q3o_sampler_init(buf, float(temperature), int(top_k), float(top_p), int(seed))
    _seek(SamplerState.from_buffer(buf).rng, int(draw0))
    return buf


def expf(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.zeros_like(x)
    L = q3oracle.lib()
    L.q3o_spec_expf_n.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    L.q3o_spec_expf_n(x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.size)
    return y


def greedy(logits, start=0, end=None):
    lg = np.asarray(logits, np.float32)
    end = lg.size if end is None else min(end, lg.size)
    best, idx = np.float32(-np.inf), start
    for i in range(start, end):
        if lg[i] > best:
            best, idx = lg[i], i
    return idx


class Row:
    """one logits row: the sort is done once, every (T, top_k, top_p) is a cut of it"""

    def __init__(self, logits):
        self.lg = np.array(logits, np.float32, copy=True)
        assert not np.isnan(self.lg).any(), "NaN rows are out of scope"
        neg = (-self.lg.astype(np.float64)).tolist()
        self.order = np.array(sorted(range(self.lg.size), key=neg.__getitem__), np.int64)
        self._greedy = greedy(self.lg)
        self._dist = {}

    def dist(self, T, top_k, top_p):
        """(candidate indices, their running f32 sums) after top-k, softmax and top-p"""
        key = (float(T), int(top_k), float(np.float32(top_p)))
        if key not in self._dist:
            T32, p32 = np.float32(T), np.float32(top_p)
            order = self.order
            if 0 < top_k < order.size:
                order = order[:top_k]
            l = self.lg[order]
            with np.errstate(invalid="ignore", over="ignore"):
                prob = expf((l - l[0]) / T32)
                s = np.add.accumulate(prob, dtype=np.float32)[-1]
                if s > 0:
                    prob = prob / s
                if p32 < np.float32(1.0):
                    cum = np.add.accumulate(prob, dtype=np.float32)
                    hit = np.nonzero(cum >= p32)[0]
                    cut = int(hit[0]) + 1 if hit.size else prob.size
                    order, prob = order[:cut], prob[:cut]
                    ns = cum[cut - 1]
                    if ns > 0:
                        prob = prob / ns
                self._dist[key] = (order, np.add.accumulate(prob, dtype=np.float32))
        return self._dist[key]

    def sample(self, T, top_k, top_p, seed, draw0=0, n_draws=1):
        """n_draws consecutive tokens from word draw0 of the seed's stream on; greedy rows consume nothing"""
        if np.float32(T) <= 0:
            return [self._greedy] * n_draws
        order, cum = self.dist(T, top_k, top_p)
        out = []
        for w in rng_words(seed, draw0, n_draws):
            r = np.float32(np.uint32(w)) / np.float32(4294967296.0)
            hit = np.nonzero(r < cum)[0]
            out.append(int(order[hit[0]]) if hit.size else int(order[0]))
        return out


def sample(logits, T, top_k, top_p, seed, draw0=0, n_draws=1):
    return Row(logits).sample(T, top_k, top_p, seed, draw0, n_draws)
