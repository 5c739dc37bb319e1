"""Row families and configuration grids shared by tests/test_sampler_cases_cpu.py and tests/test_gpu_sampler.py.  TEST INFRASTRUCTURE ONLY.

Every family is built from a seed and asserts, where it is built, that the situation it stands for really occurs in the row (the asserts
that need more elements than a small n has are skipped there; the row is still built and still run).  The situations are those the sort keys
(kdev.h pack_key: order-preserving value word, ~index word) and k_sample_pred's radix select, compaction and bitonic sort can get wrong:

  typical    random normals with planted ties at the top, a run of equal values and a few -inf  (the rows the older tests use)
  constant   every logit equal: all value words equal, the select walks every value digit and ends in the index word
  two_level  value a at ~n/3 scattered indices, b < a elsewhere: top_k cuts inside the a run, at its end and inside the b run
  ladder     np.nextafter steps from 1.0, each rung at 3 scattered indices: keys differ in the lowest value byte only
  tiny       +-0.0, +-subnormals, +-1e-38: keys on both sides of pack_key's sign fold; a -0.0 below a +0.0 wins the tie
  inf_flood  all -inf but one / but three / all -inf / one +inf / two +inf
  spread     ties at 0, the rest 5 to 200 below: at T = 0.05 everything but the ties underflows to probability 0
  greedy tie placements: equal maxima 64 / 256 / 1024 apart, at 0 and n-1, the maximum masked, the only finite entry masked

NaN logits are out of scope (tests/sampler_ref.py says why).
"""
import zlib

import numpy as np

import sampler_ref

PRED_NS = (1, 2, 255, 256, 257, 1000, 2047, 2048)      # k_sample_pred: 8 keys per thread at tid + 256*j; 2047 leaves a single pad
TALK_NS = (1, 33, 300, 2160, 4095, 4096)               # k_sample
TEMPS = (0.0, 0.05, 0.9, 1.3)
TOP_PS = (1e-9, 0.5, 0.8, float(np.float32(1) - np.float32(2.0 ** -24)), 1.0)
DRAW0S = (0, 15, 16, 31, 1000003)
N_DRAWS = 6                                            # from word 15 or 31 on this crosses a ChaCha block
ARGMAX_WINDOWS = lambda n: ((0, n, 0), (6, n - 3, 0), (0, n, 7))


def top_ks(n):
    """the power-of-two edges of the candidate sort and the edges of `0 < top_k < n`"""
    return (0, 1, 2, 50, 64, 65, 1024, 1025, n - 1, n, n + 1)


def strides(n):
    return (n, n + 1, (n + 15) // 16 * 16 + 16)


def key_hi(v):
    """value word of pack_key: -0.0 folded onto +0.0, negatives complemented, the rest with the sign bit set"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).copy()
    b[b == 0x80000000] = 0
    return np.where(b & 0x80000000, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def pack_key(v, idx):
    return (int(key_hi(np.array([v], np.float32))[0]) << 32) | (~int(idx) & 0xFFFFFFFF)


def _rng(name, n, seed):
    return np.random.default_rng([zlib.crc32(name.encode()), n, seed])


def _scatter(rng, n, m):
    return np.sort(rng.permutation(n)[:m])


class Case:
    def __init__(self, name, row, extra_top_k=(), mask=-1):
        self.name, self.row, self.extra_top_k, self.mask = name, np.ascontiguousarray(row, np.float32), tuple(extra_top_k), mask
        assert self.row.ndim == 1 and not np.isnan(self.row).any()
        self._ref = None

    @property
    def n(self):
        return self.row.size

    def masked_row(self):
        r = self.row.copy()
        if self.mask >= 0:
            r[self.mask] = -np.inf
        return r

    def ref(self):
        """the shared sampler_ref.Row of the (masked) row: sorted once, left unchanged"""
        if self._ref is None:
            self._ref = sampler_ref.Row(self.masked_row())
        return self._ref


def typical(n, seed=0):
    rng = _rng("typical", n, seed)
    lg = (rng.standard_normal(n) * 3).astype(np.float32)
    lg[rng.choice(n, min(5, n), replace=False)] = lg.max()
    lg[rng.choice(n, min(40, n // 4), replace=False)] = np.float32(0.5)
    lg[rng.choice(n, min(3, n // 8), replace=False)] = -np.inf
    if n >= 33:
        assert (lg == lg.max()).sum() >= 2 and np.isneginf(lg).any() and (lg == np.float32(0.5)).sum() >= 2
    return [Case("typical", lg)]


def constant(n, seed=0):
    c = Case("constant", np.full(n, 1.25, np.float32))
    assert np.unique(key_hi(c.row)).size == 1                      # nothing but the index word tells two keys apart
    if n > 50:
        order, _ = c.ref().dist(0.9, 50, 1.0)
        assert np.array_equal(order, np.arange(50))                 # top_k = 50 keeps exactly indices 0..49, in order
    return [c]


def two_level(n, seed=0):
    rng = _rng("two_level", n, seed)
    m = max(1, n // 3)
    lg = np.full(n, 1.0, np.float32)
    lg[_scatter(rng, n, m)] = 2.0
    ks = [k for k in (m // 2, m, m + (n - m) // 2) if 0 < k < n]    # inside the a run, exactly at its end, inside the b run
    if n >= 6:
        assert len(set(ks)) == 3 and (lg == 2.0).sum() == m and ks[0] < m < ks[2] and np.unique(key_hi(lg)).size == 2
    return [Case("two_level", lg, extra_top_k=ks)]


def ladder(n, seed=0):
    rng = _rng("ladder", n, seed)
    rungs = max(1, min(n // 3, 40))
    vals = [np.float32(1.0)]
    for _ in range(rungs - 1):
        vals.append(np.nextafter(vals[-1], np.float32(np.inf), dtype=np.float32))
    lg = np.empty(n, np.float32)
    for j, i in enumerate(rng.permutation(n)):
        lg[i] = vals[min(j // 3, rungs - 1)]
    hi = key_hi(lg)
    assert np.unique(hi >> 8).size == 1 and np.unique(hi & 0xFF).size == rungs   # the keys part in the lowest value byte, nowhere above
    if n >= 6:
        assert rungs >= 2 and all((lg == v).sum() >= 3 for v in vals)
    return [Case("ladder", lg, extra_top_k=[k for k in (4, 3 * rungs - 1) if 0 < k < n])]


def tiny(n, seed=0):
    rng = _rng("tiny", n, seed)
    allv = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 5e-39, -5e-39], np.float32)
    assert allv[2] > 0 and allv[6] < np.finfo(np.float32).tiny      # subnormals survive the conversion
    mixed = allv[rng.integers(0, 8, n)]
    nonpos = np.array([0.0, -0.0, -1e-45, -1e-38, -5e-39], np.float32)
    zmax = nonpos[rng.integers(0, 5, n)]
    if n == 1:
        zmax[0] = -0.0
        i = 0
    else:
        i, j = _scatter(rng, n, 2)
        zmax[:i][zmax[:i] == 0] = np.float32(-1e-38)
        zmax[i], zmax[j] = -0.0, 0.0
        assert np.signbit(zmax[i]) and not np.signbit(zmax[j]) and i < j
    assert sampler_ref.greedy(zmax) == i                            # the -0.0 at the lower index wins the tie against +0.0
    assert pack_key(-0.0, 5) == pack_key(0.0, 5)
    if n >= 33:
        hi = key_hi(mixed)
        assert (hi > 0x80000000).any() and (hi < 0x80000000).any() and (hi == 0x80000000).any()   # both sides of the sign fold, and on it
    return [Case("tiny_mixed", mixed), Case("tiny_zero_max", zmax)]


def inf_flood(n, seed=0):
    rng = _rng("inf_flood", n, seed)
    out = []
    one = np.full(n, -np.inf, np.float32)
    one[rng.integers(0, n)] = 0.5
    out.append(Case("inf_all_but_one", one))
    three = np.full(n, -np.inf, np.float32)
    three[_scatter(rng, n, min(3, n))] = np.array([1.0, 0.5, 0.5], np.float32)[: min(3, n)]
    out.append(Case("inf_all_but_three", three))                    # with top_k = 50: 47 candidates of probability 0
    out.append(Case("inf_all", np.full(n, -np.inf, np.float32)))
    for cnt in (1, 2):
        lg = (rng.standard_normal(n) * 3).astype(np.float32)
        lg[_scatter(rng, n, min(cnt, n))] = np.inf
        out.append(Case("inf_plus_%d" % cnt, lg))
    assert np.isfinite(one).sum() == 1 and np.isfinite(three).sum() == min(3, n) and np.isposinf(out[4].row).sum() == min(2, n)
    return out


def spread(n, seed=0):
    rng = _rng("spread", n, seed)
    lg = rng.uniform(-200.0, -5.0, n).astype(np.float32)
    ties = _scatter(rng, n, min(3, n))
    lg[ties] = 0.0
    rest = np.setdiff1d(np.arange(n), ties)
    if rest.size >= 2:
        lg[rest[0]], lg[rest[-1]] = -200.0, -5.0
        assert lg.min() == -200.0
    assert (sampler_ref.expf(lg[rest] / np.float32(0.05)) == 0).all()   # at T = 0.05 only the ties keep a probability
    return [Case("spread", lg)]


FAMILIES = (typical, constant, two_level, ladder, tiny, inf_flood, spread)


def sampling_cases(n, seed=0):
    return [c for f in FAMILIES for c in f(n, seed)]


def greedy_cases(n, seed=0):
    """tie placements for the greedy paths, then the tiny and inf_flood rows"""
    rng = _rng("greedy", n, seed)
    base = lambda: (rng.standard_normal(n) * 3).astype(np.float32)
    out = []
    for off in (64, 256, 1024):                                     # one wave, one pass of 256 threads, one pass of 1024 threads apart
        if off < n:
            lg = base()
            i = int(rng.integers(0, n - off))
            lg[i] = lg[i + off] = lg.max() + 1
            assert sampler_ref.greedy(lg) == i
            out.append(Case("tie_%d" % off, lg))
    lg = base()
    lg[0] = lg[n - 1] = lg.max() + 1
    out.append(Case("max_at_0_and_last", lg))
    lg = base()
    lg[n - 1] = lg.max() + 1
    assert sampler_ref.greedy(lg) == n - 1
    out.append(Case("max_at_last", lg))
    lg = base()
    out.append(Case("max_masked", lg, mask=int(np.argmax(lg))))
    lg = np.full(n, -np.inf, np.float32)
    j = int(rng.integers(0, n))
    lg[j] = 1.0
    out.append(Case("only_finite_masked", lg, mask=j))
    assert np.isneginf(out[-1].masked_row()).all()
    return out + tiny(n, seed) + inf_flood(n, seed)


def configs(n, extra_top_k=(), tag=0):
    """[(T, top_k, top_p, draw0, seed)]: every top_k with every T > 0 and every top_p, the five draw0 rotating under them (the starting
    word only moves the random stream, so each draw0 meets each top_k, T and top_p rather than each triple); then greedy rows, whose draw
    counters must stay put"""
    ks = []
    for k in tuple(top_ks(n)) + tuple(extra_top_k):
        if k >= 0 and k not in ks:
            ks.append(k)
    out = []
    for ki, k in enumerate(ks):
        for ti, T in enumerate(TEMPS[1:]):
            for j, p in enumerate(TOP_PS):
                out.append((T, k, p, DRAW0S[(j + ti + 2 * ki) % 5]))
    out += [(0.0, 0, 1.0, 0), (0.0, 50, 0.5, 15), (0.0, 1, 1e-9, 31), (0.0, n + 1, 0.8, 1000003)]
    return [c + (0x9E3779B97F4A7C15 * (i + 1) + 1000 * n + tag & (2 ** 63 - 1),) for i, c in enumerate(out)]
