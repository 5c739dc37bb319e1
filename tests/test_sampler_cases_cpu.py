"""The selection-kernel cases (tests/sampler_cases.py) on the CPU: every family's self-check, and three implementations of
LlamaSampler::sample (llama/mod.rs:666-776) held against each other on every case, draw for draw -- the numpy restatement
tests/sampler_ref.py, the C oracle's q3o_sample, and the product's host q3tts_sampler_sample (host_logic.cpp), the last at draw counter 0,
the only place its C ABI can start a stream.  tests/test_gpu_sampler.py holds the device kernels against the same cases."""
import numpy as np
import pytest

import sampler_cases as SC
import sampler_ref as SR

ALL_NS = sorted(set(SC.PRED_NS + SC.TALK_NS))


def _oracle_tokens(oracle, row, T, k, p, seed, draw0, n_draws):
    st = SR.oracle_state(T, k, p, seed, draw0)
    return [oracle.sample(row, 0, row.size, state=st)[0] for _ in range(n_draws)]


def _host_tokens(q3, row, T, k, p, seed, n_draws):
    s = q3.Sampler(float(T), int(k), float(p), int(seed))
    try:
        return [s.sample(row) for _ in range(n_draws)]
    finally:
        s.close()


def test_reference_building_blocks(oracle, q3):
    rng = np.random.default_rng(3)
    x = rng.random(3000).astype(np.float32)
    s = np.float32(0)
    loop = []
    for v in x:                                                     # the strict left-to-right f32 sum the reference's iterators compute
        s = np.float32(s + v)
        loop.append(s)
    assert np.array_equal(np.add.accumulate(x, dtype=np.float32), np.array(loop, np.float32))
    assert np.add.accumulate(x, dtype=np.float32)[-1] != np.float32(np.sum(x.astype(np.float64)))   # and the order is visible at this length
    # a stream entered at word draw0 is the tail of the stream read from word 0
    words = SR.rng_words(12345, 0, 70)
    for d0 in (0, 1, 15, 16, 17, 31, 32, 47):
        assert SR.rng_words(12345, d0, 20) == words[d0:d0 + 20]
    big = SR.rng_words(12345, 1000003, 20)
    assert big != words[:20] and SR.rng_words(12345, 1000000, 23)[3:] == big
    # the keys of sampler_cases are the library's
    for v in (0.0, -0.0, 1e-45, -1e-45, 1e-38, -1e-38, 1.25, -3.5, np.inf, -np.inf):
        for i in (0, 1, 2047, 4095):
            assert SC.pack_key(v, i) == q3.argmax_key(v, i)
    assert np.float32(SC.TOP_PS[3]) < np.float32(1) and np.float32(SC.TOP_PS[3]) == np.nextafter(np.float32(1), np.float32(0))


@pytest.mark.parametrize("n", ALL_NS)
def test_families_and_three_way_agreement(oracle, q3, n):
    cases = SC.sampling_cases(n)                                    # building them runs every family's self-check
    assert [c.name for c in cases] == ["typical", "constant", "two_level", "ladder", "tiny_mixed", "tiny_zero_max", "inf_all_but_one",
                                       "inf_all_but_three", "inf_all", "inf_plus_1", "inf_plus_2", "spread"]
    host_checked = 0
    for ci, c in enumerate(cases):
        for T, k, p, draw0, seed in SC.configs(n, c.extra_top_k, ci):
            want = c.ref().sample(T, k, p, seed, draw0, SC.N_DRAWS)
            assert _oracle_tokens(oracle, c.row, T, k, p, seed, draw0, SC.N_DRAWS) == want, (c.name, T, k, p, draw0)
            if draw0 == 0:
                assert _host_tokens(q3, c.row, T, k, p, seed, SC.N_DRAWS) == want, (c.name, T, k, p)
                host_checked += 1
    assert host_checked >= 8 * len(cases)                           # a fifth of the configs start at word 0, at least 8 per case


@pytest.mark.parametrize("n", ALL_NS)
def test_greedy_cases_three_way(oracle, q3, n):
    for c in SC.greedy_cases(n):
        row = c.masked_row()
        for start, end, add in SC.ARGMAX_WINDOWS(n):
            if not 0 <= start <= end <= n:
                continue
            want = SR.greedy(row, start, end)
            st = SR.oracle_state(0.0, 0, 1.0, 1)
            assert oracle.sample(row, start, end, state=st)[0] == want, (c.name, start, end)
            s = q3.Sampler(0.0, 0, 1.0, 1)
            assert s.sample(row, start, end) == want, (c.name, start, end)
            s.close()
        if c.name in ("inf_all", "only_finite_masked"):
            assert SR.greedy(row) == 0 and SR.greedy(row, min(6, n), n) == min(6, n)    # nothing beats -inf: `start`
        if c.name == "max_masked":
            assert n == 1 or SR.greedy(row) != c.mask


def test_configs_cover_the_grids():
    for n in ALL_NS:
        cfg = SC.configs(n)
        assert len(cfg) == len(set(cfg))
        assert {c[0] for c in cfg} == set(SC.TEMPS) and {c[2] for c in cfg} == set(SC.TOP_PS) and {c[3] for c in cfg} == set(SC.DRAW0S)
        assert {c[1] for c in cfg} == {k for k in SC.top_ks(n) if k >= 0} | {0, 1, 50, n + 1}
        for k in SC.top_ks(n):
            if k >= 0:
                assert {c[0] for c in cfg if c[1] == k and c[0] > 0} == set(SC.TEMPS[1:])
                assert {c[2] for c in cfg if c[1] == k and c[0] > 0} == set(SC.TOP_PS)
