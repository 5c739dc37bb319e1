"""The float64 mel reference (tests/mel_ref.py) checked without a GPU: the library's tables against their float64 definition, the frame
count against the library and the oracle, the oracle against the reference, the straddle cap of every case, and the power of the cases over
nine mutants of the reference.

Table bounds are derived in mel_ref.py's docstring (Hann 8u; filterbank norm (6 e / D + 8u) with e = 64u fr).

Power.  A mutant is the reference with one deliberate defect; it is "caught" when some case's mutant output leaves the reference's bound by a
factor of 10 or more (mel_ref.excess >= 10).  Measured worst excess per mutant: drop_512 6e6, twiddle_k1 9e5, hann_symmetric 3e6, no_eps 128
(faint_noise_512), left_pad_im1 2e5, right_pad_nm1 4e4 (impulse_0_256), floor_1e6 2e6 (silence).  Two mutants cannot be caught by any input,
because on this filterbank they change no table entry, and the test asserts exactly that instead of a factor:
  fc_strict    `freq < fc` differs from `freq <= fc` only for a bin that lies exactly on a filter centre.  Every bin frequency is more than
               10 f32 edge errors e = 64u fc (and at least 0.08 Hz) away from every centre, so no centre of the library's table is a bin.
  fb_stop_512  the Nyquist bin (12000 Hz) is the upper edge of the last filter, where the ramp is 0: column 512 of the table is all zeros."""
import numpy as np
import pytest

import mel_cases
import mel_ref as R

@pytest.fixture(scope="module")
def tables(q3):
    return q3.mel_tables()


@pytest.fixture(scope="module")
def refs(tables):
    """case -> (v, ln, dv) of the unmutated reference, computed once"""
    return {name: R.mel64(a, *tables) for name, a in mel_cases.CASES}


def test_tables_against_float64(tables):
    hann, fb = tables
    h64, f64 = R.tables64()
    hb, fbb = R.table_bounds()
    eh, ef = np.abs(hann - h64).max() / hb, (np.abs(fb - f64) / fbb).max()
    print("hann error / bound %.3g, filterbank error / bound %.3g" % (eh, ef))
    assert eh <= 1 and ef <= 1
    assert hann[0] == 0.0 and hann[512] == 1.0 and hann.min() >= 0 and hann.max() <= 1     # periodic: the peak is sample 512, not 511.5
    assert np.all(fb >= 0)
    for m in range(R.N_MELS):
        nz = np.nonzero(fb[m])[0]
        assert nz.size >= 1 and nz[-1] - nz[0] + 1 == nz.size, m
        assert np.array_equal(nz, np.nonzero(f64[m])[0]), m      # the same support as the float64 definition


def test_frame_count_agrees_everywhere(q3, oracle):
    for n in range(2101):
        want = R.frames(n)
        assert q3.mel_frames(n) == want, n
        assert oracle.mel(np.zeros(n, np.float32)).shape[0] == want, n
    assert q3.mel_frames(-1) == 0


def test_padding_by_hand():
    """padded() on a 3-sample clip, worked by hand: the left pad reads audio[2], audio[1] and zeros before them, the right pad audio[1], audio[0]
    and then audio[0] again where the index saturates."""
    assert np.array_equal(R.padded(np.arange(1, 4, dtype=np.float32))[381:390], [0, 3, 2, 1, 2, 3, 2, 1, 1])


@pytest.mark.parametrize("name", mel_cases.NAMES)
def test_oracle_against_float64(name, oracle, tables, refs):
    a = mel_cases.AUDIO[name]
    got = oracle.mel(a)
    v, _, dv = R.mel64(a, *tables, bin_bound="oracle")
    assert got.shape == (R.frames(a.size), 128) == v.shape
    e = R.excess(got, v, dv)
    print("%s: oracle error / bound %.3g" % (name, e))
    assert e <= 1


@pytest.mark.parametrize("name", mel_cases.NAMES)
def test_straddle_cap(name, refs):
    v, _, dv = refs[name]
    assert v.shape == (R.frames(mel_cases.AUDIO[name].size), 128)
    if v.size:
        share = R.classify(v, dv)[2].mean()
        print("%s: straddle share %.4f" % (name, share))
        assert share <= 0.01


def test_rfft_is_the_direct_dft(tables):
    xs = R.windowed(mel_cases.AUDIO["noise_512"], tables[0])
    c, s, _, _ = R._twiddles()
    re, im = R.spectrum(xs)
    assert np.abs(xs @ c.T - re).max() < 1e-11 and np.abs(-(xs @ s.T) - im).max() < 1e-11


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_cases_catch_mutant(mutant, tables, refs):
    hann, fb = tables
    if mutant == "fc_strict":
        centres = R.mel_edges64()[1:-1]
        freq = np.arange(R.N_BINS) * (R.SR / R.N_FFT)
        gap = np.abs(freq[:, None] - centres[None, :])
        assert np.all(gap > 10 * 64 * R.U * centres[None, :])     # measured: at least 13 edge errors (0.084 Hz) away
        assert np.array_equal(R.tables64(mutant)[1], R.tables64()[1])
        return
    if mutant == "fb_stop_512":
        assert np.all(fb[:, 512] == 0) and np.all(R.tables64()[1][:, 512] == 0)
        return
    worst, at = 0.0, None
    for name, a in mel_cases.CASES:
        v, _, dv = refs[name]
        if v.size == 0:
            continue
        e = R.excess(R.mel64(a, hann, fb, bin_bound=None, mutant=mutant)[1], v, dv)
        if e > worst:
            worst, at = e, name
    print("%s: worst excess %.3g at %s" % (mutant, worst, at))
    assert worst >= 10
