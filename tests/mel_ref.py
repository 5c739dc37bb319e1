"""float64 definition of the log-mel front end (csrc/mel.hip, k_mel) and the bound a correct f32 kernel stays inside.  numpy only.

Definition.  padded(audio) is the clip with 384 mirrored samples on either side (a sample the clip does not have reads 0 on the left and
audio[0] on the right, the reference's quirk); frame f is padded[256 f : 256 f + 1024] and exists only if it fits (frames(n) = 0 below 256
samples, n // 256 from there on).  xs = f32(padded * hann32) is ONE f32 multiply, exactly what the kernel stores in LDS, and everything after
it is float64: X = DFT(xs) (np.fft.fft on float64), mag = sqrt(re^2 + im^2 + f32(1e-9)), v = fb32 @ mag, out = ln(max(v, f32(1e-5))).
hann32 / fb32 are the library's own f32 tables (q3tts_mel_tables); tables64() is their float64 definition and test_mel_ref_cpu.py holds the
one to the other, so the kernel bound below has no table term.

Bound (u = 2^-24, gamma(n) = n u / (1 - n u)); first-order terms are written out and the second-order ones are covered by the factor
(1 + gamma(1024)) on the bin bound.
 (1) Bin k.  The kernel forms re = sum_n xs_n c_n in ascending n, c_n = cosf(ang32(n k mod 1024)), one rounded product and one rounded add per
     term (or one fma).  With p_n = xs_n cos(2 pi n k / 1024) and s_n = p_0 + .. + p_n in float64 (np.cumsum), the running-error bound of a
     recursive sum is u sum_n (|s_n| + |p_n|): each add contributes at most u |s_n|, each product at most u |p_n| (an fma chain drops the
     second part, so the bound covers it too).  The kernel's twiddle differs from the exact one by at most tau + 4u, tau = the largest
     |cos32(ang32_i) - cos(2 pi i / 1024)| (and the same for sin) over i in [0, 1024) with ang32_i = f32(f32(6.2831855f * f32(i)) / 1024)
     evaluated in numpy float32 as the kernel writes it, and 4u (2 ulp at 1) for the device's cosf / sinf differing from numpy's -- THE ONE
     ASSUMPTION of this bound.  That adds at most (tau + 4u) sum_n |xs_n|.  The tau part of it is taken at its actual value instead of its
     worst case: the numpy-f32 table's own errors dc_i = cos32(ang32_i) - cos(2 pi i / 1024) are known numbers, so their contribution is
     |sum_n xs_n dc_(n k mod 1024)| <= tau sum_n |xs_n|, computed per bin (tau is 6.8u; on a full-scale leakage-free signal the worst case
     alone would push every empty bin into the straddle class).  So d_re = (1 + gamma(1024)) (u sum_n (|s_n| + |p_n|) + |sum_n xs_n dc_n| +
     4u sum_n |xs_n|), and d_im likewise with sin.  On a leakage-free tone the partial sums of the empty bins stay near the tone's amplitude
     times a few hundred, so d_re is ~5e-5 there, where the worst case gamma(1024) sum |xs| would say 1e-2.
 (2) mag.  q = re^2 + im^2 + 1e-9 takes two products and two adds of non-negative terms: |q^ - q| <= d_q = 2 |re| d_re + d_re^2 + 2 |im| d_im +
     d_im^2 + gamma(4) (q + the same four terms).  sqrt is correctly rounded and |sqrt(a) - sqrt(b)| <= min(|a - b| / sqrt(b), sqrt(|a - b|)),
     so with d_s = min(d_q / sqrt(q), sqrt(d_q)):  d_mag = d_s + u (mag + d_s).  q >= 1e-9 keeps the quotient finite; the second form is the
     smaller one on an empty bin, where d_q exceeds q.
 (3) Filterbank.  v^ = sum_k w_k mag^_k is a recursive sum of 513 rounded products of non-negative terms:
     d_v = sum_k w_k d_mag_k + gamma(514) sum_k w_k mag_k.
 (4) Log.  With FLOOR = f32(1e-5):
       v - d_v > FLOOR   |got - ln v| <= d_v / (v - d_v) + 2u |ln v|     (ln is 1 / x-Lipschitz above v - d_v; logf within 1 ulp)
       v + d_v < FLOOR   got is logf(FLOOR) to 1 ulp
       otherwise         "straddle": got lies between those two ends, logf(FLOOR) - 1 ulp <= got <= ln(v + d_v) + 2u |ln(v + d_v)|
     A case may have at most 1 % of its outputs in the straddle class (asserted for every case in test_mel_ref_cpu.py).

The oracle (oracle/q3o_mel.c) runs a double-precision radix-2 FFT and rounds re / im to f32 before the same f32 magnitude and filterbank
chain.  oracle_bin_bound() is step (1) for that chain: a radix-2 FFT of 10 stages in double errs by at most gamma_64(4 * 10) sum_n |xs_n| per bin
(each stage is one complex multiply-add: 4 roundings on a path), plus u |re| for the cast; steps (2)-(4) are shared.

Table bounds (tables64 against q3tts_mel_tables), glibc's cosf / logf / expf taken as within 1 ulp (2u relative):
 Hann: ang = f32(f32(2 * pi32) * i) / 1024 has relative error (0.47 + 1) u (pi32, one product; the divisions by powers of two are exact), so
     |ang32 - ang| <= 1.5u 2 pi; cosf adds 2u, 1 - c adds 2u (|1 - c| <= 2), the factor 0.5 is exact: |hann32 - hann64| <= 0.5 (3 pi u + 4u) < 8u.
 Filterbank: every edge in Hz carries a relative error of at most E = 64u.  Chain: logstep = logf(6.4f) / 27 (3.6u), mel_max = 15 +
     logf(12) / logstep (<= 8u), mel_i = mel_max i / 129 (<= 11u relative, <= 600u absolute at 51.3), then either f_sp mel (13u) or
     1000 expf(logstep (mel - 15)): the exponent errs by at most 0.0687 * 600u + 2.49 * 4.6u = 53u absolute, expf and the product add 3u: 56u.
     The bin frequencies k * 23.4375 are exact in f32.  With e = E * fr the absolute edge error and D = min(fc - fl, fr - fc), the ramp
     (freq - fl) / (fc - fl) errs by at most 3 e / D + 3u, a bin within e of an edge may change sides (the ramps meet there, so that moves
     w by at most e / D), and norm = 2 / (fr - fl) errs relatively by 2 e / (fr - fl) + 2u:  |fb32 - fb64| <= norm (6 e / D + 8u)."""
import numpy as np

U = 2.0 ** -24
N_FFT, HOP, N_MELS, N_BINS, PAD, SR = 1024, 256, 128, 513, 384, 24000
FLOOR = np.float32(1e-5)
EPS = np.float32(1e-9)
LN_FLOOR32 = np.log(FLOOR)                       # f32, what logf(1e-5f) is to within 1 ulp
ULP_LN_FLOOR = float(np.spacing(np.abs(LN_FLOOR32)))

MUTANTS = ("drop_512", "twiddle_k1", "hann_symmetric", "no_eps", "left_pad_im1", "right_pad_nm1", "fc_strict", "fb_stop_512", "floor_1e6")


def gamma(n, u=U):
    return n * u / (1 - n * u)


def frames(n):
    return n // HOP if n >= HOP else 0


def padded(audio, mutant=None):
    a = np.ascontiguousarray(audio, np.float32)
    n = a.size
    out = np.zeros(n + 2 * PAD, np.float32)
    for j, i in enumerate(range(PAD, 0, -1)):           # left: audio[384] .. audio[1], 0 where the clip is shorter
        src = i - 1 if mutant == "left_pad_im1" else i
        out[j] = a[src] if i < n else 0.0
    out[PAD:PAD + n] = a
    for i in range(1, PAD + 1):                          # right: audio[n - 2] .. , saturating at index 0
        idx = n - 1 - i
        if idx < 0:
            idx = n - 1 if mutant == "right_pad_nm1" else 0
        out[PAD + n + i - 1] = a[idx] if 0 <= idx < n else 0.0
    return out


def _hz_to_mel(f):
    f = np.asarray(f, np.float64)
    return np.where(f >= 1000.0, 15.0 + np.log(np.maximum(f, 1e-300) / 1000.0) / (np.log(6.4) / 27.0), f * 3.0 / 200.0)


def _mel_to_hz(m):
    m = np.asarray(m, np.float64)
    return np.where(m >= 15.0, 1000.0 * np.exp((np.log(6.4) / 27.0) * (m - 15.0)), m * 200.0 / 3.0)


def mel_edges64():
    return _mel_to_hz(_hz_to_mel(12000.0) * np.arange(N_MELS + 2) / (N_MELS + 1))


def filterbank(edges, mutant=None):
    """the triangles of mel.hip over given edges [130] (float64 arithmetic)"""
    freq = np.arange(N_BINS) * (SR / N_FFT)
    fl, fc, fr = edges[:-2, None], edges[1:-1, None], edges[2:, None]
    up_hi = (freq < fc) if mutant == "fc_strict" else (freq <= fc)
    up = (freq >= fl) & up_hi
    down = ~up & (freq > fc) & (freq <= fr)
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(up, (freq - fl) / (fc - fl), np.where(down, (fr - freq) / (fr - fc), 0.0))
    return w * (2.0 / (fr - fl))


def tables64(mutant=None):
    i = np.arange(N_FFT)
    hann = 0.5 * (1.0 - np.cos(2.0 * np.pi * i / (N_FFT - 1 if mutant == "hann_symmetric" else N_FFT)))
    return hann, filterbank(mel_edges64(), mutant)


def table_bounds():
    """(hann bound scalar, fb bound [128][1]) of the docstring"""
    e = mel_edges64()
    fl, fc, fr = e[:-2], e[1:-1], e[2:]
    err = 64 * U * fr
    return 8 * U, ((2.0 / (fr - fl)) * (6 * err / np.minimum(fc - fl, fr - fc) + 8 * U))[:, None]


def twiddle_errors():
    """(dc, ds) [1024]: numpy-f32 twiddle of the kernel's formula minus the exact one"""
    i = np.arange(N_FFT)
    ang32 = (np.float32(6.283185307179586) * i.astype(np.float32)) / np.float32(N_FFT)
    assert ang32.dtype == np.float32
    ang = 2.0 * np.pi * i / N_FFT
    return np.cos(ang32).astype(np.float64) - np.cos(ang), np.sin(ang32).astype(np.float64) - np.sin(ang)


def twiddle_tau():
    dc, ds = twiddle_errors()
    return max(np.abs(dc).max(), np.abs(ds).max())


_TW = {}


def _twiddles():
    if not _TW:
        idx = (np.arange(N_BINS)[:, None] * np.arange(N_FFT)[None, :]) % N_FFT
        ang = 2.0 * np.pi * np.arange(N_FFT) / N_FFT
        dc, ds = twiddle_errors()
        _TW["c"], _TW["s"], _TW["dc"], _TW["ds"] = np.cos(ang)[idx], np.sin(ang)[idx], dc[idx], ds[idx]
    return _TW["c"], _TW["s"], _TW["dc"], _TW["ds"]


def windowed(audio, hann32, mutant=None):
    """xs [frames][1024] float64 holding f32 values"""
    p = padded(audio, mutant)
    nf = frames(np.asarray(audio).size)
    if nf == 0:
        return np.zeros((0, N_FFT))
    fr = np.stack([p[f * HOP:f * HOP + N_FFT] for f in range(nf)])
    xs = (fr * np.asarray(hann32, np.float32)[None, :]).astype(np.float32).astype(np.float64)
    if mutant == "drop_512":
        xs[:, 512] = 0.0
    return xs


def kernel_bin_bound(xs):
    """(d_re, d_im) [frames][513] of step (1)"""
    c, s, dc, ds = _twiddles()
    dre, dim = np.zeros((xs.shape[0], N_BINS)), np.zeros((xs.shape[0], N_BINS))
    for f in range(xs.shape[0]):
        ax = np.abs(xs[f]).sum()
        for tw, dtw, dst in ((c, dc, dre), (s, ds, dim)):
            p = xs[f][None, :] * tw
            dst[f] = (1 + gamma(N_FFT)) * (U * (np.abs(np.cumsum(p, axis=1)).sum(axis=1) + np.abs(p).sum(axis=1)) + np.abs(dtw @ xs[f]) + 4 * U * ax)
    return dre, dim


def oracle_bin_bound(xs, re, im):
    base = gamma(40, 2.0 ** -53) * np.abs(xs).sum(axis=1)[:, None]
    return base + U * np.abs(re), base + U * np.abs(im)


def spectrum(xs, mutant=None):
    X = np.fft.fft(xs, axis=1)
    if mutant == "twiddle_k1":
        X = np.roll(X, -1, axis=1)
    return X.real[:, :N_BINS], X.imag[:, :N_BINS]


def mel64(audio, hann32, fb32, bin_bound="kernel", mutant=None):
    """-> v [frames][128], ln(max(v, floor)) and the per-output bound d_v (None when bin_bound is None), all float64"""
    if mutant in ("hann_symmetric", "fc_strict"):
        h64, f64 = tables64(mutant)
        if mutant == "hann_symmetric":
            hann32 = h64.astype(np.float32)
        else:
            fb32 = f64.astype(np.float32)
    xs = windowed(audio, hann32, mutant)
    fb = np.asarray(fb32, np.float32).astype(np.float64).copy()
    if mutant == "fb_stop_512":
        fb[:, 512] = 0.0
    re, im = spectrum(xs, mutant)
    eps = 0.0 if mutant == "no_eps" else float(EPS)
    q = re * re + im * im + eps
    mag = np.sqrt(q)
    v = mag @ fb.T
    floor = 1e-6 if mutant == "floor_1e6" else float(FLOOR)
    with np.errstate(divide="ignore"):
        out = np.log(np.maximum(v, floor))
    if bin_bound is None:
        return v, out, None
    dre, dim = kernel_bin_bound(xs) if bin_bound == "kernel" else oracle_bin_bound(xs, re, im)
    extra = 2 * np.abs(re) * dre + dre ** 2 + 2 * np.abs(im) * dim + dim ** 2
    dq = extra + gamma(4) * (q + extra)
    dsq = np.minimum(dq / np.sqrt(q), np.sqrt(dq))
    dmag = dsq + U * (mag + dsq)
    dv = dmag @ fb.T + gamma(514) * v
    return v, out, dv


def classify(v, dv):
    """-> (above, floor, straddle) boolean masks of step (4)"""
    above = v - dv > float(FLOOR)
    floor = v + dv < float(FLOOR)
    return above, floor, ~(above | floor)


def limits(v, dv):
    """-> (lo, hi): a correct kernel's output lies in [lo, hi], per output"""
    above, floor, straddle = classify(v, dv)
    lo, hi = np.empty_like(v), np.empty_like(v)
    with np.errstate(divide="ignore", invalid="ignore"):
        lv = np.log(np.where(above, v, 1.0))
        tol = np.where(above, dv / np.where(above, v - dv, 1.0) + 2 * U * np.abs(lv), 0.0)
        lu = np.log(v + dv)
    lo[above], hi[above] = (lv - tol)[above], (lv + tol)[above]
    lnf = float(LN_FLOOR32)
    lo[~above] = lnf - ULP_LN_FLOOR
    hi[floor] = lnf + ULP_LN_FLOOR
    hi[straddle] = np.maximum(lnf + ULP_LN_FLOOR, (lu + 2 * U * np.abs(lu)))[straddle]
    return lo, hi


def excess(got, v, dv):
    """largest (distance from the reference value) / (allowed distance) over the outputs, 0 for an empty clip; <= 1 passes.  For the floor and
    straddle classes the reference value is the middle of [lo, hi]."""
    if v.size == 0:
        return 0.0
    lo, hi = limits(v, dv)
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    return float((np.abs(np.asarray(got, np.float64) - mid) / half).max())


def above_excess(got, v, dv):
    """largest |got - ln v| / (d_v / (v - d_v) + 2u |ln v|) over the outputs above the floor (0 if there are none): the error / bound figure of
    profiles/voice_front_end_f64.md.  The floor and straddle classes have no such ratio; limits() checks them."""
    above = classify(v, dv)[0]
    if not above.any():
        return 0.0
    lv = np.log(v[above])
    tol = dv[above] / (v[above] - dv[above]) + 2 * U * np.abs(lv)
    return float((np.abs(np.asarray(got, np.float64)[above] - lv) / tol).max())
