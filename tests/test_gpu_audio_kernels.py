"""The audio analysis kernels (csrc/audio.hip, csrc/features.hip) one entry point at a time, straight through the C ABI, against the
float64 twin tests/audio_ref.py - the method of tests/test_gpu_groupnorm.py: G = 4096 guard elements on both sides of every buffer
(NaN around inputs, a sentinel bit pattern in outputs: after each call the guards are intact, the body is fully written and no NaN
leaked in), a family whose result is exact (compared bit for bit, ranks as integers) and a random family inside a derived bound, plus
every argument check of the launchers as a refusal.  tests/test_audio_host.py proves what the exact families rest on and that these
comparisons reject off-by-one mutants of the twin.  test_zz_report prints the worst error / bound per family (WORST) and the measured
deviations of the library functions (DEVS).

Bounds (v = 2^-24), all in tests/audio_ref.py next to the result they belong to:
    stft              per frame, 2-norm over the stored bins: (t eta / (1 - t eta) + v) ||X_f||, t = log2 n_fft, eta = v + gamma_4 (sqrt 2 + v)
                      (Higham, radix-2 FFT with twiddles rounded from double; + the window product)
    istft             per sample: the same transform bound on every covering frame's 2-norm (an element errs no more than its vector),
                      3 v per term, the two sums and the division.  An element-wise use of a norm-wise bound: expect a small ratio.
    hpss              hypotf at d (both medians inherit it), a = X / Z and b at (1 + d)(1 + v) / ((1 - d)(1 - v)) - 1, squares (or powf),
                      m / (m + r): 2 rho / (1 - rho) mask (1 - mask), two roundings; (S mask)(D / S): three roundings, S cancels
    mel_power         (1025 + 4) v sum_k |basis| |D|^2
    onset_from_mel    per dB value 10 dev(log10f) + v |dB|, the floor's subtraction, twice that per difference + v; the mean adds
                      (n_mels + 1) v mean; the median moves no further than its inputs
    rms, length 300   (300 + 3) v relative;    matmul_nt   (K + 1) v sum |a| |b|
    flatness          |z|^2 within 5 v (or powf), logf absolute, the fixed tree's ceil(n / 256) + 8 additions, expf, the mean, the division
    piptrack          the decisions exact; with integer magnitudes only the division, a sum and the products round: 3 v of the terms
    spline_step       the spline itself exact; 1 / (2 m) within 5 v, the exponent's product, expf on e / (1 + e), four roundings
    magnitude, emphasize, eerp, contrast   the operation order with hypotf / powf / tanhf / sinf at their measured deviations
Exact, bit for bit: median31 and every rank of order_stat (and its three interpolations), normalize, minmax, clamp, peak_mask,
threshold_scale, rms at power-of-two lengths (sqrtf the only rounding), the Gaussian filter on integers with dyadic taps, the
rectangular-window transforms of constant and alternating signals, mel_power on axis-aligned spectra with dyadic weights, the onset
envelope's zeros, matmul_nt / autocorr_frames / fir_decimate on integers, overlap_add's single division, band_sorted_means' ascending
sums, plp_select on axis-aligned peaks, spline_step without the step, sosfilt in place against out of place.
Library functions on the device (the project's convention): the float32 CPU function against float64 over the case's own arguments,
4 x the largest deviation allowed, no other margin.  Measured (relative unless said): hypotf 5.9e-08, powf 1.0e-07, expf 1.2e-07,
logf 6.2e-07 absolute, log10f 1.2e-06 absolute, tanhf 6.0e-08 absolute, sinf 6.0e-08 absolute; the report prints them per family.
Measured on an MI355X, worst error / bound: stft 0.028 (impulses 0.020), stft_general 0.13, istft 0.0040, istft(stft(y)) 0.0038,
istft_general 0.14, hpss 0.24 (power 1.5: 0.19), mel_power 0.011, onset_from_mel 0.064 (median 0.066), rms at length 300 0.0041,
matmul_nt 0.49, flatness 0.18, piptrack 0.41, spline_step 0.45, magnitude 0.54, emphasize 0.48, eerp 0.22 / 0.26, contrast 0.23.
Where the reference itself returns NaN - the midpoint quantile landing on an infinite element, a + 0 (b - a) - the twin follows it;
an end of a signal is never a peak of peak_mask (its clamped neighbour is itself), as in the reference."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import audio_ref as R  # noqa: E402
from cabi_guard import Buf, call, cbuf, inp, ratio, refused, same  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}                                          # family -> worst error / bound seen
DEVS = {}                                           # library function -> largest measured deviation (4 x that is allowed)
INF = float("inf")


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), float(r))
    return r


def as_complex(a, rows):
    a = a.astype(np.float64).reshape(rows, -1, 2)
    return a[..., 0] + 1j * a[..., 1]


# ---------------------------------------------------------------------------------------------------------------- STFT / iSTFT
def run_stft(y, n_fft=None, hop=None, win=None):
    n = y.size
    yb = inp(y)
    if n_fft is None:
        nf, nb = 1 + n // 1024, 1025
        out = Buf(nf * nb * 2)
        call("maua_stft", yb.ptr, n, out.ptr)
    else:
        nf, nb = 1 + n // hop, n_fft // 2 + 1
        wb = inp(win)
        out = Buf(nf * nb * 2)
        call("maua_stft_general", yb.ptr, n, n_fft, hop, wb.ptr, out.ptr)
    out.check("stft")
    return as_complex(out.get(), nf)


def frame_ratio(got, spec, log_n):
    err = np.sqrt((np.abs(got - spec) ** 2).sum(1))
    assert np.isfinite(err).all()
    b = R.stft_bound(spec, log_n)
    return float(np.max(np.where(err > 0, err / np.maximum(b, 1e-300), 0.0)))


@pytest.mark.parametrize("n", R.STFT_N)
def test_stft(n):
    assert L.lib().maua_stft_num_frames(n) == 1 + n // 1024
    y = R.signal(n, n)
    assert note("stft, random", frame_ratio(run_stft(y), R.stft(y)[0], 11)) <= 1
    for i, y in enumerate(R.impulses(n)):           # the reflect padding of the first and last frames, unmasked by anything loud
        assert note("stft, impulses", frame_ratio(run_stft(y), R.stft(y)[0], 11)) <= 1, i


def run_istft(spec32, length, n_fft=None, hop=None, win=None):
    nf = spec32.shape[0]
    sb = cbuf(spec32)
    out = Buf(length)
    if n_fft is None:
        call("maua_istft", sb.ptr, nf, length, out.ptr)
    else:
        wb = inp(win)
        call("maua_istft_general", sb.ptr, nf, n_fft, hop, wb.ptr, length, out.ptr)
    out.check("istft")
    sb.check("istft spec")
    return out.get()


@pytest.mark.parametrize("n", R.STFT_N)
def test_istft(n):
    y = R.signal(n, 7 * n)
    spec = R.stft(y)[0].astype(np.complex64)
    nf = spec.shape[0]
    for length in (1024 * (nf - 1) - 5, 1024 * (nf - 1), 1024 * (nf + 1) + 3):
        want, bound = R.istft(spec, length)
        got = run_istft(spec, length)
        assert note("istft", ratio(got, want, bound)) <= 1, length
        assert (got[1024 * (nf + 1):] == 0).all()
    want, bound = R.istft(spec[:1], 1500)            # one frame: its second half alone, nothing behind it
    got = run_istft(spec[:1], 1500)
    assert note("istft", ratio(got, want, bound)) <= 1 and (got[1024:] == 0).all()
    # the round trip on the device: the forward transform's bound carried through the inverse
    dev_spec = run_stft(y)
    length = 1024 * (nf - 1)
    exact = R.stft(y)[0]
    want, bound = R.istft(exact, length, spec_err=R.stft_bound(exact, 11))
    assert np.abs(want - y[:length]).max() <= 1e-6
    got = run_istft(dev_spec.astype(np.complex64), length)
    assert note("istft(stft(y))", ratio(got, want, bound)) <= 1


GENERAL = [(2, 1), (2, 2), (2, 5), (64, 1), (64, 7), (64, 16), (64, 64), (64, 67), (1024, 7), (1024, 256), (1024, 1024), (1024, 1027),
           (2048, 512), (2048, 2051), (4096, 1024), (4096, 4096), (4096, 4099), (8192, 2048), (8192, 8192), (8192, 8195)]
# (hop 1 and 7 only where frames * n_fft stays within a few hundred thousand elements)


@pytest.mark.parametrize("n_fft,hop", GENERAL)
def test_stft_general(n_fft, hop):
    n = n_fft // 2 + 1
    log_n = int(np.log2(n_fft))
    ones = np.ones(n_fft, np.float32)
    nf, nb = 1 + n // hop, n_fft // 2 + 1
    # exact: a rectangular window over a constant / an alternating signal (the reflection keeps both): N c in one bin, zeros elsewhere
    for c in (3.0, -5.0):
        got = run_stft(np.full(n, c, np.float32), n_fft, hop, ones)
        want = np.zeros((nf, nb), np.complex128)
        want[:, 0] = n_fft * c
        assert same(got, want), ("constant", c)
        alt = c * (-1.0) ** np.arange(n)
        got = run_stft(alt.astype(np.float32), n_fft, hop, ones)
        want = np.zeros((nf, nb), np.complex128)
        want[:, -1] = n_fft * c * (-1.0) ** ((np.arange(nf) * hop - n_fft // 2) % 2)
        assert same(got, want), ("alternating", c)
    y = R.signal(n, n_fft + hop)
    win = R.f32(np.random.default_rng(hop).uniform(0.25, 1.0, n_fft))
    assert note("stft_general", frame_ratio(run_stft(y, n_fft, hop, win), R.stft(y, n_fft, hop, win)[0], log_n)) <= 1


@pytest.mark.parametrize("n_fft,hop", GENERAL)
def test_istft_general(n_fft, hop):
    rng = np.random.default_rng(n_fft + hop)
    nf = 3 if n_fft > 64 else 5
    nb = n_fft // 2 + 1
    spec = (R.f32(rng.normal(size=(nf, nb))) + 1j * R.f32(rng.normal(size=(nf, nb)))).astype(np.complex64)
    win = R.f32(rng.uniform(0.25, 1.0, n_fft))
    length = max((nf - 1) * hop + n_fft // 2 + 3, 1)
    want, bound = R.istft(spec, length, n_fft, hop, win)
    got = run_istft(spec, length, n_fft, hop, win)
    assert note("istft_general", ratio(got, want, bound)) <= 1
    if hop > n_fft:                                  # samples no frame covers come out 0
        p = np.arange(length) + n_fft // 2
        gap = (p % hop >= n_fft) | (p // hop >= nf)
        assert gap.any() and (got[gap] == 0).all() and (want[gap] == 0).all()


def test_stft_refusals():
    y, out, win = inp(np.zeros(9000)), Buf(64), inp(np.ones(16384))
    refused("maua_stft", y.ptr, 1024, out.ptr)
    refused("maua_stft_general", y.ptr, 9000, 3000, 100, win.ptr, out.ptr)
    refused("maua_stft_general", y.ptr, 9000, 16384, 100, win.ptr, out.ptr)
    refused("maua_stft_general", y.ptr, 9000, 64, 0, win.ptr, out.ptr)
    refused("maua_stft_general", y.ptr, 32, 64, 16, win.ptr, out.ptr)
    refused("maua_istft_general", y.ptr, 1, 3000, 100, win.ptr, 10, out.ptr)
    refused("maua_istft_general", y.ptr, 1, 64, 0, win.ptr, 10, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- medians, HPSS
def run_median(x, axis):
    nf, nb = x.shape
    xb, out = inp(x), Buf(x.size)
    call("maua_median31", xb.ptr, nf, nb, axis, out.ptr)
    out.check("median31", nan_ok=False)
    return out.get().reshape(nf, nb)


@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("kind", R.MEDIAN_KINDS)
def test_median31(axis, kind):
    for n in R.MEDIAN_AXIS_LEN:
        for other in R.MEDIAN_OTHER:
            shape = (n, other) if axis == 0 else (other, n)
            x = R.median_input(*shape, kind, seed=n + other, axis=axis)
            got = run_median(x, axis)
            assert same(got, R.median31(x, axis)), (kind, shape)
            if kind.startswith("ramp"):
                ramp = np.arange(n, dtype=np.float32) * (1 if kind == "ramp_up" else -1)
                assert same(got[:, 0] if axis == 0 else got[0], ramp[R.ramp_median_index(n)])


def test_median31_beyond_one_grid():
    """65537 frames: the frame index no longer fits one launch's gridDim.y"""
    x = R.median_input(65537, 1, "random", 1)
    assert same(run_median(x, 0), R.median31(x, 0))
    x = R.median_input(65537, 16, "ties3", 2)
    assert same(run_median(x, 1), R.median31(x, 1))


def test_median31_refusals():
    x, out = inp(np.zeros(15 * 20)), Buf(300)
    refused("maua_median31", x.ptr, 15, 20, 0, out.ptr)
    refused("maua_median31", x.ptr, 20, 15, 1, out.ptr)
    refused("maua_median31", x.ptr, 20, 15, 2, out.ptr)
    assert out.untouched()


@pytest.mark.parametrize("n_frames", (16, 33))
@pytest.mark.parametrize("margin,power", [(1.0, 2.0), (8.0, 2.0), (1.0, 1.5)])
def test_hpss(n_frames, margin, power):
    D = R.hpss_input(n_frames, n_frames)
    ref = R.hpss(D, margin, power)
    DEVS["hypotf, relative (hpss)"] = max(DEVS.get("hypotf, relative (hpss)", 0.0), ref["hyp_dev"] / 4)
    if power != 2:
        DEVS["powf, relative (hpss)"] = max(DEVS.get("powf, relative (hpss)", 0.0), ref["pow_dev"] / 4)
    db = cbuf(D)
    n = D.size * 2
    for want_h, want_p in ((1, 1), (1, 0), (0, 1)):
        h, p = (Buf(n) if want_h else None), (Buf(n) if want_p else None)
        call("maua_hpss", db.ptr, n_frames, margin, power, h.ptr if h else None, p.ptr if p else None)
        for b, key in ((h, "h"), (p, "p")):
            if b is None:
                continue
            b.check("hpss " + key)
            got = b.get().reshape(n_frames, 1025, 2)
            assert note(f"hpss, power {power}", ratio(got, ref[key], ref["b" + key])) <= 1, (key, want_h, want_p)
            f0 = n_frames // 3                       # Z = 0 under a value that is not 0: the mask is exactly 0.5 or 0
            assert same(got[f0, 30], (0.5 if margin == 1 else 0.0) * np.array([1.5, -0.5], np.float32))
            assert (got[:, :30] == 0).all() and (got[n_frames // 2, 500:510] == 0).all()
    db.check("hpss spec")
    refused("maua_hpss", db.ptr, n_frames, margin, power, None, None)


# ---------------------------------------------------------------------------------------------------------------- mel, onsets
def run_mel(D, basis, T, n_mels):
    db, bb, out = cbuf(D), inp(basis), Buf(n_mels * T)
    call("maua_mel_power", db.ptr, T, bb.ptr, n_mels, out.ptr)
    out.check("mel")
    return out.get().reshape(n_mels, T)


@pytest.mark.parametrize("T", (1, 15, 16, 17, 33))
def test_mel_power(T):
    for n_mels in (1, 40, 127, 128):
        D, basis = R.mel_exact_input(T, n_mels, T + n_mels)
        assert same(run_mel(D, basis, T, n_mels), R.f32(R.mel_power(D, basis)[0])), n_mels
        rng = np.random.default_rng(T * n_mels)
        Dr = (R.f32(rng.normal(size=(T, 1025))) + 1j * R.f32(rng.normal(size=(T, 1025)))).astype(np.complex64)
        br = R.f32(rng.uniform(0, 0.05, size=(n_mels, 1025)) * (rng.uniform(size=(n_mels, 1025)) < 0.1))
        want, bound = R.mel_power(Dr, br)
        assert note("mel_power", ratio(run_mel(Dr, br, T, n_mels), want, bound)) <= 1, n_mels
    d, b, out = inp(np.zeros(2050)), inp(np.zeros(1025)), Buf(8)
    refused("maua_mel_power", d.ptr, 1, b.ptr, 0, out.ptr)
    refused("maua_mel_power", d.ptr, 1, b.ptr, 129, out.ptr)
    assert out.untouched()


def run_onset(mel, pad, aggregate):
    n_mels, T = mel.shape
    mb, env = inp(mel), Buf(T)
    call("maua_onset_from_mel", mb.ptr, n_mels, T, 1e-10, 80.0, pad, aggregate, env.ptr)
    env.check("onset envelope")
    mb.check("mel in place")
    assert not np.isnan(mb.get()).any()
    return env.get()


@pytest.mark.parametrize("aggregate", (0, 1))
@pytest.mark.parametrize("n_mels", (1, 2, 127, 128))
def test_onset_from_mel(aggregate, n_mels):
    amin = float(np.float32(1e-10))
    for T in (1, 2, 3, 255, 256, 257) + ((513,) if n_mels == 128 else ()):       # 128 x 513: the min / max partials grid-stride
        mel = R.onset_input(n_mels, T, n_mels + T)
        dev = R.measured_dev(np.log10, np.log10, [np.maximum(np.float32(amin), mel)], relative=False)
        DEVS["log10f, absolute (onset_from_mel)"] = max(DEVS.get("log10f, absolute (onset_from_mel)", 0.0), dev)
        const = R.onset_input(n_mels, T, T, constant_rows=True)
        for pad in (1, 2, 3):
            got = run_onset(mel, pad, aggregate)
            _, want, bound = R.onset_from_mel(mel, amin, 80.0, pad, aggregate, log_dev=4 * dev)
            assert (got[:pad] == 0).all() and (pad < T or (got == 0).all())
            assert note(f"onset_from_mel, {'median' if aggregate else 'mean'}", ratio(got, want, bound)) <= 1, (T, pad)
            assert (run_onset(const, pad, aggregate) == 0).all(), "constant rows"
    m, e = inp(np.ones(4)), Buf(2)
    refused("maua_onset_from_mel", m.ptr, 2, 2, 1e-10, 80.0, 1, 2, e.ptr)
    assert e.untouched()


# ---------------------------------------------------------------------------------------------------------------- envelope kernels
def envelope_inputs(n):
    """negative values with the extremes at the first and last element, swapped, and at an element only the grid-stride tail reaches"""
    x = R.signal(n, n) - 3.0
    a, b, c = x.copy(), x.copy(), x.copy()
    a[0], a[-1] = -9.0, 7.5
    b[0], b[-1] = 7.5, -9.0
    c[65536 + (n - 65536) // 2 if n > 65536 else n - 1] = 7.5
    if n > 2:
        c[n // 2] = -9.0
    return a, b, c


@pytest.mark.parametrize("n", R.NORM_N)
def test_normalize_minmax_clamp(n):
    for x in envelope_inputs(n):
        xb = inp(x)
        for eps in (1e-8, 0.0):
            out = Buf(n)
            call("maua_normalize", xb.ptr, n, eps, out.ptr)
            out.check("normalize", nan_ok=(n == 1 and eps == 0))
            assert same(out.get(), R.normalize32(x, eps)), eps
        mm = Buf(2)
        call("maua_minmax", xb.ptr, n, mm.ptr)
        mm.check("minmax")
        assert same(mm.get(), [x.min(), x.max()])
        xn = x.copy()
        xn[n // 3] = np.nan
        xnb = inp(xn)
        lo, hi = inp([-3.5]), inp([-2.0])
        pinf = inp([INF])
        for lo_b, lo_c, hi_b, hi_v, add in ((lo, 0.0, hi, -2.0, 0.0), (lo, 0.0, hi, -2.0, 0.25), (None, -INF, hi, -2.0, 1e-10), (None, -4.0, pinf, INF, 0.0)):
            out = Buf(n)
            call("maua_clamp", xnb.ptr, lo_b.ptr if lo_b else None, hi_b.ptr, lo_c, add, n, out.ptr)
            out.check("clamp", nan_ok=True)
            assert same(out.get(), R.clamp32(xn, -3.5 if lo_b else lo_c, hi_v, add)), (lo_c, hi_v, add)
            assert np.isnan(out.get()[n // 3])
        for b in (xb, xnb, lo, hi, pinf):
            b.check("an input")
    const = np.full(n, -1.25, np.float32)
    cb = inp(const)
    for eps in (1e-8, 0.0):                          # a constant input: 0 with eps > 0; 0 / 0 = NaN everywhere with eps = 0, like the reference
        out = Buf(n)
        call("maua_normalize", cb.ptr, n, eps, out.ptr)
        out.check("normalize", nan_ok=True)
        assert same(out.get(), R.normalize32(const, eps)) and bool(np.isnan(out.get()).all()) == (eps == 0)


def test_minmax_refusal():
    x, out = inp(np.zeros(4)), Buf(2)
    refused("maua_minmax", x.ptr, 0, out.ptr)
    assert out.untouched()


def test_peak_mask():
    rng = np.random.default_rng(0)
    cases = [np.array([1.0]), np.array([2.0, 1.0]), np.array([1.0, 2.0]), np.array([1.0, 1.0]), np.array([0, 1, 1, 0, 2, 2, 2, 1, 3.0]),
             np.array([3.0, 1, 0, 1, 3]), np.array([0.0, -0.0, 0.0, 5, 5, -INF, INF, INF])]
    cases += [rng.integers(0, 3, size=n).astype(np.float64) for n in (255, 256, 257, 65537)] + [R.signal(n, n) for n in (256, 257, 65537)]
    for x in cases:
        x = R.f32(x)
        xb, out = inp(x), Buf(x.size, torch.uint8)
        call("maua_peak_mask", xb.ptr, x.size, out.ptr)
        out.check("peak_mask")
        assert same(out.get(), R.peak_mask(x)), x[:10]


@pytest.mark.parametrize("fl", (2, 64, 256, 2048, 300))
def test_rms(fl):
    for hop in (1, 100, fl):
        for n in (fl // 2 + 1, fl + 39):
            y = np.random.default_rng(fl + hop + n).integers(-15, 16, size=n).astype(np.float32)
            nf = 1 + n // hop
            yb, out = inp(y), Buf(nf)
            call("maua_rms", yb.ptr, n, fl, hop, nf, out.ptr)
            out.check("rms")
            want = R.rms(y, fl, hop, nf)
            mean = (R.frames_of(y, fl, hop)[:nf] ** 2).mean(1)
            if fl == 300:
                assert note("rms, length 300", ratio(out.get(), want, (300 + 3) * R.V * want)) <= 1
            else:                                    # the sum and the division by 2^k are exact: sqrtf is the only rounding
                assert same(out.get(), np.sqrt(R.f32(mean))), (hop, n)
            none = Buf(4)
            call("maua_rms", yb.ptr, n, fl, hop, 0, none.ptr)
            assert none.untouched()
    yb, out = inp(np.zeros(64)), Buf(4)
    refused("maua_rms", yb.ptr, 32, 64, 16, 1, out.ptr)
    refused("maua_rms", yb.ptr, 64, 64, 0, 1, out.ptr)
    refused("maua_rms", yb.ptr, 64, 0, 16, 1, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- Gaussian filter
def run_gauss(x, taps, radius, mode):
    T, Cc = x.shape
    xb, tb, out = inp(x), inp(taps), Buf(x.size)
    call("maua_gaussian_filter1d", xb.ptr, tb.ptr, radius, T, Cc, mode, out.ptr)
    out.check("gaussian_filter1d")
    return out.get().reshape(T, Cc)


@pytest.mark.parametrize("mode", range(4))
def test_gaussian_filter1d(mode):
    for T in R.GAUSS_T:
        for radius in R.gauss_radii(T):
            for Cc in R.GAUSS_C:
                x, taps = R.gauss_exact_input(T, Cc, radius, seed=T * 1000 + radius * 10 + mode)
                if mode == R.PAD["reflect"] and radius >= T:
                    xb, tb, out = inp(x), inp(taps), Buf(x.size)
                    refused("maua_gaussian_filter1d", xb.ptr, tb.ptr, radius, T, Cc, mode, out.ptr)
                    assert out.untouched()
                    continue
                assert same(run_gauss(x, taps, radius, mode), R.f32(R.gaussian_filter1d(x, taps, radius, mode))), (T, radius, Cc)


def test_gaussian_filter1d_beyond_one_grid():
    """T = 65537 rows: the row index no longer fits one launch's gridDim.y"""
    for mode, radius in ((R.PAD["replicate"], 2), (R.PAD["circular"], 3)):
        x, taps = R.gauss_exact_input(65537, 1, radius, seed=mode)
        assert same(run_gauss(x, taps, radius, mode), R.f32(R.gaussian_filter1d(x, taps, radius, mode)))


def test_gaussian_filter1d_refusals():
    x, taps, out = inp(np.zeros(40)), inp(np.ones(3)), Buf(40)
    refused("maua_gaussian_filter1d", x.ptr, taps.ptr, 1, 40, 1, 4, out.ptr)
    refused("maua_gaussian_filter1d", x.ptr, taps.ptr, 1, 40, 1, 0, x.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- order statistics
def run_order(xb, mb, n, mode, q, k):
    out, ranks = Buf(3), Buf(2, torch.int64)
    call("maua_order_stat", xb.ptr, mb.ptr if mb else None, n, mode, q, k, out.ptr, ranks.ptr)
    out.check("order_stat", nan_ok=True)
    ranks.check("order_stat ranks")
    return out.get(), ranks.get()


def check_order(x, mask, what):
    n = x.size
    xb = inp(x, guard=1e30)                          # (NaN is skipped by design: a finite guard shows up in the count and the ranks)
    mb = inp(mask, torch.uint8, guard=1) if mask is not None else None
    valid = int((~np.isnan(x) & (np.ones(n, bool) if mask is None else mask != 0)).sum())
    specs = [(0, q, 0) for q in R.ORDER_Q] + [(2, q, 0) for q in R.ORDER_Q] + [(1, 0.0, 1), (1, 0.0, max(valid, 1))]
    for mode, q, k in specs:
        got, ranks = run_order(xb, mb, n, mode, q, k)
        want, wranks = R.order_stat(x, mask, mode, q, k)
        assert np.array_equal(ranks, wranks), (what, mode, q, k, ranks, wranks)
        assert same(got, want), (what, mode, q, k, got, want)
    xb.check("order_stat x")
    if mb:
        mb.check("order_stat mask")


@pytest.mark.parametrize("kind", R.ORDER_KINDS)
def test_order_stat(kind):
    big = kind in ("random", "ties", "nan", "low_byte", "sign")
    for n in R.ORDER_N[:7] + (R.ORDER_N[7:] if big else ()):
        check_order(R.order_input(n, kind, seed=n), None, (kind, n))


def test_order_stat_masks_and_refusals():
    for n in (3, 257, 262145):
        x = R.order_input(n, "nan", n)
        for keep in (0, 1, 2, n // 2):
            check_order(x, R.keep_mask(n, keep, keep), ("mask", n, keep))
    out, x = Buf(3), inp(np.zeros(4))
    refused("maua_order_stat", x.ptr, None, 4, 3, 0.5, 0, out.ptr, None)
    refused("maua_order_stat", x.ptr, None, 4, 1, 0.5, 0, out.ptr, None)
    refused("maua_order_stat", None, None, 4, 0, 0.5, 0, out.ptr, None)
    assert out.untouched()
    call("maua_order_stat", x.ptr, None, 4, 0, 0.5, 0, out.ptr, None)      # ranks2 may be NULL
    out.check("order_stat")
    assert same(out.get(), [0, 0, 0])


# ---------------------------------------------------------------------------------------------------------------- feature kernels
@pytest.mark.parametrize("M", R.MATMUL_MN)
def test_matmul_nt(M):
    rng = np.random.default_rng(M)
    for N in R.MATMUL_MN:
        for K in R.MATMUL_K:
            for fam in ("integers", "gaussian"):
                a = rng.integers(-8, 9, size=(M, K)).astype(np.float32) if fam == "integers" else R.f32(rng.normal(size=(M, K)))
                b = rng.integers(-8, 9, size=(N, K)).astype(np.float32) if fam == "integers" else R.f32(rng.normal(size=(N, K)))
                ab, bb, out = inp(a), inp(b), Buf(M * N)
                call("maua_matmul_nt", ab.ptr, bb.ptr, out.ptr, M, N, K)
                out.check("matmul_nt")
                want, bound = R.matmul_nt(a, b)
                got = out.get().reshape(M, N)
                if fam == "integers":
                    assert same(got, R.f32(want)), (N, K)
                else:
                    assert note("matmul_nt", ratio(got, want, bound)) <= 1, (N, K)
    a, out = inp(np.zeros(4)), Buf(4)
    refused("maua_matmul_nt", a.ptr, a.ptr, out.ptr, 2, 2, 0)
    assert out.untouched()


def test_band_sorted_means():
    rng = np.random.default_rng(3)
    nb, nf = 1100, 3
    spec = rng.integers(-5, 6, size=(nf, nb)) * np.where(rng.integers(0, 2, size=(nf, nb)) == 1, 1j, 1)       # axis-aligned, heavy ties
    sb = cbuf(spec)
    for band in (1, 2, 3, 599, 1023, 1024):
        for lo, hi in ((0, band), (nb - band, nb), (37, 37 + band)):
            for k in sorted({1, min(2, band), band}):
                v, p = Buf(nf), Buf(nf)
                call("maua_band_sorted_means", sb.ptr, nf, nb, lo, hi, k, v.ptr, p.ptr)
                v.check("valley")
                p.check("peak")
                wv, wp = R.band_sorted_means(spec, lo, hi, k)
                assert same(v.get(), wv) and same(p.get(), wp), (band, lo, hi, k)
    v, p = Buf(nf), Buf(nf)
    refused("maua_band_sorted_means", sb.ptr, nf, nb, 0, 1025, 1, v.ptr, p.ptr)
    refused("maua_band_sorted_means", sb.ptr, nf, nb, 0, 10, 0, v.ptr, p.ptr)
    refused("maua_band_sorted_means", sb.ptr, nf, nb, 0, 10, 11, v.ptr, p.ptr)
    refused("maua_band_sorted_means", sb.ptr, nf, nb, 5, 5, 1, v.ptr, p.ptr)
    refused("maua_band_sorted_means", sb.ptr, nf, nb, 1000, 1101, 1, v.ptr, p.ptr)
    assert v.untouched() and p.untouched()
    sb.check("spec")


def test_autocorr_frames():
    rng = np.random.default_rng(4)
    nf = 3
    for W in (1, 2, 255, 256, 257, 1000):
        e, w = rng.integers(0, 8, size=nf + W - 1).astype(np.float32), (rng.integers(0, 3, size=W) / 2.0).astype(np.float32)
        eb, wb = inp(e), inp(w)
        for n_lags in sorted({1, W, min(W, 300)}):
            out = Buf(nf * n_lags)
            call("maua_autocorr_frames", eb.ptr, wb.ptr, nf, W, n_lags, out.ptr)
            out.check("autocorr")
            assert same(out.get().reshape(nf, n_lags), R.f32(R.autocorr_frames(e, w, nf, W, n_lags))), (W, n_lags)
        out = Buf(8)
        refused("maua_autocorr_frames", eb.ptr, wb.ptr, nf, W, W + 1, out.ptr)
        assert out.untouched()
        eb.check("envelope")


def test_fir_decimate():
    rng = np.random.default_rng(5)
    ntaps, n = 7, 50
    x, taps = rng.integers(-16, 17, size=n).astype(np.float32), (rng.integers(-4, 5, size=ntaps) / 8.0).astype(np.float32)
    xb, tb = inp(x), inp(taps)
    for stride in (1, 2, 3):
        for left in (0, ntaps - 1, ntaps + 5):
            n_out = n // stride + 8                  # reads past both ends: zero fill
            out = Buf(n_out)
            call("maua_fir_decimate", xb.ptr, n, tb.ptr, ntaps, stride, left, 0.5, out.ptr, n_out)
            out.check("fir_decimate")
            assert same(out.get(), R.f32(R.fir_decimate(x, taps, stride, left, 0.5, n_out))), (stride, left)
    out = Buf(5)
    call("maua_fir_decimate", xb.ptr, 0, tb.ptr, ntaps, 2, 3, 0.5, out.ptr, 5)         # an empty signal: zeros
    out.check("fir_decimate")
    assert (out.get() == 0).all()
    xb.check("x")


def test_overlap_add():
    rng = np.random.default_rng(6)
    W, nf = 8, 5
    frames = rng.integers(-8, 9, size=(nf, W)).astype(np.float32)
    win = np.array([0, 0.5, 1, 1, 0.5, 0, 0, 0], np.float32)       # zeros: samples whose denominator is 0 come out 0
    fb, wb = inp(frames), inp(win)
    for hop in (1, 3, W, W + 2):
        for start in (0, 2):
            length = (nf - 1) * hop + W + 3 - start
            out = Buf(length)
            call("maua_overlap_add", fb.ptr, nf, W, hop, wb.ptr, start, length, out.ptr)
            out.check("overlap_add")
            want, num, den = R.overlap_add(frames, W, hop, win, start, length)
            assert (den == 0).any() and same(out.get(), want), (hop, start)
    fb.check("frames")


def dev_note(name, value):
    DEVS[name] = max(DEVS.get(name, 0.0), float(value))


@pytest.mark.parametrize("nb", (1, 255, 256, 257, 1025))
def test_spectral_flatness(nb):
    rng = np.random.default_rng(nb)
    z = (R.f32(rng.normal(size=(3, nb))) + 1j * R.f32(rng.normal(size=(3, nb)))).astype(np.complex64)
    z[1] = 0                                         # a frame of exact zeros sits at the amin floor: flatness 1
    zb = cbuf(z)
    amin = float(np.float32(1e-10))
    for power in (2.0, 1.5):
        out = Buf(3)
        call("maua_spectral_flatness", zb.ptr, 3, nb, amin, power, out.ptr)
        out.check("flatness")
        ref = R.spectral_flatness(z, amin, power)
        assert abs(ref["out"][1] - 1) <= 1e-12
        assert note(f"spectral_flatness, power {power}", ratio(out.get(), ref["out"], ref["bound"])) <= 1
        dev_note("logf, absolute (flatness)", ref["log_dev"])
        dev_note("expf, relative (flatness)", ref["exp_dev"])
        dev_note("powf, relative (flatness)", ref["pow_dev"])
    zb.check("spec")
    out = Buf(3)
    refused("maua_spectral_flatness", zb.ptr, 3, 0, amin, 2.0, out.ptr)
    assert out.untouched()


@pytest.mark.parametrize("nb", (1, 255, 256, 257, 513))
def test_plp_select(nb):
    ft, fq, lo, hi = R.plp_input(nb, nb)
    want, gap = R.plp_select(ft, fq, lo, hi)
    assert gap.min() > 0.5                           # (tests/test_audio_host.py: far more than the library functions can move a value)
    fb, qb = cbuf(ft), inp(fq)
    call("maua_plp_select", fb.ptr, 4, nb, qb.ptr, lo, hi)
    fb.check("tempogram in place")
    qb.check("tempo frequencies")
    got = as_complex(fb.get(), 4)
    assert not np.isnan(got).any() and same(got, want.astype(np.complex128))
    assert (np.abs(got) > 0).sum(1).tolist() == ([0, 1, 1, 1] if nb == 1 else [0, 1, 2, 1])
    refused("maua_plp_select", fb.ptr, 4, 0, qb.ptr, lo, hi)


@pytest.mark.parametrize("nb", (1, 2, 3, 257))
def test_piptrack(nb):
    nf = 4
    S = R.piptrack_input(nf, nb, nb)
    freqs = R.f32(np.arange(nb) * 10.0)
    sb, mb, qb = inp(S), inp(S.max(1)), inp(freqs)
    for fmin, fmax in ((0.0, 1e9), (10.0, float(freqs[-1]))):          # the band's ends on bin frequencies: fmin included, fmax not
        pitch, mag = Buf(nf * nb), Buf(nf * nb)
        call("maua_piptrack", sb.ptr, nf, nb, mb.ptr, 0.5, qb.ptr, 10.0, fmin, fmax, pitch.ptr, mag.ptr)
        pitch.check("pitch")
        mag.check("mag")
        wp, wm, ok, bp, bm = R.piptrack(S, S.max(1), 0.5, freqs, 10.0, fmin, fmax)
        gp, gm = pitch.get().reshape(nf, nb), mag.get().reshape(nf, nb)
        assert np.array_equal(gm != 0, ok) and (gp[~ok] == 0).all(), "the decisions are exact"
        assert note("piptrack", max(ratio(gp, wp, bp), ratio(gm, wm, bm))) <= 1
    for b in (sb, mb, qb):
        b.check("an input")


@pytest.mark.parametrize("nk", (2, 3, 9))
def test_spline_step(nk):
    x, knots, coef = R.spline_input(nk, nk)
    xb, kb, cb = inp(x), inp(knots), inp(coef)
    out = Buf(x.size)
    call("maua_spline_step", xb.ptr, x.size, kb.ptr, cb.ptr, nk, 0.25, 20.0, 0, out.ptr)
    out.check("spline")
    assert same(out.get(), R.f32(R.spline_step(x, knots, coef, 0.25, 20.0, 0)["w"]))
    out = Buf(x.size)
    call("maua_spline_step", xb.ptr, x.size, kb.ptr, cb.ptr, nk, 0.25, 20.0, 1, out.ptr)
    out.check("spline step")
    ref = R.spline_step(x, knots, coef, 0.25, 20.0, 1)
    dev_note("expf, relative (spline_step)", ref["exp_dev"])
    assert ref["dist"].min() > 1e-3
    assert note("spline_step", ratio(out.get(), ref["out"], ref["bound"])) <= 1
    none = Buf(4)
    refused("maua_spline_step", xb.ptr, x.size, kb.ptr, cb.ptr, 1, 0.25, 20.0, 0, none.ptr)
    assert none.untouched()


@pytest.mark.parametrize("n", (1, 257, 65537))
def test_single_guarded_calls(n):
    rng = np.random.default_rng(n)
    z = (R.f32(rng.normal(size=n)) + 1j * R.f32(rng.normal(size=n))).astype(np.complex64)
    zb = cbuf(z)
    for power in (1.0, 2.0, 1.5):
        out = Buf(n)
        call("maua_magnitude", zb.ptr, n, power, out.ptr)
        out.check("magnitude")
        want, bound, hd, pd = R.magnitude(z, power)
        dev_note("hypotf, relative (magnitude)", hd)
        dev_note("powf, relative (magnitude)", pd)
        assert note("magnitude", ratio(out.get(), want, bound)) <= 1, power
    x = R.f32(rng.uniform(-1, 1, n))
    xb = inp(x)
    # emphasize on a normalised envelope, its device scalars {min, max} and q
    xn = R.f32(rng.uniform(0, 1, n))
    xnb, mmb, qb, out = inp(xn), inp([-2.0, 3.0]), inp([0.4]), Buf(n)
    call("maua_emphasize", xnb.ptr, n, mmb.ptr, qb.ptr, 5.0, out.ptr)
    out.check("emphasize")
    want, bound, td = R.emphasize(xn, -2.0, 3.0, 0.4, 5.0)
    dev_note("tanhf, absolute (emphasize)", td)
    assert note("emphasize", ratio(out.get(), want, bound)) <= 1
    for invert in (0, 1):
        out = Buf(n)
        call("maua_threshold_scale", xb.ptr, n, 0.25, 0.5, invert, out.ptr)
        out.check("threshold_scale")
        assert same(out.get(), R.threshold_scale32(x, 0.25, 0.5, invert))
    a, b, t = (R.f32(rng.uniform(0.1, 0.9, n)) for _ in range(3))
    t[:2] = (0, 1) if n > 1 else t[:2]
    ab, bb, tb = inp(a), inp(b), inp(t)
    for mode in (0, 1):
        out = Buf(n)
        call("maua_eerp", ab.ptr, bb.ptr, tb.ptr, n, mode, out.ptr)
        out.check("eerp")
        want, bound, pd = R.eerp(a, b, t, mode)
        dev_note("powf, relative (eerp)", pd)
        assert note(f"eerp, mode {mode}", ratio(out.get(), want, bound)) <= 1
    if n > 4:                                        # a or b equal to 0 (mode 0: the product is 0 unless the exponent is 0 too)
        a0, b0, t0 = a[:4].copy(), b[:4].copy(), np.array([0.0, 1.0, 0.5, 0.5], np.float32)
        a0[[1, 2]] = 0
        b0[[0, 3]] = 0
        zab, zbb, ztb, out = inp(a0), inp(b0), inp(t0), Buf(4)
        call("maua_eerp", zab.ptr, zbb.ptr, ztb.ptr, 4, 0, out.ptr)
        out.check("eerp")
        assert same(out.get(), [a0[0], b0[1], 0, 0])
    out = Buf(n)
    call("maua_contrast", xb.ptr, n, 75.0, out.ptr)
    out.check("contrast")
    want, bound, sd = R.contrast(x, 75.0)
    dev_note("sinf, absolute (contrast)", sd)
    assert note("contrast", ratio(out.get(), want, bound)) <= 1
    for b_ in (zb, xb, xnb, ab, bb, tb):
        b_.check("an input")
    none = Buf(4)
    refused("maua_contrast", xb.ptr, n, 101.0, none.ptr)
    refused("maua_eerp", ab.ptr, bb.ptr, tb.ptr, n, 2, none.ptr)
    assert none.untouched()


@pytest.mark.parametrize("n", (129, 32769))
def test_sosfilt_in_place(n):
    """x aliasing y: the same bits as out of place, guards intact (scipy at the chunk edges: tests/test_gpu_audio.py)"""
    from scipy import signal as sps
    sos = np.ascontiguousarray(sps.butter(4, 0.2, output="sos"), dtype=np.float64)
    x = np.random.default_rng(n).standard_normal(n)
    xb, out = inp(x, torch.float64), Buf(n, torch.float64)
    call("maua_sosfilt", sos.ctypes.data, sos.shape[0], xb.ptr, n, out.ptr)
    out.check("sosfilt")
    xb.check("sosfilt x")
    want = sps.sosfilt(sos, x)
    assert np.abs(out.get() - want).max() <= 1e-13 * np.abs(want).max()
    call("maua_sosfilt", sos.ctypes.data, sos.shape[0], xb.ptr, n, xb.ptr)
    xb.check("sosfilt in place")
    assert same(xb.get(), out.get())


# ---------------------------------------------------------------------------------------------------------------- report
def test_zz_report():
    """the worst error / bound per family and the measured deviations of the library functions"""
    for k in sorted(WORST):
        print(f"[audio kernels] worst error / bound, {k}: {WORST[k]:.4f}")
    for k in sorted(DEVS):
        print(f"[audio kernels] float32 against float64 over the cases' arguments, {k}: {DEVS[k]:.3e} (4 x allowed)")
    assert all(v <= 1 for v in WORST.values())
