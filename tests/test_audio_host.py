"""What tests/test_gpu_audio_kernels.py rests on, checked without a GPU: (1) the float64 twin tests/audio_ref.py agrees with independent
implementations (torch.stft / istft in float64, torch's unfold(...).median, numpy.sort quantiles and torch.quantile, the reference's
gaussian_filter fallback branch restated with torch.nn.functional.pad, oracle/audio.py, oracle/quantile.py) at the GPU test's shapes;
(2) the preconditions of every exact family hold per input: partial sums are integer multiples of 2^-k below 2^(24 - k), products are
float32 numbers (contraction cannot change a bit); (3) the bounded cases with a discontinuity sit away from it on the reference alone;
(4) the comparison the GPU test uses (np.array_equal for the exact families, error <= bound for the random ones) rejects off-by-one
mutants of the twin at the named shapes."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = Path(__file__).resolve().parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT.parent))
import audio_ref as R  # noqa: E402
from oracle import audio as O  # noqa: E402
from oracle import quantile as OQ  # noqa: E402


def rejected_exact(good, bad):
    return not np.array_equal(np.asarray(good), np.asarray(bad), equal_nan=True)


def rejected_bound(good, bad, bound):
    return bool((np.abs(np.asarray(good) - np.asarray(bad)) > bound).any())


# ---------------------------------------------------------------------------------------------------------------- STFT / iSTFT
@pytest.mark.parametrize("n", R.STFT_N)
def test_stft_twin_against_torch(n):
    y = R.signal(n, n)
    spec, _ = R.stft(y)
    t = torch.stft(torch.from_numpy(y).double(), 2048, 1024, window=torch.from_numpy(R.hann(2048)), center=True, pad_mode="reflect",
                   return_complex=True).T.numpy()
    assert spec.shape == t.shape == (1 + n // 1024, 1025)
    assert np.abs(spec - t).max() <= 1e-10 * np.abs(t).max()
    o = O.stft(torch.from_numpy(y)).T.numpy()           # the oracle computes in float32: inside the GPU test's own bound, per frame
    err = np.sqrt((np.abs(o - spec) ** 2).sum(1))
    assert (err <= R.stft_bound(spec, 11) * 4).all()


@pytest.mark.parametrize("n_fft,hop", [(2, 1), (64, 7), (64, 16), (64, 64), (64, 67), (1024, 256), (4096, 4099)])
def test_stft_general_twin_against_torch(n_fft, hop):
    n = n_fft // 2 + 1 + 3 * hop
    y = R.signal(n, n_fft + hop)
    win = R.f32(np.random.default_rng(1).uniform(0.25, 1.0, n_fft))
    spec, _ = R.stft(y, n_fft, hop, win)
    t = torch.stft(torch.from_numpy(y).double(), n_fft, hop, window=torch.from_numpy(win).double(), center=True, pad_mode="reflect",
                   return_complex=True).T.numpy()
    assert spec.shape == t.shape and np.abs(spec - t).max() <= 1e-10 * max(np.abs(t).max(), 1)


@pytest.mark.parametrize("n", R.STFT_N)
def test_istft_twin_against_torch(n):
    y = R.signal(n, 7 * n)
    spec, _ = R.stft(y)
    nf = spec.shape[0]
    length = 1024 * (nf - 1)
    got, bound = R.istft(spec, length)
    t = torch.istft(torch.from_numpy(spec.T.copy()), 2048, 1024, window=torch.from_numpy(R.hann(2048)), center=True, length=length).numpy()
    assert np.abs(got - t).max() <= 1e-10
    assert np.abs(got - y[:length]).max() <= 1e-6       # (the window is the float32 one: sin^4 + cos^4 only to float32)
    assert (bound > 0).all()
    # shorter, and longer than the frames cover: zero where no frame reaches
    short, _ = R.istft(spec, length - 5)
    assert np.array_equal(short, got[:length - 5])
    longer, _ = R.istft(spec, 1024 * (nf + 1) + 3)
    assert np.array_equal(longer[:length], got) and (longer[1024 * (nf + 1):] == 0).all()


def test_stft_mutants_are_rejected():
    """reflect with edge repeat and a frame offset of +-1 sample move the impulse families' first and last frames by far more than the
    bound; a dropped last frame changes the shape"""
    for n in R.STFT_N:
        for y in R.impulses(n) + [R.signal(n, 3)]:
            spec, _ = R.stft(y)
            bound = R.stft_bound(spec, 11)
            for m in ("edge_repeat", "offset+1", "offset-1"):
                bad, _ = R.stft(y, mutant=m)
                err = np.sqrt((np.abs(bad - spec) ** 2).sum(1))
                if m == "edge_repeat" and y[1024 % n] == 1 and n > 2048:
                    continue                             # an interior impulse is not in any reflected region: nothing to reject
                assert (err > bound).any(), (n, m)
            assert R.stft(y, mutant="drop_last")[0].shape[0] == spec.shape[0] - 1


# ---------------------------------------------------------------------------------------------------------------- medians
@pytest.mark.parametrize("axis", (0, 1))
@pytest.mark.parametrize("kind", R.MEDIAN_KINDS)
def test_median_twin_against_unfold_median(axis, kind):
    for n in R.MEDIAN_AXIS_LEN:
        for other in (1, 257):
            shape = (n, other) if axis == 0 else (other, n)
            x = R.median_input(*shape, kind, seed=n + other, axis=axis)
            got = R.median31(x, axis)
            t = torch.from_numpy(x)[None, None]
            k, p = ((31, 1), (0, 0, 15, 15)) if axis == 0 else ((1, 31), (15, 15, 0, 0))
            want = O.median_filter2d(t, k, p)[0, 0].numpy()
            assert np.array_equal(got, want), (kind, shape)
            if kind.startswith("ramp"):
                src = R.ramp_median_index(n)
                ramp = np.arange(n, dtype=np.float32) * (1 if kind == "ramp_up" else -1)
                # the median of a monotone ramp is the ramp at a known index (decreasing: the same index by symmetry of the rank)
                want_ramp = ramp[src]
                assert np.array_equal(got[:, 0] if axis == 0 else got[0], want_ramp)
            for m in ("rank+1", "rank-1", "edge_repeat"):
                if kind in ("random", "ramp_up", "ramp_down"):
                    assert rejected_exact(got, R.median31(x, axis, mutant=m)), (kind, m, shape)


# ---------------------------------------------------------------------------------------------------------------- Gaussian filter
def reference_fallback(x, taps, radius, mode):
    """the reference's gaussian_filter with its short-sequence branch (processing.py:11-49), restated: pad min(radius, T) with `mode`,
    the rest with replicate, then a depthwise correlation; float64"""
    t = torch.from_numpy(np.asarray(x, dtype=np.float64)).T[None]          # [1][C][T]
    T = t.shape[-1]
    name = {0: "circular", 1: "reflect", 2: "replicate", 3: "constant"}[mode]
    if radius > T:
        t = F.pad(t, (T, T), mode=name)
        t = F.pad(t, (radius - T, radius - T), mode="replicate")
    elif radius:
        t = F.pad(t, (radius, radius), mode=name)
    k = torch.from_numpy(np.asarray(taps, dtype=np.float64)).view(1, 1, -1).repeat(t.shape[1], 1, 1)
    return F.conv1d(t, k, groups=t.shape[1])[0].T.numpy()


@pytest.mark.parametrize("mode", range(4))
def test_gaussian_twin_preconditions_and_mutants(mode):
    seen_mutant = False
    for T in R.GAUSS_T:
        for radius in R.gauss_radii(T):
            if mode == 1 and radius >= T:
                continue                                 # refused by the entry point (torch's reflect padding refuses it too)
            for C in (1, 257):
                x, taps = R.gauss_exact_input(T, C, radius, seed=T * 1000 + radius * 10 + mode)
                got = R.gaussian_filter1d(x, taps, radius, mode)
                assert np.array_equal(got, reference_fallback(x, taps, radius, mode)), (T, radius, C)
                # exactness: every tap * x is a float32 number, and all of them lie on one dyadic grid with the sum of magnitudes
                # below 2^24 units: every partial sum, in any order, contracted or not, is exact
                assert R.products_exact(taps[:, None], x.reshape(1, -1))
                assert R.sums_exact((np.abs(R.f64(taps)) * np.abs(x).max())[None, :])
                assert np.array_equal(R.f64(R.f32(got)), got)
                if radius > T and mode != 2:
                    bad = R.gaussian_filter1d(x, taps, radius, mode, mutant="full_radius")
                    if rejected_exact(got, bad):
                        seen_mutant = True
    assert seen_mutant or mode != 0          # (replicate and zero padding give the same array either way; reflect never gets there)


def test_gaussian_twin_against_oracle():
    """the oracle builds its own Gaussian taps: hand the same taps to the twin"""
    for T, sigma in ((40, 2.0), (5, 3.0), (2, 1.0)):
        for mode in ("circular", "replicate", "constant"):
            x = torch.from_numpy(R.signal(T * 3, T).reshape(T, 3))
            radius = min(int(sigma * 4), 3 * T)
            k = torch.arange(-radius, radius + 1, dtype=torch.float32)
            k = torch.exp(-0.5 / sigma ** 2 * k ** 2)
            k = (k / k.sum()).numpy()
            if radius == T:
                continue                                 # the oracle's `radius > n` leaves radius == T to torch's own padding
            want = O.gaussian_filter(x, sigma, mode=mode).numpy()
            got = R.gaussian_filter1d(x.numpy(), k, radius, R.PAD[mode])
            assert np.abs(got - want).max() <= 1e-5 * max(np.abs(want).max(), 1e-3), (T, sigma, mode)


# ---------------------------------------------------------------------------------------------------------------- order statistics
@pytest.mark.parametrize("kind", R.ORDER_KINDS)
def test_order_stat_twin_against_sort_torch_and_oracle(kind):
    for n in R.ORDER_N[:-2] + (4097,):
        x = R.order_input(n, kind, seed=n)
        clean = np.sort(x[~np.isnan(x)])
        for q in R.ORDER_Q:
            out, ranks = R.order_stat(x, None, 0, q, 0)
            v, lo, hi = OQ.quantile_with_indices(torch.from_numpy(x), q) if n else (float("nan"), -1, -1)
            assert (lo, hi) == tuple(ranks), (kind, n, q)
            assert np.array_equal(np.float32(v), out[0], equal_nan=True), (kind, n, q)
            out2, ranks2 = R.order_stat(x, None, 2, q, 0)
            if clean.size and kind not in ("inf",):
                want = torch.quantile(torch.from_numpy(clean), float(np.float32(q))).numpy()
                assert np.array_equal(want, out2[0], equal_nan=True), (kind, n, q, want, out2)
                pos = float(np.float32(q) * np.float32(clean.size - 1))
                assert ranks2[0] == int(np.floor(pos)) and ranks2[1] == int(np.ceil(pos))
                assert out2[1] == clean[ranks2[0]] and out2[2] == clean[ranks2[1]]
        for k in (1, clean.size):
            if clean.size:
                out, ranks = R.order_stat(x, None, 1, 0.0, k)
                want = torch.kthvalue(torch.from_numpy(clean), k).values.numpy()
                assert np.array_equal(out[0], want) and tuple(ranks) == (k - 1, k - 1)


def test_order_stat_masks_and_mutant():
    x = R.order_input(257, "random", 5)
    for keep in (0, 1, 2):
        m = R.keep_mask(257, keep, 1)
        out, ranks = R.order_stat(x, m, 0, 0.5, 0)
        kept = np.sort(x[m != 0])
        if keep == 0:
            assert np.isnan(out).all() and tuple(ranks) == (-1, -1)
        else:
            assert out[1] == kept[0] and out[2] == kept[-1] and tuple(ranks) == (0, keep - 1)
    good = R.order_stat(x, None, 0, float(np.float32(0.025)), 0)
    bad = R.order_stat(x, None, 0, float(np.float32(0.025)), 0, mutant="swap")
    assert rejected_exact(good[1], bad[1]) and rejected_exact(good[0][1:], bad[0][1:])


# ---------------------------------------------------------------------------------------------------------------- envelope kernels
@pytest.mark.parametrize("n", R.NORM_N)
def test_normalize_clamp_peak_twin(n):
    x = R.signal(n, n) - 3.0
    want = O.normalize(torch.from_numpy(x)).numpy()      # (x - min) / (max(x - min) + 1e-8): the same float32 operations
    assert np.array_equal(R.normalize32(x, 1e-8), want)
    const = np.full(n, -1.25, np.float32)
    assert (R.normalize32(const, 1e-8) == 0).all() and np.isnan(R.normalize32(const, 0.0)).all()
    lo, hi = np.float32(-3.5), np.float32(-2.0)
    xn = x.copy()
    xn[n // 2] = np.nan
    want = torch.clamp(torch.from_numpy(xn), float(lo), float(hi + np.float32(0.25))).numpy()
    assert np.array_equal(R.clamp32(xn, lo, hi, 0.25), want, equal_nan=True)
    t = torch.from_numpy(x)
    pm = ((t > torch.cat((t[1:], t[-1:]))) & (t > torch.cat((t[:1], t[:-1])))).numpy().astype(np.uint8)
    assert np.array_equal(R.peak_mask(x), pm)


def test_peak_mask_mutant_is_rejected():
    for x in (np.array([1.0], np.float32), np.array([2.0, 1.0], np.float32), np.array([0, 1, 1, 0, 2, 2, 2, 1, 3], np.float32)):
        assert rejected_exact(R.peak_mask(x), R.peak_mask(x, mutant=">="))
    assert R.peak_mask(np.array([1.0], np.float32)).tolist() == [0]
    assert R.peak_mask(np.array([2.0, 1.0, 2.0], np.float32)).tolist() == [0, 0, 0]      # an end is never above its clamped neighbour


@pytest.mark.parametrize("fl", (2, 64, 256, 2048))
def test_rms_twin_preconditions_and_mutants(fl):
    for hop in (1, 100, fl):
        for n in (fl // 2 + 1, fl + 39):
            y = np.random.default_rng(fl + hop + n).integers(-15, 16, size=n).astype(np.float32)
            nf = 1 + n // hop
            got = R.rms(y, fl, hop, nf)
            fr = R.frames_of(y, fl, hop)
            assert R.sums_exact(fr ** 2) and R.products_exact(fr, fr)      # integer squares below 2^24: exact in any order; / 2^k exact
            o = O.rms(torch.from_numpy(y), fl, hop)[:, 0].numpy()          # (the oracle drops the last frame)
            assert nf == 1 or np.abs(o - got[:nf - 1]).max() <= 4 * R.V * max(got.max(), 1)
            for m in ("edge_repeat", "offset+1", "offset-1"):
                if n > fl // 2 + 1:             # (at the minimum length a frame is one whole period of the reflected signal)
                    bad = R.rms(y, fl, hop, nf, mutant=m)
                    assert rejected_exact(R.f32(got), R.f32(bad)) or fl == 2, (fl, hop, n, m)


# ---------------------------------------------------------------------------------------------------------------- mel, onsets, HPSS
@pytest.mark.parametrize("T,n_mels", [(1, 1), (15, 40), (16, 127), (17, 128), (33, 128)])
def test_mel_twin_preconditions_and_mutants(T, n_mels):
    D, basis = R.mel_exact_input(T, n_mels, T + n_mels)
    mel, _ = R.mel_power(D, basis)
    P = np.abs(D) ** 2
    assert np.array_equal(np.hypot(D.real, D.imag), np.abs(D.real + D.imag))        # axis-aligned: hypot is exact by definition
    assert R.products_exact(basis[:, None, :], P[None]) and R.sums_exact(R.f64(basis)[:, None, :] * P[None])
    want = (torch.from_numpy(R.f64(basis)) @ torch.from_numpy(P).T).numpy()
    assert np.array_equal(mel, want)
    for m in ("drop_last_bin", "drop_last_row"):
        assert rejected_exact(mel, R.mel_power(D, basis, mutant=m)[0]), m
    rng = np.random.default_rng(T)
    Dr = R.f32(rng.normal(size=(T, 1025))) + 1j * R.f32(rng.normal(size=(T, 1025)))
    br = R.f32(rng.uniform(0, 0.05, size=(n_mels, 1025)))
    good, bound = R.mel_power(Dr, br)
    for m in ("drop_last_bin", "drop_last_row"):
        assert rejected_bound(good, R.mel_power(Dr, br, mutant=m)[0], bound), m


@pytest.mark.parametrize("aggregate", (0, 1))
def test_onset_twin_against_oracle(aggregate):
    for n_mels, T, pad in ((1, 3, 1), (2, 255, 2), (127, 256, 3), (128, 257, 2), (128, 2, 3), (128, 513, 2)):
        mel = R.onset_input(n_mels, T, n_mels + T)
        db, env, bound = R.onset_from_mel(mel, 1e-10, 80.0, pad, aggregate)
        S = O.power_to_db(torch.from_numpy(mel).double())
        assert np.abs(S.numpy() - db).max() <= 1e-9
        assert db.max() - db.min() == 80.0               # the floor is active
        d = torch.clamp(S[:, 1:] - S[:, :-1], min=0)
        d = d.mean(0) if aggregate == 0 else torch.median(d, dim=0).values
        want = F.pad(d, (pad, 0))[:T].numpy()
        assert np.abs(want - env).max() <= 1e-9, (n_mels, T, pad)
        assert (env[:pad] == 0).all()
        if T > pad + 2:
            assert rejected_bound(env, R.onset_from_mel(mel, 1e-10, 80.0, pad, aggregate, mutant="pad+1")[1], bound + 1e-5)
            if aggregate == 1 and n_mels > 2:
                assert rejected_bound(env, R.onset_from_mel(mel, 1e-10, 80.0, pad, 1, mutant="rank+1")[1], bound + 1e-5)


@pytest.mark.parametrize("n_frames", (16, 33))
@pytest.mark.parametrize("margin,power", [(1.0, 2.0), (8.0, 2.0), (1.0, 1.5)])
def test_hpss_twin_against_oracle_and_conditions(n_frames, margin, power):
    D = R.hpss_input(n_frames, n_frames)
    res = R.hpss(D, margin, power)
    h, p, Zs = res["h"], res["p"], res["Z"]
    assert 0 < res["hyp_dev"] <= 8 * R.V and res["pow_dev"] <= 16 * R.V and (res["bh"] >= 0).all()
    oh, op = O.hpss(torch.from_numpy(D.astype(np.complex128).T.copy()), power=power, margin=margin)
    for got, want in ((h, oh), (p, op)):
        w = want.T.numpy()
        assert np.abs(got[..., 0] - w.real).max() <= 1e-12 and np.abs(got[..., 1] - w.imag).max() <= 1e-12
    for Z in Zs:                                         # soft masks: Z is 0 or far above tiny - never near the branch
        assert ((Z == 0) | (Z > 1e-3)).all() and (Z == 0).any() and (Z > 0).any()
    # an isolated value inside the zero region: both medians are 0 there, the mask is 0.5 (margin 1) or 0, and D is not 0
    f0 = n_frames // 3
    assert Zs[0][f0, 30] == 0 and Zs[1][f0, 30] == 0 and D[f0, 30] != 0
    assert np.array_equal(h[f0, 30], (0.5 if margin == 1 else 0.0) * np.array([1.5, -0.5]))


# ---------------------------------------------------------------------------------------------------------------- feature kernels
def test_feature_twins_and_mutants():
    rng = np.random.default_rng(0)
    a, b = rng.integers(-8, 9, size=(17, 100)), rng.integers(-8, 9, size=(33, 100))
    c, _ = R.matmul_nt(a, b)
    assert np.array_equal(c, (torch.from_numpy(a) @ torch.from_numpy(b).T).numpy())
    assert R.sums_exact(R.f64(a)[:, None, :] * R.f64(b)[None])
    # fir_decimate against conv1d, and `left` off by one
    for stride in (1, 2, 3):
        for left in (0, 6, 12):
            x = rng.integers(-16, 17, size=50).astype(np.float64)
            taps = rng.integers(-4, 5, size=7) / 8.0
            n_out = 50 // stride + 8
            got = R.fir_decimate(x, taps, stride, left, 0.5, n_out)
            padded = np.concatenate((np.zeros(left), x, np.zeros(n_out * stride + 8)))
            want = 0.5 * F.conv1d(torch.from_numpy(padded)[None, None], torch.from_numpy(taps)[None, None], stride=stride)[0, 0, :n_out].numpy()
            assert np.array_equal(got, want)
            assert R.sums_exact(np.abs(taps)[None] * 16.0)
            for m in ("left+1", "left-1"):
                assert rejected_exact(got, R.fir_decimate(x, taps, stride, left, 0.5, n_out, mutant=m))
    # autocorrelation against numpy.correlate
    e, w = rng.integers(0, 8, size=300).astype(np.float64), rng.integers(0, 3, size=257) / 2.0
    ac = R.autocorr_frames(e, w, 4, 257, 257)
    for f in range(4):
        fr = w * e[f:f + 257]
        assert np.array_equal(ac[f], np.correlate(fr, fr, "full")[256:])
    assert R.sums_exact((w.max() * e.max()) ** 2 * np.ones((1, 257)))
    # overlap_add against torch's fold-style accumulation
    W, hop, nf = 8, 3, 5
    frames = rng.integers(-8, 9, size=(nf, W)).astype(np.float64)
    win = np.array([0, 0.5, 1, 1, 0.5, 0, 0, 0])
    y, num, den = R.overlap_add(frames, W, hop, win, 2, 30)
    full_n, full_d = np.zeros(64), np.zeros(64)
    for f in range(nf):
        full_n[f * hop:f * hop + W] += frames[f]
        full_d[f * hop:f * hop + W] += win ** 2
    assert np.array_equal(num, full_n[2:32]) and np.array_equal(den, full_d[2:32])
    assert (y[den == 0] == 0).all() and (den == 0).any()
    # band_sorted_means against numpy
    spec = rng.integers(-5, 6, size=(3, 1100)) * np.where(rng.integers(0, 2, size=(3, 1100)) == 1, 1j, 1)
    v, p = R.band_sorted_means(spec, 0, 1024, 1024)
    mags = np.sort(np.abs(spec[:, :1024]), axis=1)
    assert np.array_equal(v, p) and np.array_equal(R.f64(v), mags.sum(1) / 1024)
    v, p = R.band_sorted_means(spec, 501, 1100, 2)
    mags = np.sort(np.abs(spec[:, 501:1100]), axis=1)
    assert np.array_equal(R.f64(v), mags[:, :2].mean(1)) and np.array_equal(R.f64(p), mags[:, -2:].mean(1))


# ---------------------------------------------------------------------------------------------------------------- further features
@pytest.mark.parametrize("nb", (1, 255, 256, 257, 513))
def test_plp_twin_and_its_gap(nb):
    ft, fq, lo, hi = R.plp_input(nb, nb)
    out, gap = R.plp_select(ft, fq, lo, hi)
    z = torch.from_numpy(ft.astype(np.complex128).T.copy())                   # the reference's steps on [bins][frames], float64
    f = torch.from_numpy(fq)
    z[f < lo] = 0
    z[f > hi] = 0
    mag = torch.log1p(1e6 * z.abs())
    z[mag < mag.max(0, keepdim=True).values] = 0
    z = z / (float(R.SQRT_TINY) + z.abs().max(0, keepdim=True).values)
    assert np.abs(z.T.numpy() - out.astype(np.complex128)).max() <= 2 * R.V
    assert (out[0] == 0).all() and nb == 1 or (np.abs(out) > 0).sum(1).tolist() == [0, 1, 2, 1]
    # the selection is unambiguous: the gap exceeds twice what log1pf, hypotf and the product can move a value
    mags = np.abs(ft.astype(np.complex128))
    dev = 4 * R.measured_dev(np.log1p, np.log1p, [1e6 * mags], relative=False) + 4 * R.measured_dev(np.hypot, np.hypot, [ft.real, ft.imag]) + R.V
    assert (gap > 2 * dev).all() and gap.min() > 0.5


@pytest.mark.parametrize("nb", (1, 2, 3, 257))
def test_piptrack_twin(nb):
    S = R.piptrack_input(4, nb, nb)
    freqs = R.f32(np.arange(nb) * 10.0)
    for fmin, fmax in ((0.0, 1e9), (10.0, float(freqs[-1]))):
        pitch, mag, ok, _, _ = R.piptrack(S, S.max(1), 0.5, freqs, 10.0, fmin, fmax)
        St = torch.from_numpy(S.astype(np.float64)).T                            # the reference's layout [bins][frames]
        avg = 0.5 * (St[2:] - St[:-2])
        shift = 2 * St[1:-1] - St[2:] - St[:-2]
        shift = avg / (shift + (shift.abs() < R.TINY))
        avg, shift = F.pad(avg, (0, 0, 1, 1)), F.pad(shift, (0, 0, 1, 1))
        if nb < 3:
            avg, shift = torch.zeros_like(St), torch.zeros_like(St)
        x = St * (St > 0.5 * St.max(0).values)
        xp = F.pad(x, (0, 0, 1, 1))
        lm = (x > xp[:-2]) & (x >= xp[2:])
        fm = ((fmin <= torch.from_numpy(freqs)) & (torch.from_numpy(freqs) < fmax)).reshape(-1, 1)
        sel = (lm & fm).T.numpy()
        assert np.array_equal(sel, ok)
        want_p = np.where(sel, ((torch.arange(nb).reshape(-1, 1) + shift) * 10.0).T.numpy(), 0)
        want_m = np.where(sel, (St + 0.5 * avg * shift).T.numpy(), 0)
        assert np.array_equal(want_p, pitch) and np.array_equal(want_m, mag)
        if fmin == 0:
            if nb == 2:
                assert ok[0::2, 0].all() and ok[1::2, 1].all() and ok.sum() == 4
            else:
                assert ok[:, 0].all() and ok[:, -1].all()                        # peaks at the first and the last bin
        elif nb > 2:
            assert not ok[:, 0].any() and not ok[:, -1].any() and (nb < 4 or ok[:, 1:-1].any())
    if nb == 257:
        pitch, mag, ok, _, _ = R.piptrack(S, S.max(1), 0.5, freqs, 10.0, 0.0, 1e9)
        assert ok[0, 4] and not ok[0, 5] and not ok[1, 4:9].any() and not ok[2, 9:11].any()


@pytest.mark.parametrize("nk", (2, 3, 9))
def test_spline_twin_preconditions_and_mutant(nk):
    x, knots, coef = R.spline_input(nk, nk)
    r = R.spline_step(x, knots, coef, 0.25, 20.0, 0)
    t, y = torch.from_numpy(x.astype(np.float64)), torch.from_numpy(knots.astype(np.float64))
    idx = (torch.bucketize(t, y) - 1).clamp(0, nk - 2)
    f = t - y[idx]
    c = torch.from_numpy(coef.astype(np.float64))
    want = c[0, idx] + (c[1, idx] + (c[2, idx] + c[3, idx] * f) * f) * f
    assert np.array_equal(want.numpy(), r["w"])
    # exact: every product and sum of the Horner steps is a float32 number (so contraction changes nothing)
    f_, i_ = r["f"], r["idx"]
    s3 = coef[3, i_] * f_
    s2 = (coef[2, i_] + s3) * f_
    s1 = (coef[1, i_] + s2) * f_
    for v in (s3, coef[2, i_] + s3, s2, coef[1, i_] + s2, s1, r["w"]):
        assert np.array_equal(R.f64(R.f32(v)), v)
    assert nk == 2 or rejected_exact(r["w"], R.spline_step(x, knots, coef, 0.25, 20.0, 0, mutant="right")["w"])
    rs = R.spline_step(x, knots, coef, 0.25, 20.0, 1)
    m = 1 / (1 + np.exp(-20.0)) - 0.5
    want = 0.25 * (torch.floor(want - 0.5) + 1 / (2 * m) / (1 + torch.exp(-40.0 * ((want - 0.5) - torch.floor(want - 0.5) - 0.5))))
    assert np.abs(want.numpy() - rs["out"]).max() <= 1e-15
    assert rs["dist"].min() > 1e-3                       # w - 0.5 stays away from the steps of floor (w itself is exact: its bound is 0)


def test_flatness_and_single_kernel_twins():
    rng = np.random.default_rng(0)
    for nb in (1, 255, 256, 257, 1025):
        z = (R.f32(rng.normal(size=(3, nb))) + 1j * R.f32(rng.normal(size=(3, nb)))).astype(np.complex64)
        z[1] = 0
        for power in (2.0, 1.5):
            r = R.spectral_flatness(z, 1e-10, power)
            v = torch.clamp(torch.from_numpy(z.astype(np.complex128)).abs() ** power, min=1e-10)
            want = torch.exp(torch.log(v).mean(1)) / v.mean(1)
            assert np.abs(want.numpy() - r["out"]).max() <= 1e-12 and abs(r["out"][1] - 1) <= 1e-12
            if nb > 1:
                assert rejected_bound(r["out"], R.spectral_flatness(z, 1e-10, power, mutant="drop_last_bin")["out"], r["bound"])
    x = R.f32(rng.uniform(-1, 1, 257))
    y, bound, _ = R.contrast(x, 75.0)
    t = x.astype(np.float64) * np.pi / 2
    assert np.abs(y - np.sin(t + 0.1 * np.sin(4 * t))).max() <= 1e-6 and bound.max() < 1e-6
    a, b, t = (R.f32(rng.uniform(0.1, 0.9, 257)) for _ in range(3))
    t[:2] = (0, 1)
    a[2], b[3] = 0, 0
    y0 = R.eerp(a, b, t, 0)[0]
    assert y0[0] == a[0] and y0[1] == b[1] and y0[2] == 0 and y0[3] == 0
    y1 = R.eerp(a, b, t, 1)[0]
    at, bt = a.astype(np.float64) ** t, b.astype(np.float64) ** t
    assert np.array_equal(y1, at * (1 - bt) / (1 - at + bt))
    assert np.array_equal(R.threshold_scale32(x, 0.25, 0.5, 0), np.where(x > 0.25, x * np.float32(0.5), x))
    xn = R.normalize32(x, 0.0)
    y, bound, _ = R.emphasize(xn, -2.0, 3.0, 0.4, 5.0)
    want = xn.astype(np.float64) * (1 + np.tanh(5.0 * (xn.astype(np.float64) - float(np.float32(0.4))))) * 5.0 - 2.0
    assert np.array_equal(y, want) and bound.max() < 1e-5


@pytest.mark.parametrize("N", (2, 64, 1024, 2048, 4096, 8192))
def test_rectangular_window_family_is_exact_in_the_transform(N):
    """on the float32 emulation of the Stockham network: a constant and an alternating frame give N c in bin 0 / N / 2 and exact zeros
    elsewhere - every subtraction but the last stage's is exactly 0 and the only twiddle that meets a nonzero value is (1, 0); a random
    frame stays inside the bound the GPU test uses"""
    twn = 2048 if N <= 2048 else 8192
    for c in (3.0, -5.0):
        X, used = R.stockham32(np.full(N, c), twn)
        want = np.zeros(N)
        want[0] = N * c
        assert np.array_equal(X, want) and used == set()
        for sign in (1.0, -1.0):
            X, used = R.stockham32(sign * c * (-1.0) ** np.arange(N), twn)
            want = np.zeros(N)
            want[N // 2] = sign * N * c
            assert np.array_equal(X, want) and used <= {0}
    x = R.signal(N, N)
    X, _ = R.stockham32(x, twn)
    ref = np.fft.fft(x.astype(np.float64))
    err = np.sqrt((np.abs(X - ref)[:N // 2 + 1] ** 2).sum())
    bound = R.stft_bound(ref[None, :N // 2 + 1], int(np.log2(N)))[0]
    assert 0 < err <= bound


def test_overlap_add_and_autocorr_preconditions():
    """at the GPU test's inputs: integer frames and a dyadic window make numerator and denominator exact (one division rounds);
    an integer envelope under a window of halves makes every product and partial sum of the autocorrelation exact"""
    rng = np.random.default_rng(6)
    frames = rng.integers(-8, 9, size=(5, 8)).astype(np.float32)
    win = np.array([0, 0.5, 1, 1, 0.5, 0, 0, 0], np.float32)
    assert R.products_exact(win, win) and R.sums_exact(np.tile(win.astype(np.float64) ** 2, 5)[None]) and R.sums_exact(np.abs(frames).reshape(1, -1))
    for hop in (1, 3, 8, 10):
        y, num, den = R.overlap_add(frames, 8, hop, win, 0, 4 * hop + 11)
        assert np.array_equal(R.f64(R.f32(num)), num) and np.array_equal(R.f64(R.f32(den)), den)
        assert ((den == 0) | (den >= 0.25)).all()        # nowhere near the 1e-11 threshold
    rng = np.random.default_rng(4)
    for W in (1, 2, 255, 256, 257, 1000):
        e, w = rng.integers(0, 8, size=3 + W - 1).astype(np.float32), (rng.integers(0, 3, size=W) / 2.0).astype(np.float32)
        fr = np.stack([w.astype(np.float64) * e[f:f + W] for f in range(3)])
        assert R.products_exact(w, e[:W]) and R.products_exact(fr, fr) and R.sums_exact(fr * fr.max())
