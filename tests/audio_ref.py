"""The float64 twin of the audio analysis kernels (csrc/audio.hip, csrc/features.hip), in plain numpy: for every entry point that
tests/test_gpu_audio_kernels.py pins, a float64 result written from the formula in the header (include/maua_hip.h) and in the
kernels' header comments, a float32 restatement where the operation order is part of the contract (normalize, clamp, threshold_scale,
the three interpolation modes of order_stat, overlap_add's single division, band_sorted_means' ascending sums, plp_select's
division), and the bound of the random family as a function of the operands.  The inputs of both test files are generated here too,
so that what the host test proves about an input is proved about the one the GPU test uploads.  tests/test_audio_host.py holds this file against torch, numpy and the oracle, proves the
preconditions of the exact families and shows that the comparisons reject off-by-one mutants of it (the `mutant=` arguments).

v = 2^-24 throughout (half a unit in the last place of float32)."""
import numpy as np

V = 2.0 ** -24
F32 = np.float32
TINY = float(np.finfo(np.float32).tiny)
PAD = {"circular": 0, "reflect": 1, "replicate": 2, "constant": 3}
_NPMODE = {0: "wrap", 1: "reflect", 2: "edge", 3: "constant"}


def f32(a):
    return np.asarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------------- framing
def reflect_index(i, n, mutant=None):
    """torch's 'reflect' padding: no edge repeat (mutant 'edge_repeat': numpy's 'symmetric')"""
    i = np.asarray(i)
    if mutant == "edge_repeat":
        return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


def hann(n):
    """periodic Hann as the library tabulates it: float64 formula, stored as float32"""
    return f64(f32(0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n) / n)))


def frames_of(y, n_fft, hop, mutant=None):
    """centred, reflect-padded frames [1 + n // hop][n_fft] of y"""
    y = f64(y)
    n = y.size
    nf = 1 + n // hop
    off = {"offset+1": 1, "offset-1": -1}.get(mutant, 0)
    idx = np.arange(nf)[:, None] * hop - n_fft // 2 + np.arange(n_fft)[None, :] + off
    fr = y[np.clip(reflect_index(idx, n, mutant), 0, n - 1)]
    return fr[:-1] if mutant == "drop_last" else fr


def stft(y, n_fft=2048, hop=1024, win=None, mutant=None):
    """[frames][n_fft / 2 + 1] complex128 and the frames' windowed samples"""
    win = hann(n_fft) if win is None else f64(win)
    xw = frames_of(y, n_fft, hop, mutant) * win
    return np.fft.rfft(xw, axis=1), xw


def fft_eps(log_n):
    """Higham (Accuracy and Stability of Numerical Algorithms, 24.2): a radix-2 FFT of 2^t points whose twiddles carry an error mu
    has ||X^ - X||_2 <= t eta / (1 - t eta) ||X||_2, eta = mu + gamma_4 (sqrt 2 + mu); twiddles rounded from double: mu = v."""
    g4 = 4 * V / (1 - 4 * V)
    eta = V + g4 * (np.sqrt(2.0) + V)
    return log_n * eta / (1 - log_n * eta)


def stft_bound(spec, log_n):
    """per frame, on the 2-norm over the stored bins: the transform's bound plus the window product's rounding"""
    return (fft_eps(log_n) + V) * np.sqrt((np.abs(spec) ** 2).sum(1))


def istft(spec, length, n_fft=2048, hop=1024, win=None, spec_err=None):
    """y[t] = sum_f frame_f[p - f hop] / sum_f win[p - f hop]^2, p = t + n_fft / 2, frame_f = irfft(spec_f) win; 0 where no frame
    covers p.  Returns (y, bound): per sample, the inverse transform's 2-norm bound of every covering frame (an element's error is at
    most the vector's), the 1 / n_fft and window products (2 v), the sums and the division."""
    spec = np.asarray(spec, dtype=np.complex128).copy()
    win = hann(n_fft) if win is None else f64(win)
    spec[:, 0] = spec[:, 0].real
    spec[:, -1] = spec[:, -1].real
    x = np.fft.irfft(spec, n=n_fft, axis=1)
    nf = spec.shape[0]
    eps = fft_eps(int(np.log2(n_fft)))
    xnorm = np.sqrt((x ** 2).sum(1))
    y, bound = np.zeros(length), np.zeros(length)
    for t in range(length):
        p = t + n_fft // 2
        fs = [f for f in range(max(0, (p - n_fft) // hop), min(nf - 1, p // hop) + 1) if 0 <= p - f * hop < n_fft]
        if not fs:
            continue
        o = np.array([p - f * hop for f in fs])
        num = (x[fs, o] * win[o]).sum()
        den = (win[o] ** 2).sum()
        if den <= 0:
            continue
        enum = (np.abs(win[o]) * (eps * xnorm[fs] + 3 * V * np.abs(x[fs, o]))).sum() + len(fs) * V * np.abs(x[fs, o] * win[o]).sum()
        if spec_err is not None:
            enum += (np.abs(win[o]) * np.sqrt(2.0 / n_fft) * np.asarray(spec_err)[fs]).sum() * (1 + eps)
        y[t] = num / den
        bound[t] = enum / den + (len(fs) + 3) * V * abs(num / den)
    return y, bound


# ----------------------------------------------------------------------------------------------------------------- medians, HPSS
def median31(mag, axis, mutant=None, K=31):
    """median of K along time (axis 0) or frequency (axis 1) of mag [frames][bins], reflect padding K // 2"""
    mag = np.asarray(mag)
    n = mag.shape[axis]
    idx = reflect_index(np.arange(n)[:, None] + np.arange(K)[None, :] - K // 2, n, mutant)
    w = np.take(mag, idx, axis=axis)                    # axis 0: [n][K][bins]; axis 1: [frames][n][K]
    rank = K // 2 + {"rank+1": 1, "rank-1": -1}.get(mutant, 0)
    return np.sort(w, axis=axis + 1).take(rank, axis=axis + 1)


def softmask(X, Xref, power, split_zeros):
    """(mask, Z): X^p / (X^p + Xref^p) over Z = max(X, Xref); where Z < tiny: 0.5 if split_zeros else 0"""
    Z = np.maximum(X, Xref)
    bad = Z < TINY
    Zs = np.where(bad, 1.0, Z)
    m, r = (X / Zs) ** power, (Xref / Zs) ** power
    return np.where(bad, 0.5 if split_zeros else 0.0, m / np.where(bad, 1.0, m + r)), Z


def hpss(D, margin, power):
    """D [frames][1025] complex (float32 values).  A dict: h, p (the harmonic / percussive outputs as [..., 2] reals: mask D), bh, bp
    (their bounds), Z (the two soft-mask denominators), hyp_dev / pow_dev (4 x the measured deviations of hypotf and powf).
    The kernel's order: S = hypotf (relative deviation d), the medians select (an order statistic moves no further than its inputs: d
    again), a = X / Z and b = Xref / Z (one of them is exactly 1), squares or powf, m / (m + r), then (S mask) (D / S)."""
    D = np.asarray(D, dtype=np.complex128)
    S = np.abs(D)
    harm, perc = median31(S, 0), median31(S, 1)
    d = 4 * measured_dev(np.hypot, np.hypot, [D.real, D.imag])
    res = {"hyp_dev": d, "pow_dev": 0.0, "Z": []}
    ri = np.abs(np.stack((D.real, D.imag), -1))
    for name, X, Y in (("h", harm, perc), ("p", perc, harm)):
        mask, Z = softmask(X, Y * margin, power, margin == 1)
        ra = (1 + d) * (1 + V) / ((1 - d) * (1 - V)) - 1         # a or b: both medians at d, the margin product and the division
        pd = V
        if power != 2:
            Zs = np.where(Z < TINY, 1.0, Z)
            pd = 4 * measured_dev(np.power, np.power, [np.concatenate(((X / Zs).ravel(), (Y * margin / Zs).ravel())), np.float32(power)])
            res["pow_dev"] = max(res["pow_dev"], pd)
        rho = (1 + power * ra * (1 + ra) ** max(power - 1, 1)) * (1 + pd) - 1
        e0 = 2 * rho / (1 - rho) * mask * (1 - mask)             # m (1 + s) / (m (1 + s) + r (1 + t)), |s|, |t| <= rho
        emask = e0 + ((1 + V) ** 2 - 1) * (mask + e0)            # the sum and the division of m / (m + r)
        scale = (1 + V) ** 3 - 1                                 # S mask, D / S, their product (S itself cancels)
        res[name] = mask[..., None] * np.stack((D.real, D.imag), -1)
        res["b" + name] = (emask * (1 + scale) + mask * scale)[..., None] * ri
        res["Z"].append(Z)
    return res


# ----------------------------------------------------------------------------------------------------------------- mel, onsets
def mel_power(D, basis, mutant=None):
    """mel[m][f] = sum_k basis[m][k] |D[f][k]|^2; (mel, bound): (1025 + 4) v sum_k |basis| |D|^2"""
    P = np.abs(np.asarray(D, dtype=np.complex128)) ** 2
    B = f64(basis)
    if mutant == "drop_last_bin":
        P = P[:, :-1]
        B = B[:, :-1]
    mel = B @ P.T
    if mutant == "drop_last_row":
        mel[-1] = 0
    return mel, (P.shape[1] + 4) * V * (np.abs(B) @ P.T)


def onset_from_mel(mel, amin, top_db, pad_width, aggregate, log_dev=0.0, mutant=None):
    """(db, env, bound): db = max(10 log10(max(amin, mel)), max(db) - top_db); env[f] = mean (0) or lower median (1) over mels of
    relu(db[:, c + 1] - db[:, c]), c = f - pad_width, 0 where c < 0; cropped to T.  log_dev: the absolute deviation allowed to log10f.
    Per value: both dB values carry 10 log_dev + v |db| (the floor adds its subtraction's rounding), their difference v."""
    mel = f64(mel)
    n_mels, T = mel.shape
    raw = 10.0 * np.log10(np.maximum(amin, mel))
    floor = raw.max() - top_db
    db = np.maximum(raw, floor)
    e_db = 10.0 * log_dev + V * np.abs(raw).max() + V * abs(floor)
    env, bound = np.zeros(T), np.zeros(T)
    pw = pad_width + {"pad+1": 1}.get(mutant, 0)
    for f in range(T):
        c = f - pw
        if c < 0 or c + 1 >= T:
            continue
        val = np.maximum(db[:, c + 1] - db[:, c], 0.0)
        e_val = 2 * e_db + V * val
        if aggregate == 0:
            env[f] = val.mean()
            bound[f] = e_val.mean() + (n_mels + 1) * V * val.mean()
        else:
            rank = (n_mels - 1) // 2 + {"rank+1": 1}.get(mutant, 0)
            env[f] = np.sort(val)[min(rank, n_mels - 1)]
            bound[f] = e_val.max()
    return db, env, bound


# ----------------------------------------------------------------------------------------------------------------- envelope kernels
def normalize32(x, eps):
    """(x - min) / ((max - min) + eps), every operation rounded to float32 in this order"""
    x = f32(x)
    with np.errstate(all="ignore"):
        mn, mx = x.min(), x.max()
        return (x - mn) / F32(F32(mx - mn) + F32(eps))


def clamp32(x, lo, hi, hi_add):
    """min(max(x, lo), hi + hi_add), NaN propagates"""
    x = f32(x)
    h = F32(F32(hi) + F32(hi_add))
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x), x, np.minimum(np.maximum(x, F32(lo)), h)).astype(np.float32)


def peak_mask(x, mutant=None):
    """x[i] > x[i + 1] and x[i] > x[i - 1], neighbours clamped to the ends (so n = 1 has no peak)"""
    x = np.asarray(x)
    nxt, prv = np.concatenate((x[1:], x[-1:])), np.concatenate((x[:1], x[:-1]))
    if mutant == ">=":
        return ((x >= nxt) & (x >= prv)).astype(np.uint8)
    return ((x > nxt) & (x > prv)).astype(np.uint8)


def rms(y, frame_length, hop, n_frames, mutant=None):
    """out[f] = sqrt(mean(frame_f^2)) over centred reflect-padded frames; float64"""
    fr = frames_of(y, frame_length, hop, mutant)
    assert n_frames <= fr.shape[0] or mutant
    return np.sqrt((fr[:n_frames] ** 2).mean(1))


# ----------------------------------------------------------------------------------------------------------------- Gaussian filter
def gaussian_filter1d(x, taps, radius, mode, mutant=None):
    """depthwise correlation along axis 0 of x [T][C]: min(radius, T) samples each side padded with `mode`, the rest by replicating
    the edge of that padded array.  float64 (exact for the integer / dyadic family)."""
    x = f64(x)
    T = x.shape[0]
    inner = radius if mutant == "full_radius" else min(radius, T)
    if mutant == "full_radius" and mode == PAD["reflect"]:
        inner = min(radius, T - 1)
    extra = radius - inner
    p = np.pad(x, ((inner, inner), (0, 0)), mode=_NPMODE[mode]) if inner else x
    p = np.pad(p, ((extra, extra), (0, 0)), mode="edge") if extra else p
    taps = f64(taps)
    out = np.zeros_like(x)
    for k in range(2 * radius + 1):
        out += taps[k] * p[k:k + T]
    return out


def binomial_taps(radius):
    """the row 2 radius of Pascal's triangle over 2^(2 radius): dyadic, sums to 1 (radius <= 8)"""
    row = np.array([1.0])
    for _ in range(2 * radius):
        row = np.convolve(row, [1.0, 1.0])
    return row / 2.0 ** (2 * radius)


# ----------------------------------------------------------------------------------------------------------------- order statistics
def order_stat(x, mask, mode, q, k, mutant=None):
    """exact order statistics of the non-NaN, unmasked elements.  Returns (out3 float32, ranks int64).
    mode 0: lo = trunc, hi = ceil of (double)(float)q (n - 1); the midpoint in double, rounded once;
    mode 1: the k-th smallest (1-based);  mode 2: rank = float32 q * float32 (n - 1), float32 lerp as torch.quantile computes it."""
    x = f32(x).ravel()
    keep = ~np.isnan(x)
    if mask is not None:
        keep &= np.asarray(mask).ravel() != 0
    s = np.sort(x[keep])
    n = s.size
    if n == 0:
        return np.full(3, np.nan, np.float32), np.array([-1, -1], np.int64)
    with np.errstate(all="ignore"):
        if mode == 0:
            pos = float(F32(q)) * (n - 1)
            lo, hi = int(pos), int(np.ceil(pos))
        elif mode == 1:
            lo = hi = k - 1
        else:
            pos = F32(q) * F32(n - 1)
            lo, hi = int(np.floor(pos)), int(np.ceil(pos))
        lo, hi = min(lo, n - 1), min(hi, n - 1)
        if mutant == "swap":
            lo, hi = hi, lo
        a, b = s[lo], s[hi]
        if mode == 0:
            # the reference's lerp in double, also where lo == hi: a + 0 (b - a), which is NaN for an infinite a (its own behaviour)
            v = F32(float(b) - (float(b) - float(a)) * 0.5) if hi > lo else F32(float(a) + 0.0 * (float(b) - float(a)))
        elif mode == 1:
            v = a
        else:
            w = F32(pos - np.floor(pos))
            diff = F32(b - a)
            v = F32(a + F32(w * diff)) if w < 0.5 else F32(b - F32(diff * F32(F32(1) - w)))
    return np.array([v, a, b], np.float32), np.array([lo, hi], np.int64)


# ----------------------------------------------------------------------------------------------------------------- feature kernels
def matmul_nt(a, b):
    """(a b^T, bound): (K + 1) v sum |a| |b|"""
    a, b = f64(a), f64(b)
    return a @ b.T, (a.shape[1] + 1) * V * (np.abs(a) @ np.abs(b).T)


def autocorr_frames(env_padded, window, n_frames, W, n_lags):
    """ac[f][l] = sum_{n < W - l} (w[n] e[f + n]) (w[n + l] e[f + n + l])"""
    e, w = f64(env_padded), f64(window)
    ac = np.zeros((n_frames, n_lags))
    for f in range(n_frames):
        fr = w * e[f:f + W]
        for lag in range(n_lags):
            ac[f, lag] = (fr[:W - lag] * fr[lag:]).sum()
    return ac


def fir_decimate(x, taps, stride, left, scale, n_out, mutant=None):
    """out[i] = scale sum_k taps[k] x[i stride + k - left], zero outside the signal"""
    x, taps = f64(x), f64(taps)
    left = left + {"left+1": 1, "left-1": -1}.get(mutant, 0)
    out = np.zeros(n_out)
    for i in range(n_out):
        j = i * stride - left + np.arange(taps.size)
        ok = (j >= 0) & (j < x.size)
        out[i] = scale * (taps[ok] * x[j[ok]]).sum()
    return out


def overlap_add(frames, W, hop, window, start, length):
    """y[t] = sum_f frames[f][p - f hop] / sum_f window[p - f hop]^2, p = t + start; 0 where the denominator is <= 1e-11.
    Returns (num, den) in float64 too: with integer frames and a dyadic window both are exact and float32(num) / float32(den),
    rounded once, is the whole result."""
    frames, window = f64(frames), f64(window)
    nf = frames.shape[0]
    num, den = np.zeros(length), np.zeros(length)
    for t in range(length):
        p = t + start
        for f in range(nf):
            o = p - f * hop
            if 0 <= o < W:
                num[t] += frames[f, o]
                den[t] += window[o] ** 2
    with np.errstate(all="ignore"):
        y = np.where(den > 1e-11, f32(num) / f32(np.where(den > 1e-11, den, 1)), F32(0)).astype(np.float32)
    return y, num, den


def band_sorted_means(spec, lo, hi, k):
    """per frame: |spec[f][lo:hi]| sorted ascending; the means of the first and of the last k, summed in ascending order in float32
    (torch.mean over the sorted slice); the magnitudes must be exact (axis-aligned values)"""
    mag = np.sort(np.abs(np.asarray(spec, dtype=np.complex128))[:, lo:hi], axis=1)
    assert np.array_equal(f64(f32(mag)), mag)
    mag = f32(mag)
    valley, peak = np.zeros(mag.shape[0], np.float32), np.zeros(mag.shape[0], np.float32)
    for f in range(mag.shape[0]):
        s = F32(0)
        for v in mag[f, :k]:
            s = F32(s + v)
        valley[f] = s / F32(k)
        s = F32(0)
        for v in mag[f, mag.shape[1] - k:]:
            s = F32(s + v)
        peak[f] = s / F32(k)
    return valley, peak


# ----------------------------------------------------------------------------------------------------------------- preconditions
def sums_exact(terms, axis=-1):
    """every partial sum of `terms` along `axis`, in any order, is exact in float32: all terms are integer multiples of one 2^-k and the
    sum of their magnitudes stays below 2^(24 - k)"""
    t = np.abs(f64(terms))
    nz = t[t > 0]
    if nz.size == 0:
        return True
    k = 0
    while k < 60 and not np.array_equal(np.floor(nz * 2.0 ** k), nz * 2.0 ** k):
        k += 1
    return k < 60 and bool((t.sum(axis) * 2.0 ** k < 2.0 ** 24).all())


def products_exact(a, b):
    """a * b is a float32 number (so a contracted multiply-add rounds the same sum as a separate one)"""
    p = f64(a) * f64(b)
    return bool(np.array_equal(f64(f32(p)), p))


def measured_dev(fn32, fn64, args, relative=True):
    """the project's convention for a device library function: the float32 CPU function against float64 over the case's own
    arguments; 4 x the largest deviation is what a bound may allow"""
    a32 = [f32(a) for a in args]
    with np.errstate(all="ignore"):
        got = f64(fn32(*a32))
        want = fn64(*[f64(a) for a in a32])
    ok = np.isfinite(want) & np.isfinite(got)
    err = np.abs(got - want)[ok]
    if relative:
        err = err[np.abs(want[ok]) > 0] / np.abs(want[ok])[np.abs(want[ok]) > 0]
    return float(err.max()) if err.size else 0.0


# ----------------------------------------------------------------------------------------------------------------- the cases
STFT_N = (1025, 2048, 3000, 3 * 1024 + 1)
MEDIAN_AXIS_LEN = (16, 17, 31, 32, 40)
MEDIAN_OTHER = (1, 255, 256, 257)
MEDIAN_KINDS = ("random", "ties3", "equal", "zeros", "inf", "denormal", "ramp_up", "ramp_down")
GAUSS_T = (1, 2, 5, 40)
GAUSS_C = (1, 255, 256, 257)
ORDER_N = (0, 1, 2, 3, 255, 256, 257, 262144, 262145)
ORDER_KINDS = ("random", "ties", "equal", "zeros", "inf", "denormal", "negative", "nan", "all_nan", "low_byte", "sign")
ORDER_Q = (0.0, float(np.float32(0.025)), 0.5, 1.0)
NORM_N = (1, 2, 255, 256, 257, 65536, 65537, 262145)
MATMUL_MN = (1, 15, 16, 17, 33)
MATMUL_K = (1, 31, 32, 33, 100)


def gauss_radii(T):
    return sorted({0, 1, max(T - 1, 0), T, T + 1, 3 * T})


def signal(n, seed):
    return f32(np.random.default_rng(seed).normal(size=n))


def impulses(n):
    """unit impulses at samples 0, 1, n - 2, n - 1 and at the frame boundary 1024: one signal each"""
    out = []
    for at in (0, 1, n - 2, n - 1, 1024):
        y = np.zeros(n, np.float32)
        y[at] = 1.0
        out.append(y)
    return out


def median_input(nf, nb, kind, seed, axis=0):
    rng = np.random.default_rng(seed)
    if kind == "random":
        x = rng.normal(size=(nf, nb))
    elif kind == "ties3":
        x = rng.integers(0, 3, size=(nf, nb)).astype(np.float64)
    elif kind == "equal":
        x = np.full((nf, nb), 0.75)
    elif kind == "zeros":
        x = np.where(rng.integers(0, 2, size=(nf, nb)) == 1, 0.0, -0.0) * np.where(rng.integers(0, 3, size=(nf, nb)) == 0, 0.0, 1.0)
        x = np.where(rng.integers(0, 4, size=(nf, nb)) == 0, rng.normal(size=(nf, nb)), x)
    elif kind == "inf":
        x = rng.choice([-np.inf, np.inf, 0.0, 1.0, -1.0], size=(nf, nb))
    elif kind == "denormal":
        x = rng.integers(-8, 9, size=(nf, nb)) * 2.0 ** -149
    else:
        ramp = np.arange(nf if axis == 0 else nb, dtype=np.float64)
        ramp = ramp if kind == "ramp_up" else -ramp
        x = np.broadcast_to(ramp[:, None] if axis == 0 else ramp[None, :], (nf, nb)).copy()
    return f32(x)


def ramp_median_index(n, K=31):
    """on a strictly monotone ramp the median of the reflect-padded window around i is the value at this index: the window's sorted
    source indices are |i + j| reflected, and the middle one follows from counting"""
    idx = reflect_index(np.arange(n)[:, None] + np.arange(K)[None, :] - K // 2, n)
    return np.sort(idx, axis=1)[:, K // 2]


def order_input(n, kind, seed):
    """(x, mask or None)"""
    rng = np.random.default_rng(seed)
    if kind == "random":
        x = rng.normal(size=n)
    elif kind == "ties":
        x = rng.integers(0, 3, size=n).astype(np.float64)
    elif kind == "equal":
        x = np.full(n, -2.5)
    elif kind == "zeros":
        x = np.where(rng.integers(0, 2, size=n) == 1, 0.0, -0.0)
    elif kind == "inf":
        x = rng.choice([-np.inf, np.inf, 0.0, 3.0], size=n)
    elif kind == "denormal":
        x = rng.integers(-100, 101, size=n) * 2.0 ** -149
    elif kind == "negative":
        x = -np.abs(rng.normal(size=n)) - 1.0
    elif kind == "nan":
        x = np.where(rng.integers(0, 3, size=n) == 0, np.nan, rng.normal(size=n))
    elif kind == "all_nan":
        x = np.full(n, np.nan)
    elif kind == "low_byte":
        x = 1.0 + rng.integers(0, 256, size=n) * 2.0 ** -23
    else:
        x = np.where(rng.integers(0, 2, size=n) == 1, 1.5, -1.5)
    return f32(x)


def keep_mask(n, keep, seed):
    """a mask that keeps `keep` elements (None: no mask)"""
    if keep is None:
        return None
    m = np.zeros(n, np.uint8)
    if n:
        m[np.random.default_rng(seed).permutation(n)[:min(keep, n)]] = 1
    return m


def gauss_exact_input(T, C, radius, seed):
    """integer x and dyadic taps: the binomial row over 2^(2 radius) up to radius 8, small integers over 8 beyond"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-64, 65, size=(T, C)).astype(np.float32)
    taps = binomial_taps(radius) if radius <= 8 else rng.integers(-4, 5, size=2 * radius + 1) / 8.0
    return x, f32(taps)


def mel_exact_input(T, n_mels, seed):
    """axis-aligned spectra (a, 0) or (0, a), a a small integer, and dyadic weights: hypot and every sum are exact"""
    rng = np.random.default_rng(seed)
    a = rng.integers(-7, 8, size=(T, 1025)).astype(np.float64)
    on_im = rng.integers(0, 2, size=(T, 1025)) == 1
    D = np.where(on_im, 1j * a, a + 0j)
    D[:, 1024] = 7.0                                    # the 33rd chunk of 32 bins holds this bin alone
    basis = rng.integers(0, 5, size=(n_mels, 1025)) / 4.0
    basis[:, 1024] = 1.0
    return D, f32(basis)


def onset_input(n_mels, T, seed, constant_rows=False):
    """mel power over far more than 80 dB (the top_db floor is active); constant_rows: every row constant, the envelope exactly 0"""
    rng = np.random.default_rng(seed)
    if constant_rows:
        return f32(np.broadcast_to(10.0 ** rng.uniform(-14, 3, size=(n_mels, 1)), (n_mels, T)).copy())
    # two frames in three rise by 40 dB (then fall by 80), staggered over the rows: the median over mels is positive in every frame
    e = rng.uniform(-9, -6, size=(n_mels, 1)) + 4.0 * ((np.arange(T)[None, :] + np.arange(n_mels)[:, None]) % 3) + rng.uniform(0, 1, size=(n_mels, T))
    mel = f32(10.0 ** e)
    mel.flat[0], mel.flat[-1] = 1e-13, 1e3
    return mel


def hpss_input(n_frames, seed):
    """a spectrum with whole 31-windows of exact zeros in both directions (bins 0..99 of every frame are zero, so both medians of the
    bins below 69 are 0), one isolated value inside that region (there Z = 0 while D is not), zeros elsewhere (D = 0: phase 1), and
    magnitudes in [0.5, 2) otherwise"""
    rng = np.random.default_rng(seed)
    mag = rng.uniform(0.5, 2.0, size=(n_frames, 1025))
    ph = rng.uniform(0, 2 * np.pi, size=(n_frames, 1025))
    D = (f32(mag * np.cos(ph)) + 1j * f32(mag * np.sin(ph))).astype(np.complex64)
    D[:, :100] = 0
    D[n_frames // 2, 500:510] = 0
    D[n_frames // 3, 30] = 1.5 - 0.5j
    return D


# ----------------------------------------------------------------------------------------------------------------- further features
SQRT_TINY = np.float32(1.0842021724855044e-19)      # finfo(float32).tiny ** 0.5


def spectral_flatness(spec, amin, power, mutant=None):
    """out[f] = exp(mean(log(max(amin, |z|^power)))) / mean(max(amin, |z|^power)).  A dict: out, bound, and the measured deviations
    (4 x each is allowed) of logf (absolute), expf, powf (relative).  The kernel's fixed tree: a thread adds its ceil(n / 256) terms,
    then 8 levels - depth D additions on any path; |z| = sqrtf(x x + y y) is within 2 v, its square within 5 v."""
    z = np.asarray(spec, dtype=np.complex128)
    if mutant == "drop_last_bin":
        z = z[:, :-1]
    n = z.shape[1]
    mag = np.abs(z)
    val = np.maximum(amin, mag ** power)
    lg = np.log(val)
    ml = lg.mean(1)
    out = np.exp(ml) / val.mean(1)
    pow_dev = 4 * measured_dev(np.power, np.power, [mag, np.float32(power)]) if power != 2 else 0.0
    rv = 5 * V if power == 2 else (1 + 2 * V) ** power * (1 + pow_dev) - 1
    log_dev = 4 * measured_dev(np.log, np.log, [val], relative=False)
    exp_dev = 4 * measured_dev(np.exp, np.exp, [ml])
    D = -(-n // 256) + 8
    e_ml = (log_dev + rv / (1 - rv)) + (D + 1) * V * np.abs(lg).mean(1) / (1 - (D + 1) * V)
    rel = (1 + exp_dev) * np.exp(e_ml) * (1 + V) / (1 - rv - (D + 1) * V) - 1
    return {"out": out, "bound": rel * out, "log_dev": log_dev / 4, "exp_dev": exp_dev / 4, "pow_dev": pow_dev / 4}


def plp_select(ft, tempo_freq, tempo_min, tempo_max):
    """one tempogram frame per row: zero the bins whose tempo lies outside [tempo_min, tempo_max] (both comparisons strict), keep the
    bins at the frame's peak of log1p(1e6 |z|) - a monotone function: the bins of largest magnitude, every one of them -, divide by
    tiny ** 0.5 + that magnitude in float32.  Returns (out complex64, gap): gap[f] = the difference of log1p(1e6 |z|) between the
    largest and the second largest distinct magnitude (inf where there is none): what keeps the selection unambiguous."""
    z = np.asarray(ft, dtype=np.complex128).copy()
    fq = f32(tempo_freq)
    z[:, (fq < F32(tempo_min)) | (fq > F32(tempo_max))] = 0
    mag = np.abs(z)
    assert np.array_equal(f64(f32(mag.max(1))), mag.max(1)), "the peak's magnitude must be a float32 number (axis-aligned peaks)"
    top = mag.max(1, keepdims=True)
    keep = mag == top
    rest = np.where(keep, -1.0, mag).max(1)
    gap = np.where(rest >= 0, np.log1p(1e6 * top[:, 0]) - np.log1p(1e6 * np.maximum(rest, 0)), np.inf)
    z = np.where(keep, z, 0)
    den = (SQRT_TINY + f32(top)).astype(np.float32)
    with np.errstate(all="ignore"):
        out = (f32(z.real) / den) + 1j * (f32(z.imag) / den)
    return out.astype(np.complex64), gap


def piptrack(S, frame_max, threshold, freqs, bin_hz, fmin, fmax):
    """parabolic peak interpolation on S [frames][bins]: ref = threshold frame_max (a float32 product); a bin is a peak where its gated
    value (S where S > ref, else 0; 0 outside the spectrum) is above its left and not below its right neighbour, inside fmin <= freq <
    fmax.  avg = (S+ - S-) / 2, sh = 2 S0 - S+ - S- (+ 1 where |sh| < tiny), shift = avg / sh (both 0 at the first and last bin);
    pitch = (bin + shift) bin_hz, mag = S0 + avg shift / 2; 0 where rejected.  (pitch, mag, accepted, bound_pitch, bound_mag): with
    integer S only the division, the sum and the products round: 3 v of the terms' magnitudes."""
    S = f64(S)
    nf, nb = S.shape
    ref = f64(F32(threshold) * f32(frame_max))[:, None]
    g = np.where(S > ref, S, 0.0)
    gp = np.pad(g, ((0, 0), (1, 1)))
    lmax = (g > gp[:, :-2]) & (g >= gp[:, 2:])
    fr = f32(freqs)[None, :]
    ok = lmax & (F32(fmin) <= fr) & (fr < F32(fmax))
    avg, shift = np.zeros_like(S), np.zeros_like(S)
    if nb > 2:
        avg[:, 1:-1] = 0.5 * (S[:, 2:] - S[:, :-2])
        sh = 2 * S[:, 1:-1] - S[:, 2:] - S[:, :-2]
        sh = sh + (np.abs(sh) < TINY)
        shift[:, 1:-1] = avg[:, 1:-1] / sh
    b = np.arange(nb)[None, :]
    pitch = np.where(ok, (b + shift) * float(F32(bin_hz)), 0.0)
    mag = np.where(ok, S + 0.5 * avg * shift, 0.0)
    bp = np.where(ok, 3 * V * (b + np.abs(shift)) * float(F32(bin_hz)), 0.0)
    bm = np.where(ok, 3 * V * (np.abs(S) + np.abs(0.5 * avg * shift)), 0.0)
    return pitch, mag, ok, bp, bm


def spline_step(x, knots, coef, h, alpha, apply_step, mutant=None):
    """the piecewise cubic a + f (b + f (c + f d)), f = x - knot[i], i = (number of knots < x) - 1 clamped to [0, n_knots - 2]
    (torch.bucketize, right=False), then step(w) = h (floor(w - 0.5) + 1 / (2 m) / (1 + exp(-2 alpha r))), r = (w - 0.5) -
    floor(w - 0.5) - 0.5, m = 1 / (1 + exp(-alpha)) - 0.5.  A dict: w (the spline), out, bound (for exact w: 1 / (2 m) within 5 v -
    three roundings around m ~ 0.5 -, the exponent's product v |2 alpha r| and expf's deviation on e / (1 + e), the sum and the
    division, the last sum and product), dist (how far w - 0.5 is from an integer), exp_dev (measured)."""
    x, knots = f64(f32(x)), f64(f32(knots))
    coef = f64(f32(coef)).reshape(4, -1)
    nk = knots.size
    idx = np.searchsorted(knots, x, side="right" if mutant == "right" else "left") - 1
    idx = np.clip(idx, 0, nk - 2)
    f = x - knots[idx]
    w = coef[0, idx] + f * (coef[1, idx] + f * (coef[2, idx] + f * coef[3, idx]))
    res = {"w": w, "f": f, "idx": idx}
    if not apply_step:
        res["out"] = w
        return res
    fl = np.floor(w - 0.5)
    r = (w - 0.5) - fl - 0.5
    m = 1.0 / (1.0 + np.exp(-alpha)) - 0.5
    arg = -2.0 * alpha * r
    e = np.exp(arg)
    gsig = 1.0 / (2 * m) / (1 + e)
    exp_dev = 4 * measured_dev(np.exp, np.exp, [arg])
    rg = (1 + 5 * V) * (1 + (exp_dev + V * np.abs(arg)) * e / (1 + e) / (1 - exp_dev - V * np.abs(arg))) * (1 + V) ** 2 - 1
    res.update(out=h * (fl + gsig), bound=abs(h) * (gsig * rg * (1 + 2 * V) + ((1 + V) ** 2 - 1) * np.abs(fl + gsig)),
               dist=np.abs((w - 0.5) - np.round(w - 0.5)), exp_dev=exp_dev / 4)
    return res


def magnitude(spec, power):
    """|z|^power; (out, bound, hyp_dev, pow_dev): hypotf at 4 x its measured deviation, m m one rounding more, powf at its own"""
    z = np.asarray(spec, dtype=np.complex128)
    m = np.abs(z)
    d = 4 * measured_dev(np.hypot, np.hypot, [z.real, z.imag])
    pd = 0.0
    if power == 1:
        rel = d
    elif power == 2:
        rel = (1 + d) ** 2 * (1 + V) - 1
    else:
        pd = 4 * measured_dev(np.power, np.power, [m, np.float32(power)])
        rel = (1 + d) ** power * (1 + pd) - 1
    return m ** power, rel * m ** power, d / 4, pd / 4


def emphasize(xn, mn, mx, q, strength):
    """y = xn (1 + tanh(strength (xn - q))) (max - min) + min; (y, bound, tanh_dev): the difference, the product (v each) and tanhf's
    measured absolute deviation (its slope is at most 1), 1 + t, xn (...), then e range + min at 3 v"""
    xn = f64(f32(xn))
    mn, mx, q, s = float(F32(mn)), float(F32(mx)), float(F32(q)), float(F32(strength))
    arg = s * (xn - q)
    td = 4 * measured_dev(np.tanh, np.tanh, [arg], relative=False)
    t = np.tanh(arg)
    e = xn * (1 + t)
    y = e * (mx - mn) + mn
    e_t = td + 2 * V * np.abs(arg)
    e_e = np.abs(xn) * (e_t + V * (1 + t)) + V * np.abs(e)
    bound = abs(mx - mn) * e_e * (1 + V) + 3 * V * np.abs(e * (mx - mn)) + V * np.abs(y)
    return y, bound, td / 4


def threshold_scale32(x, threshold, ratio, invert):
    """x ratio where x > threshold (invert: x < threshold), else x: one float32 product"""
    x = f32(x)
    hit = x < F32(threshold) if invert else x > F32(threshold)
    return np.where(hit, x * F32(ratio), x).astype(np.float32)


def eerp(a, b, t, mode):
    """mode 0: a^(1 - t) b^t; mode 1: a^t (1 - b^t) / (1 - a^t + b^t).  (y, bound, pow_dev): powf at 4 x its measured deviation, the
    exponent 1 - t rounded once (v |ln a|), every product, sum and division one v on its terms' magnitudes"""
    a, b, t = f64(f32(a)), f64(f32(b)), f64(f32(t))
    with np.errstate(all="ignore"):
        if mode == 0:
            pd = 4 * max(measured_dev(np.power, np.power, [a, 1 - t]), measured_dev(np.power, np.power, [b, t]))
            y = a ** (1 - t) * b ** t
            la = np.where(a > 0, np.abs(np.log(np.where(a > 0, a, 1.0))), 0.0)
            rel = (1 + pd) ** 2 * (1 + V * la) * (1 + V) / (1 - V * la) - 1
            return y, rel * np.abs(y), pd / 4
        pd = 4 * max(measured_dev(np.power, np.power, [a, t]), measured_dev(np.power, np.power, [b, t]))
        at, bt = a ** t, b ** t
        num, den = at * (1 - bt), 1 - at + bt
        e_1b = pd * bt + V * np.abs(1 - bt)
        e_num = (at * e_1b + pd * at * np.abs(1 - bt)) * (1 + pd) + V * np.abs(num)
        e_den = pd * (at + bt) + V * (np.abs(1 - at) + np.abs(den))
        y = num / den
        bound = (e_num + np.abs(y) * e_den) / (np.abs(den) - e_den) + V * np.abs(y)
        return y, bound, pd / 4


def contrast(x, amount):
    """y = sin(t + amount / 750 sin(4 t)), t = x pi / 2: the products and the sum are single float32 operations, so t and 4 t are
    restated exactly; (y, bound, sin_dev): sinf's measured absolute deviation over both sets of arguments, the inner one scaled by
    amount / 750, plus the roundings of c sin and of the sum (the outer sine's slope is at most 1)"""
    t1 = f32(x) * F32(1.57079632679489661923)
    t4 = f64(t1 * F32(4.0))
    c = float(F32(amount) / F32(750.0))
    t2 = c * np.sin(t4)
    arg = f64(t1) + t2
    d1 = 4 * measured_dev(np.sin, np.sin, [t4], relative=False)
    d2 = 4 * measured_dev(np.sin, np.sin, [arg], relative=False)
    return np.sin(arg), c * d1 + V * np.abs(t2) + V * np.abs(arg) + d2, max(d1, d2) / 4


def piptrack_input(nf, nb, seed):
    """integer magnitudes with flat tops, values exactly at threshold * frame_max (threshold 0.5, the frame's maximum 8), peaks at the
    first and the last bin, flat stretches (2 S0 - S+ - S- = 0)"""
    rng = np.random.default_rng(seed)
    S = rng.integers(0, 8, size=(nf, nb)).astype(np.float32)
    S[:, 0] = 8
    S[:, -1] = 8
    if nb == 2:                                          # two bins cannot both be peaks: the first in the even rows, the last in the odd
        S[0::2, 1] = 6
        S[1::2, 0] = 6
    if nb > 16:
        S[0, 3:6] = (1, 5, 5)
        S[0, 6] = 1
        S[1, 4:9] = 4                                    # exactly at the reference value: gated away
        S[2, 8:12] = 6                                   # a flat stretch
        S[3 % nf, nb // 2] = 8
    return S


def spline_input(nk, seed):
    """(x, knots, coef): knots at multiples of 1 / 4, integer coefficients, x below the first knot, on every knot, inside every
    interval at dyadic offsets, above the last"""
    rng = np.random.default_rng(seed)
    knots = np.arange(nk) / 4.0
    coef = rng.integers(-3, 4, size=(4, nk - 1)).astype(np.float64)
    inside = (knots[:-1, None] + np.array([1, 2, 3, 5, 7]) / 32.0).ravel()
    x = np.concatenate(([-0.5, -1 / 32.0], knots, inside, [knots[-1] + 1 / 32.0, knots[-1] + 0.5]))
    return f32(x), f32(knots), f32(coef)


def plp_input(nb, seed):
    """(tempogram [4][nb] complex64, tempo_freq, tempo_min, tempo_max): a frame of zeros; a frame whose largest value lies outside the
    tempo band; a frame with two equal axis-aligned peaks on the band's two edge frequencies (both comparisons are strict: both kept);
    a frame of small values under one peak.  Everything that is not a peak is at most half a peak."""
    rng = np.random.default_rng(seed)
    fq = f32(np.arange(nb, dtype=np.float64))
    lo, hi = (60.0, 180.0) if nb > 200 else (0.0, float(nb - 1))
    ilo, ihi = int(lo), int(hi)
    small = (f32(rng.uniform(-2, 2, size=(4, nb))) + 1j * f32(rng.uniform(-2, 2, size=(4, nb)))).astype(np.complex64)
    ft = small.copy()
    ft[0] = 0
    ft[1, (ilo + ihi) // 2] = -8.0
    if nb > 200:
        ft[1, ilo - 1] = 64.0                           # louder, but outside the band
        ft[1, ihi + 1] = 64.0j
    ft[2, ilo] = 8.0
    ft[2, ihi] = -8.0j if ihi != ilo else ft[2, ilo]
    ft[3, min(ilo + 7, ihi)] = 16.0j
    return ft, fq, lo, hi


def stockham32(x, twn=None):
    """A float32 emulation of the transform the kernels' header describes: radix-2 Stockham, decimation in frequency, natural order in
    and out.  Stage t (stride s = 2^t): butterfly i = p s + q reads src[i] and src[i + N / 2] and writes dst[q + 2 s p] = a + b,
    dst[q + 2 s p + s] = (a - b) exp(-2 pi i p s / N), the twiddles rounded from double (a table of twn >= N entries read with stride
    twn / N).  Every operation is rounded separately.  Returns (X, used): used = the set of twiddle indices that met a nonzero a - b."""
    x = np.asarray(x)
    N = x.size
    twn = N if twn is None else twn
    ang = -2.0 * np.pi * np.arange(max(twn // 2, 1)) / twn
    twr, twi = f32(np.cos(ang)), f32(np.sin(ang))
    re, im = f32(x.real).copy(), f32(x.imag).copy() if np.iscomplexobj(x) else np.zeros(N, np.float32)
    used = set()
    t, s = 0, 1
    while s < N:
        i = np.arange(N // 2)
        p, q = i >> t, i & (s - 1)
        ur, ui, vr, vi = re[i], im[i], re[i + N // 2], im[i + N // 2]
        k = p * s * (twn // N)
        wr, wi = twr[k], twi[k]
        dr, di = ur - vr, ui - vi
        used |= set(k[(dr != 0) | (di != 0)].tolist())
        nr, ni = np.zeros(N, np.float32), np.zeros(N, np.float32)
        nr[q + 2 * s * p], ni[q + 2 * s * p] = ur + vr, ui + vi
        nr[q + 2 * s * p + s] = f32(dr * wr) - f32(di * wi)
        ni[q + 2 * s * p + s] = f32(dr * wi) + f32(di * wr)
        re, im = nr, ni
        t, s = t + 1, s * 2
    return re.astype(np.float64) + 1j * im.astype(np.float64), used
