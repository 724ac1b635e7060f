"""Host restatements for the video-feature and correlation tests (no reference code: restated from
maua/audiovisual/audioreactive/selfsupervised/features/video.py:12-75, correlation.py:14-121, 278-282, 353-382 and kornia's published
rgb_to_hsv).

  * float32: every step one correctly rounded float32 operation in the order the C header states, so the device must agree to the bit;
  * float64: what the float32 results are measured against, the correlations both in the reference's T x T form and in the reduced
    moment form the library uses;
  * the error bounds of the float32-input sums, derived below for ANY summation order in float64.
"""
import math

import numpy as np
import torch

U64 = 2.0 ** -53   # unit roundoff of float64
U32 = 2.0 ** -24   # ... of float32
LUT255 = (np.arange(256, dtype=np.float32) / np.float32(255))   # the value a byte stands for: an IEEE division, no reciprocal


def u8_to_float(frames_u8_chw):
    """uint8 [.., 3, H, W] (numpy or torch) -> float32 torch tensor, k / 255 by a true division."""
    a = frames_u8_chw.numpy() if isinstance(frames_u8_chw, torch.Tensor) else np.asarray(frames_u8_chw)
    return torch.from_numpy(LUT255[a])


# ---- float32 restatement ------------------------------------------------------------------------------------------------------------
def rgb_to_hsv_f32(video):
    """[.., 3, H, W] float32 -> (h, s, v); the first maximal channel wins a tie (written out, not left to torch.max)."""
    r, g, b = video.unbind(-3)
    mx, k = r, torch.zeros_like(r, dtype=torch.int64)
    sel = g > mx
    mx, k = torch.where(sel, g, mx), torch.where(sel, torch.ones_like(k), k)
    sel = b > mx
    mx, k = torch.where(sel, b, mx), torch.where(sel, torch.full_like(k, 2), k)
    mn = torch.minimum(torch.minimum(r, g), b)
    dc = mx - mn
    s = dc / (mx + 1e-8)
    d = torch.where(dc == 0, torch.ones_like(dc), dc)
    rc, gc, bc = mx - r, mx - g, mx - b
    h1 = bc - gc
    h2 = (rc - bc) + 2.0 * d
    h3 = (gc - rc) + 4.0 * d
    hk = torch.where(k == 0, h1, torch.where(k == 1, h2, h3))
    h = torch.remainder((hk / d) / 6.0, 1.0)
    h = (2.0 * math.pi) * h
    assert h.dtype == torch.float32 and s.dtype == torch.float32
    return h, s, mx


def rgb_to_hsv_published(video):
    """kornia.color.rgb_to_hsv as published (max / argmax over the channel axis, gather): pins the tie rule of rgb_to_hsv_f32 to torch.max on
    the CPU."""
    mx, arg = video.max(-3)
    mn = video.min(-3).values
    dc = mx - mn
    v = mx
    s = dc / (mx + 1e-8)
    dc = torch.where(dc == 0, torch.ones_like(dc), dc)
    rc, gc, bc = torch.unbind(mx.unsqueeze(-3) - video, dim=-3)
    h = torch.stack((bc - gc, (rc - bc) + 2.0 * dc, (gc - rc) + 4.0 * dc), dim=-3) / dc.unsqueeze(-3)
    h = torch.gather(h, dim=-3, index=arg.unsqueeze(-3)).squeeze(-3)
    h = (h / 6.0) % 1.0
    return 2.0 * math.pi * h, s, v


def histc_counts_f32(x, bins):
    """torch.histc(x, bins) with min = max = 0 restated: the bin rule in float32, counts as integers."""
    x = x.reshape(-1)
    assert x.dtype == torch.float32
    mn, mx = x.min(), x.max()
    if mn == mx:
        mn, mx = mn - 1, mx + 1
    pos = ((x - mn) * float(bins) / (mx - mn)).to(torch.int64)
    pos[pos == bins] = bins - 1
    return torch.bincount(pos, minlength=bins)


def features_f32(video, bins):
    """video float32 [T, 3, H, W] -> (counts int64 [T, 6, bins], hist float32 [T, 6, bins]) in the order R, G, B, H, S, V."""
    h, s, v = rgb_to_hsv_f32(video)
    planes = torch.stack((video[:, 0], video[:, 1], video[:, 2], h, s, v), dim=1)
    counts = torch.stack([torch.stack([histc_counts_f32(planes[t, c], bins) for c in range(6)]) for t in range(video.shape[0])])
    hist = counts.float() / counts.max(dim=2, keepdim=True).values.float()
    return counts, hist


# ---- float64 restatement of the scalar features ----------------------------------------------------------------------------------------
def variance_f64(video):
    """video.std((1, 2, 3)) ** 2, unbiased, in float64 -> [T]."""
    return video.double().flatten(1).var(dim=1, unbiased=True)


def diff_f64(video):
    """diff[t] = sum |frame[t] - frame[t - 1]| with diff[0] = 0: the difference in the video's own dtype (as torch.diff forms it), the sum in
    float64 -> [T]."""
    d = (video[1:] - video[:-1]).abs().double().flatten(1).sum(1)
    return torch.cat((torch.zeros(1, dtype=torch.float64), d))


def variance_u8_exact(frames_u8):
    """The unbiased variance of k / 255 over a uint8 frame batch [T, ...] from exact integers: (N S2 - S1^2) / (N (N - 1) 255^2), the quotient
    correctly rounded to float64 -> list of T floats."""
    out = []
    for f in np.asarray(frames_u8):
        k = f.astype(np.int64).reshape(-1)
        N, S1, S2 = int(k.size), int(k.sum()), int((k * k).sum())
        out.append((N * S2 - S1 * S1) / (N * (N - 1) * 65025))
    return out


def diff_u8_exact(frames_u8):
    """diff[t] of k / 255 from exact integers -> list of T floats (diff[0] = 0)."""
    a = np.asarray(frames_u8).astype(np.int64)
    return [0.0] + [int(np.abs(a[t] - a[t - 1]).sum()) / 255 for t in range(1, a.shape[0])]


def absdiff_from_diff(diff):
    return torch.cat((diff[1:], diff[-1:])).unsqueeze(-1)


# ---- error bounds of the float32-input sums --------------------------------------------------------------------------------------------
# The device accumulates sum x, sum x^2 and sum |x_t - x_{t-1}| of float32 values in float64 (per thread, then a wave butterfly, the waves,
# the workgroups: n - 1 additions in some fixed order).  Every term is exact in float64 (a float32, the square of a float32 - 48 bits - or a
# float32 difference) and non-negative, so for ANY order |S^ - S| <= gamma(n - 1) S with gamma(k) = k u / (1 - k u) (Higham, Accuracy and
# Stability of Numerical Algorithms, 4.2).
def gamma(k, u=U64):
    return k * u / (1 - k * u)


def diff_bound_f32(n, ref):
    """|float32(D^) - D| for D = sum of n non-negative terms: the float64 sum's gamma(n - 1) D, then one float32 rounding of D^."""
    e = gamma(n - 1) * abs(ref)
    return e + U32 * (abs(ref) + e)


def variance_bound_f32(n, s2, ref):
    """var^ = (S2^ - S1^ S1^ / n) / (n - 1).  S2^ = S2 (1 + a), |a| <= gamma(n - 1); S1^ S1^ / n = (S1^2 / n)(1 + b), |b| <= 2 gamma(n - 1) + 3u
    to first order (two sums, a product, a quotient); S1^2 / n <= S2 (Cauchy-Schwarz).  So the numerator is off by at most
    (3 gamma(n - 1) + 4u) S2 including its own subtraction, the quotient adds 2u |var|, and float32(var^) one float32 rounding."""
    e = (3 * gamma(n - 1) + 4 * U64) * s2 / (n - 1) + 2 * U64 * abs(ref)
    return e + U32 * (abs(ref) + e)


def device_order_sum(values):
    """One float64 summation in the order the frame pass uses: workgroups of 4096 elements, 256 threads taking every 256th element 16 times,
    a 64-lane butterfly, the 4 waves in order, the workgroups in order (csrc/video_features.hip)."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    pad = (-len(v)) % 4096
    v = np.concatenate((v, np.zeros(pad))).reshape(-1, 16, 256)
    t = np.zeros((v.shape[0], 256))
    for j in range(16):
        t = t + v[:, j]
    t = t.reshape(-1, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        t = t + t[:, :, np.arange(64) ^ o]
    w = t[:, :, 0]
    blk = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    s = 0.0
    for b in blk:
        s = s + b
    return float(s)


# ---- correlations, float64 ---------------------------------------------------------------------------------------------------------------
def _pearson_cols(X, Y):
    T = X.shape[0]
    cx, cy = X - X.mean(0, keepdim=True), Y - Y.mean(0, keepdim=True)
    cov = (cx * cy).sum(0, keepdim=True) / (T - 1)
    return cov / (X.std(0, keepdim=True) * Y.std(0, keepdim=True))


def _lower_median(v):
    return v.reshape(-1).sort().values[(v.numel() - 1) // 2]


def corr_full(name, X, Y):
    """The metric in the reference's own form (T x T matrices where it builds them), float64."""
    X, Y = X.double(), Y.double()
    T = X.shape[0]
    if name == "pearson":
        return float(_lower_median(_pearson_cols(X, Y)))
    if name == "concordance":
        r = _pearson_cols(X, Y)
        bct = (T - 1) / T
        mx, my, sx, sy = X.mean(0, keepdim=True), Y.mean(0, keepdim=True), X.std(0, keepdim=True), Y.std(0, keepdim=True)
        return float(_lower_median(2 * r * sx * sy / (sx * sx + sy * sy + (mx - my) * (mx - my) / bct)))
    X, Y = X - X.mean(0), Y - Y.mean(0)
    if name == "autocorrcorr":
        X, Y = X / X.norm(p=2, dim=1, keepdim=True), Y / Y.norm(p=2, dim=1, keepdim=True)
        i, j = torch.triu_indices(T, T, offset=1).unbind(0)
        return float(_pearson_cols((X @ X.T)[i, j].unsqueeze(1), (Y @ Y.T)[i, j].unsqueeze(1)))
    if name in ("rv", "rv2"):
        A, B = X @ X.T, Y @ Y.T
        if name == "rv2":
            A, B = A - torch.diag(torch.diag(A)), B - torch.diag(torch.diag(B))
        return float(torch.trace(A.T @ B) / torch.sqrt(torch.trace(A.T @ A) * torch.trace(B.T @ B)))
    if name == "r1":
        return float(torch.trace(X @ Y.T) / torch.sqrt(torch.trace(X @ X.T) * torch.trace(Y @ Y.T)))
    raise KeyError(name)


def corr_reduced(name, X, Y):
    """The same metric from second moments over the time axis (the library's form), float64: no T x T matrix."""
    X, Y = X.double(), Y.double()
    T = X.shape[0]
    mx, my = X.mean(0), Y.mean(0)
    X, Y = X - mx, Y - my
    Gxx, Gxy, Gyy = X.T @ X, X.T @ Y, Y.T @ Y
    if name in ("pearson", "concordance"):
        sx, sy = torch.sqrt(torch.diag(Gxx) / (T - 1)), torch.sqrt(torch.diag(Gyy) / (T - 1))
        r = torch.diag(Gxy) / (T - 1) / (sx * sy)
        if name == "pearson":
            return float(_lower_median(r))
        return float(_lower_median(2 * r * sx * sy / (sx * sx + sy * sy + (mx - my) ** 2 / ((T - 1) / T))))
    if name == "r1":
        return float(torch.trace(Gxy) / torch.sqrt(torch.trace(Gxx) * torch.trace(Gyy)))
    if name in ("rv", "rv2"):
        xy, xx, yy = (Gxy ** 2).sum(), (Gxx ** 2).sum(), (Gyy ** 2).sum()
        if name == "rv2":
            nx, ny = (X * X).sum(1), (Y * Y).sum(1)
            xy, xx, yy = xy - (nx * ny).sum(), xx - (nx * nx).sum(), yy - (ny * ny).sum()
        return float(xy / torch.sqrt(xx * yy))
    if name == "autocorrcorr":
        X, Y = X / X.norm(p=2, dim=1, keepdim=True), Y / Y.norm(p=2, dim=1, keepdim=True)
        n = T * (T - 1) / 2
        Sa, Sb = ((X.sum(0) ** 2).sum() - T) / 2, ((Y.sum(0) ** 2).sum() - T) / 2
        Saa, Sbb, Sab = (((X.T @ X) ** 2).sum() - T) / 2, (((Y.T @ Y) ** 2).sum() - T) / 2, (((X.T @ Y) ** 2).sum() - T) / 2
        return float((Sab - Sa * Sb / n) / torch.sqrt((Saa - Sa * Sa / n) * (Sbb - Sb * Sb / n)))
    raise KeyError(name)


METRICS = ("pearson", "concordance", "autocorrcorr", "rv", "rv2", "r1")
RECT_METRICS = ("autocorrcorr", "rv", "rv2")   # take Fx != Fy
CORR_BAR = 4 * 2.0 ** -23                      # the value lies in [-1, 1], the moments are float64: only the float32 output conversion rounds


def corr_inputs(T, Fx, Fy, seed):
    """Feature matrices with a shared component, column standard deviations >= 1e-2 of the column means (asserted)."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(T, max(Fx, Fy), generator=g)
    X = (base[:, :Fx] + 0.5 + 0.3 * torch.randn(T, Fx, generator=g)).float()
    Y = (0.5 * base[:, :Fy].flip(1) + 0.5 * base[:, :Fy] - 1.0 + 0.6 * torch.randn(T, Fy, generator=g)).float()
    for M in (X, Y):
        assert bool((M.double().std(0) >= 1e-2 * M.double().mean(0).abs()).all())
    return X, Y
