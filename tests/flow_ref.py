"""CPU restatements used by the video-pipeline tests only (tests/test_video_pipeline_host.py, tests/test_gpu_video_pipeline.py): the warp
through ``torch.nn.functional.grid_sample``, the consistency map (flow/consistency.py:78-127 with torchvision's 3-tap ``gaussian_blur``
restated), ``interpolate``, the composition formulae of diffusion/video.py:221-277, and Farneback's dense flow from the published
algorithm (G. Farneback, SCIA 2003; the stages DESIGN 5e lists) in float32 or, with ``dtype=torch.float64``, in double."""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------------------------ warp / resize
def flow_warp_map(flow):
    """flow/lib.py:51-63 without the in-place division of the argument."""
    b, h, w, _ = flow.shape
    neutral = torch.stack(torch.meshgrid(torch.linspace(-1, 1, w), torch.linspace(-1, 1, h), indexing="xy"), axis=2).unsqueeze(0).to(flow)
    return neutral + torch.stack([flow[..., 0] / w, flow[..., 1] / h], dim=-1)


def warp(x, grid):
    return F.grid_sample(x, grid, padding_mode="reflection", align_corners=False)


def warp_flow(x, flow, exaggeration=1.0):
    return warp(x, flow_warp_map(flow * exaggeration))


def resize_bilinear(x, size, multiplier=1.0, clamp=None):
    """diffusion/video.py:149-157 on a channels-last tensor [B, H, W, C]: clamp, multiply, ``interpolate(mode="bilinear")``."""
    if clamp is not None:
        x = x.clamp(-clamp, clamp)
    x = x * multiplier
    return F.interpolate(x.permute(0, 3, 1, 2), tuple(size), mode="bilinear").permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------------------------ consistency
def gaussian_blur3(img):
    """torchvision.transforms.functional.gaussian_blur(img, 3) for [..., H, W]: sigma 0.3 ((3 - 1) 0.5 - 1) + 0.8 = 0.8, taps
    exp(-0.5 (x / sigma)^2) at linspace(-1, 1, 3) normalised, outer product, reflect padding, depthwise conv2d."""
    sigma = 0.3 * ((3 - 1) * 0.5 - 1) + 0.8
    x = torch.linspace(-1, 1, 3)
    pdf = torch.exp(-0.5 * (x / sigma).pow(2))
    k1 = (pdf / pdf.sum()).to(img.dtype)
    k2 = torch.mm(k1[:, None], k1[None, :])
    shape = img.shape
    im = img.reshape(-1, 1, shape[-2], shape[-1])
    im = F.pad(im, [1, 1, 1, 1], mode="reflect")
    return F.conv2d(im, k2[None, None]).reshape(shape)


def consistency_terms(flow_forward, flow_backward):
    """The quantities check_consistency compares, for one pair [1, H, W, 2] -> dict of [H, W] tensors (in the flows' dtype)."""
    _, height, width, _ = flow_forward.shape
    dt = flow_forward.dtype
    ff, fb = flow_forward.permute(0, 3, 1, 2), flow_backward.permute(0, 3, 1, 2)
    dx_ker = torch.tensor([[[[0, 0, 0], [1, 0, -1], [0, 0, 0]]]]).to(dt).div(2).repeat(2, 2, 1, 1)
    dy_ker = torch.tensor([[[[0, 1, 0], [0, 0, 0], [0, -1, 0]]]]).to(dt).div(2).repeat(2, 2, 1, 1)
    f_x = F.conv2d(fb, dx_ker, padding="same")
    f_y = F.conv2d(fb, dy_ker, padding="same")
    motionedge = torch.cat([f_x, f_y]).square().sum(dim=(0, 1))
    y, x = torch.meshgrid([torch.arange(0, height), torch.arange(0, width)], indexing="ij")
    p1 = torch.stack([x, y])
    v1 = ff.squeeze(0)
    p0 = p1 + fb.squeeze(0)
    max_pos = torch.tensor([width - 1, height - 1]).view(2, 1, 1)
    grid = p0.div(max_pos / 2).sub(1).movedim(0, -1).unsqueeze(0)
    v0 = F.grid_sample(v1.unsqueeze(0), grid.to(dt), align_corners=True).squeeze(0)
    p1_back = p0 + v0
    v1_back = fb.squeeze(0)
    r1 = torch.floor(p0)
    r2 = r1 + 1
    min_pos = torch.tensor([0, 0]).view(2, 1, 1)
    overshoot = torch.logical_or(r1.lt(min_pos), r2.gt(max_pos))
    overshoot = torch.logical_or(overshoot[0], overshoot[1])
    return dict(missed_lhs=(p1_back - p1).square().sum(dim=0), missed_rhs=torch.stack([v1_back, v0]).square().sum(dim=(0, 1)).mul(0.01).add(0.5),
                edge_lhs=motionedge, edge_rhs=v1_back.square().sum(dim=0).mul(0.01).add(0.002), overshoot=overshoot)


def consistency_classes(flow_forward, flow_backward):
    t = consistency_terms(flow_forward, flow_backward)
    missed = t["missed_lhs"].ge(t["missed_rhs"])
    boundary = t["edge_lhs"].ge(t["edge_rhs"])
    reliable = torch.ones(flow_forward.shape[1:3], dtype=flow_forward.dtype)
    reliable[boundary] = 0
    reliable[missed] = -0.75
    reliable[t["overshoot"]] = 0
    return reliable, dict(boundary=boundary, missed=missed, overshoot=t["overshoot"])


def check_consistency(flow_forward, flow_backward):
    """flow/consistency.py:85-127 -> [1, H, W]."""
    reliable, _ = consistency_classes(flow_forward, flow_backward)
    return gaussian_blur3(reliable.unsqueeze(0)).clip(0, 1)


def near_threshold(flow_forward, flow_backward, eps=1e-5):
    """Pixels whose classification comparisons come within ``eps`` of their thresholds in float64, and their 3 x 3 neighbourhoods (the
    blur spreads a flipped class over them) -> (bool [H, W] of pixels to exclude, fraction of pixels with a close comparison)."""
    t = consistency_terms(flow_forward.double(), flow_backward.double())
    close = (t["missed_lhs"] - t["missed_rhs"]).abs().le(eps) | (t["edge_lhs"] - t["edge_rhs"]).abs().le(eps)
    p0 = None
    _, h, w, _ = flow_forward.shape
    y, x = torch.meshgrid([torch.arange(0, h), torch.arange(0, w)], indexing="ij")
    p0 = torch.stack([x, y]) + flow_backward.double().permute(0, 3, 1, 2).squeeze(0)
    fl = torch.floor(p0)
    lim = torch.tensor([w - 1, h - 1]).view(2, 1, 1)
    edge = ((p0 - fl).abs().le(eps) | (p0 - fl - 1).abs().le(eps)) & ((fl.abs() <= 1) | ((fl - lim).abs() <= 1))
    close = close | edge[0] | edge[1]
    spread = F.max_pool2d(close[None, None].float(), 3, 1, 1)[0, 0] > 0
    return spread, float(close.float().mean())


# ------------------------------------------------------------------------------------------------------------------ composition
def compose(frame, prev, flow, consistency, cached, exaggeration, trust, blend, fade, noise_scale, noise):
    """diffusion/video.py:248-277: frame / prev / cached [1, 3, H, W], flow [1, H, W, 2], consistency [1, 1, H, W] or None."""
    init = frame.clone()
    if blend > 0 and prev is not None:
        if trust > 0 and consistency is not None:
            mask = consistency.clone()
            mask *= trust
            mask += 1 - trust
        else:
            mask = torch.ones_like(init)
        mask = mask * blend
        init = init + mask * warp_flow(prev, flow, exaggeration)
        init = init / (1 + mask)
    if cached is not None:
        init = fade * init + (1 - fade) * cached
    if noise_scale != 0:
        init = init + noise_scale * noise
    return init


def turbo(prev, nxt, flow, exaggeration, warp_next, bt):
    """One skipped frame of diffusion/video.py:224-237 -> (prev', next', img)."""
    if prev is not None:
        prev = warp_flow(prev, flow, exaggeration)
    if warp_next:
        nxt = warp_flow(nxt, flow, exaggeration)
    img = prev * (1.0 - bt) + nxt * bt if prev is not None else nxt
    return prev, nxt, img


# ------------------------------------------------------------------------------------------------------------------ Farneback
PYR_SCALE, LEVELS, WINSIZE, ITERATIONS, POLY_N, POLY_SIGMA, MIN_SIZE = 0.8, 15, 15, 15, 7, 1.5, 32
BORDER = (0.14, 0.14, 0.4472, 0.4472, 0.4472)
V = 2.0 ** -24          # one float32 rounding, relative


def to_gray_u8(im):
    """luminance(im).mul(255).byte() of [3, H, W] in [0, 1] -> float32 [H, W] (the estimator's input; float32 arithmetic, as there)."""
    im = im.float()
    lum = 0.2126 * im[0] + 0.7152 * im[1] + 0.0722 * im[2]
    return lum.mul(255).clamp(0, 255).byte().float()


def pyramid_levels(rows, cols):
    k, scale = 0, 1.0
    while k < LEVELS:
        scale *= PYR_SCALE
        if cols * scale < MIN_SIZE or rows * scale < MIN_SIZE:
            break
        k += 1
    return k


def _round(v):
    return int(np.rint(v))


def blur_taps(sigma):
    ksize = max(_round(sigma * 5) | 1, 3)
    if sigma <= 0:
        return torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)
    x = torch.arange(ksize, dtype=torch.float64) - ksize // 2
    v = torch.exp(-x * x / (2 * sigma * sigma))
    return v / v.sum()


def _conv_axis(img, taps, axis, mode):
    """1-D correlation of [H, W] along ``axis`` with border ``mode`` ("reflect" = reflect-101, "replicate")."""
    r = taps.shape[0] // 2
    pad = [r, r, 0, 0] if axis == 1 else [0, 0, r, r]
    x = F.pad(img[None, None], pad, mode=mode)
    k = taps.to(img.dtype).reshape(1, 1, 1, -1) if axis == 1 else taps.to(img.dtype).reshape(1, 1, -1, 1)
    return F.conv2d(x, k)[0, 0]


def _resize_coords(n_in, n_out):
    f = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).float()
    i0 = torch.floor(f)
    t = f - i0
    i0 = i0.long()
    low, high = i0 < 0, i0 >= n_in - 1
    t = torch.where(low | high, torch.zeros_like(t), t)
    i0 = torch.where(low, torch.zeros_like(i0), torch.where(high, torch.full_like(i0, n_in - 1), i0))
    return i0, (i0 + 1).clamp(max=n_in - 1), t


def fb_resize(x, h, w):
    """Bilinear resize of [..., H, W] with pixel-centre mapping and a replicated edge; columns first, then rows."""
    x0, x1, tx = _resize_coords(x.shape[-1], w)
    y0, y1, ty = _resize_coords(x.shape[-2], h)
    tx, ty = tx.to(x.dtype), ty.to(x.dtype)[:, None]
    rows = x[..., x0] * (1 - tx) + x[..., x1] * tx
    return rows[..., y0, :] * (1 - ty) + rows[..., y1, :] * ty


def poly_setup():
    """-> (g, xg, xxg [8] float32 taps as float64 tensors, (ig11, ig03, ig33, ig55) rounded to float32)."""
    n = POLY_N
    x = torch.arange(-n, n + 1, dtype=torch.float64)
    g = torch.exp(-x * x / (2 * POLY_SIGMA * POLY_SIGMA))
    g = (g / g.sum()).float().double()
    G = torch.zeros(6, 6, dtype=torch.float64)
    wgt = g[:, None] * g[None, :]            # [y, x]
    xx, yy = (x * x)[None, :], (x * x)[:, None]
    G[0, 0] = wgt.sum()
    G[1, 1] = (wgt * xx).sum()
    G[3, 3] = (wgt * xx * xx).sum()
    G[5, 5] = (wgt * xx * yy).sum()
    G[2, 2] = G[0, 3] = G[0, 4] = G[3, 0] = G[4, 0] = G[1, 1]
    G[4, 4] = G[3, 3]
    G[3, 4] = G[4, 3] = G[5, 5]
    inv = torch.linalg.inv(G)
    f32 = lambda v: float(torch.tensor(float(v)).float())
    k = torch.arange(0, n + 1, dtype=torch.float64)
    gh = g[n:]
    return gh, (k * gh).float().double(), (k * k * gh).float().double(), tuple(f32(inv[i, j]) for i, j in ((1, 1), (0, 3), (3, 3), (5, 5)))


def poly_exp(img):
    """[H, W] -> [5, H, W]: coefficients of x, y, x^2, y^2, xy (replicated borders)."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_setup()
    sym = lambda t: torch.cat([t[1:].flip(0), t])
    anti = lambda t: torch.cat([-t[1:].flip(0), t])
    t0 = _conv_axis(img, sym(g), 0, "replicate")
    t1 = _conv_axis(img, anti(xg), 0, "replicate")
    t2 = _conv_axis(img, sym(xxg), 0, "replicate")
    b1 = _conv_axis(t0, sym(g), 1, "replicate")
    b2 = _conv_axis(t0, anti(xg), 1, "replicate")
    b4 = _conv_axis(t0, sym(xxg), 1, "replicate")
    b3 = _conv_axis(t1, sym(g), 1, "replicate")
    b6 = _conv_axis(t1, anti(xg), 1, "replicate")
    b5 = _conv_axis(t2, sym(g), 1, "replicate")
    return torch.stack([b2 * ig11, b3 * ig11, b1 * ig03 + b4 * ig33, b1 * ig03 + b5 * ig33, b6 * ig55])


def _border_scale(h, w, dt):
    def side(n):
        v = torch.ones(n, dtype=dt)
        b = torch.tensor(BORDER, dtype=torch.float32).to(dt)
        for i in range(min(5, n)):
            v[i] = v[i] * b[i]
            v[n - 1 - i] = v[n - 1 - i] * b[i]
        return v
    return side(h)[:, None] * side(w)[None, :]


def update_matrices(R0, R1, flow, with_bound=False):
    """R0 / R1 [5, H, W], flow [H, W, 2] -> M [5, H, W].  The sampling positions x + dx, their floors and fractions are taken in the
    flow's dtype (a float32 flow with float64 coefficients: the device's own positions, exact float32 operations, so the branch taken
    is the device's at every pixel) and the rest in the coefficients'.  ``with_bound``: -> (M, bound [5, H, W], inside [H, W]), the
    float32 rounding bound of the kernel's expression tree, element-wise, from the absolute values of the intermediate terms
    (V = 2^-24 per rounding, contracted or not):
        weights a = (1 - tx)(1 - ty) ...: two subtractions and a product, 3 V;  s = sum of 4 products: 4 V more -> Es = 7 V sum a |p|
        r4 = (R0 + s) / 2: Es / 2 + V |R0 + s| / 2 (r5 alike, r6 with 1 / 4; r2' = (R0 - s) / 2);  outside the frame: exact
        r2 = r2' + r4 dx + r6 dy: E2' + |dx| E4 + |dy| E6 + 3 V (|r2'| + |r4 dx| + |r6 dy|)
        border scale (up to three products of table entries, one more on r): sc E + 4 V |r sc|, where sc != 1
        m0 = r4^2 + r6^2: 2 |r4| E4 + 2 |r6| E6 + 2 V (r4^2 + r6^2);  m1 = (r4 + r5) r6: (E4 + E5) |r6| + |r4 + r5| E6 + 2 V |m1|
        m3 = r4 r2 + r6 r3: |r4| E2 + |r2| E4 + |r6| E3 + |r3| E6 + 2 V (|r4 r2| + |r6 r3|)   (m2 like m0, m4 like m3)"""
    _, h, w = R0.shape
    dt, pt = R0.dtype, flow.dtype
    y, x = torch.meshgrid([torch.arange(h), torch.arange(w)], indexing="ij")
    fx, fy = x.to(pt) + flow[..., 0], y.to(pt) + flow[..., 1]
    flx, fly = torch.floor(fx), torch.floor(fy)
    inside = (flx >= 0) & (flx < w - 1) & (fly >= 0) & (fly < h - 1)
    x1, y1 = flx.clamp(0, w - 2).long(), fly.clamp(0, h - 2).long()
    tx, ty = (fx - flx).to(dt), (fy - fly).to(dt)
    dx, dy = flow[..., 0].to(dt), flow[..., 1].to(dt)
    a00, a01, a10, a11 = (1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty
    p00, p01, p10, p11 = R1[:, y1, x1], R1[:, y1, x1 + 1], R1[:, y1 + 1, x1], R1[:, y1 + 1, x1 + 1]
    s = a00 * p00 + a01 * p01 + a10 * p10 + a11 * p11
    zero = torch.zeros_like(dx)
    r2 = torch.where(inside, s[0], zero)
    r3 = torch.where(inside, s[1], zero)
    r4 = torch.where(inside, (R0[2] + s[2]) * 0.5, R0[2])
    r5 = torch.where(inside, (R0[3] + s[3]) * 0.5, R0[3])
    r6 = torch.where(inside, (R0[4] + s[4]) * 0.25, R0[4] * 0.5)
    r2p = (R0[0] - r2) * 0.5
    r3p = (R0[1] - r3) * 0.5
    r2 = r2p + r4 * dx + r6 * dy
    r3 = r3p + r6 * dx + r5 * dy
    sc = _border_scale(h, w, dt)
    if with_bound:
        Es = 7 * V * (a00 * p00.abs() + a01 * p01.abs() + a10 * p10.abs() + a11 * p11.abs())
        E2p = torch.where(inside, 0.5 * (Es[0] + V * (R0[0] - s[0]).abs()), zero)
        E3p = torch.where(inside, 0.5 * (Es[1] + V * (R0[1] - s[1]).abs()), zero)
        E4 = torch.where(inside, 0.5 * (Es[2] + V * (R0[2] + s[2]).abs()), zero)
        E5 = torch.where(inside, 0.5 * (Es[3] + V * (R0[3] + s[3]).abs()), zero)
        E6 = torch.where(inside, 0.25 * (Es[4] + V * (R0[4] + s[4]).abs()), zero)
        E2 = E2p + dx.abs() * E4 + dy.abs() * E6 + 3 * V * (r2p.abs() + (r4 * dx).abs() + (r6 * dy).abs())
        E3 = E3p + dx.abs() * E6 + dy.abs() * E5 + 3 * V * (r3p.abs() + (r6 * dx).abs() + (r5 * dy).abs())
        scaled = lambda r, E: sc * E + torch.where(sc != 1, 4 * V * (r * sc).abs(), zero)
        E2, E3, E4, E5, E6 = scaled(r2, E2), scaled(r3, E3), scaled(r4, E4), scaled(r5, E5), scaled(r6, E6)
    r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
    M = torch.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3])
    if not with_bound:
        return M
    a = torch.abs
    bound = torch.stack([2 * a(r4) * E4 + 2 * a(r6) * E6 + 2 * V * (r4 * r4 + r6 * r6),
                         (E4 + E5) * a(r6) + a(r4 + r5) * E6 + 2 * V * a(M[1]),
                         2 * a(r5) * E5 + 2 * a(r6) * E6 + 2 * V * (r5 * r5 + r6 * r6),
                         a(r4) * E2 + a(r2) * E4 + a(r6) * E3 + a(r3) * E6 + 2 * V * (a(r4 * r2) + a(r6 * r3)),
                         a(r6) * E2 + a(r2) * E6 + a(r5) * E3 + a(r3) * E5 + 2 * V * (a(r6 * r2) + a(r5 * r3))])
    return M, bound, inside


def _box_mean(M):
    r = WINSIZE // 2
    ones = torch.ones(WINSIZE, dtype=M.dtype)
    x = F.pad(M[:, None], [r, r, r, r], mode="replicate")
    x = F.conv2d(x, ones.reshape(1, 1, 1, -1))
    x = F.conv2d(x, ones.reshape(1, 1, -1, 1))[:, 0]
    return x * torch.tensor(1.0 / (WINSIZE * WINSIZE), dtype=torch.float32).to(M.dtype)


def blur_solve(M, E_M=None, with_bound=False):
    """15 x 15 box mean of M (replicated border) and the 2 x 2 solve -> flow [H, W, 2].  ``with_bound``: -> (flow, bound [H, W, 2],
    valid [H, W]) with the float32 rounding bound of the kernel, element-wise (V = 2^-24; E_M: a bound on M's own error, or None):
        box mean: 225 terms through 30 additions and one product, e_c = mean(E_M) + 31 V mean(|M_c| + E_M)
        det = g0 g2 - g1^2 + 1e-3: E_det = |g2| e0 + |g0| e2 + 2 |g1| e1 + 3 V (|g0 g2| + g1^2 + 1e-3)
        num_x = g2 g3 - g1 g4: E_num = |g3| e2 + |g2| e3 + |g4| e1 + |g1| e4 + 2 V (|g2 g3| + |g1 g4|)    (num_y alike)
        f = num (1 / det): E = (E_num + |f| E_det) / det + 3 V |f|;  valid where E_det < det / 2 (det >= 1e-3 by Cauchy-Schwarz)"""
    g = _box_mean(M)
    g11, g12, g22, h1, h2 = g
    eps = torch.tensor(1e-3, dtype=torch.float32).to(M.dtype)
    det = g11 * g22 - g12 * g12 + eps
    idet = 1.0 / det
    flow = torch.stack([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet], dim=-1)
    if not with_bound:
        return flow
    E_M = torch.zeros_like(M) if E_M is None else E_M
    e = _box_mean(E_M) + 31 * V * _box_mean(M.abs() + E_M)
    a = torch.abs
    E_det = a(g22) * e[0] + a(g11) * e[2] + 2 * a(g12) * e[1] + 3 * V * (a(g11 * g22) + g12 * g12 + eps)
    E_nx = a(h1) * e[2] + a(g22) * e[3] + a(h2) * e[1] + a(g12) * e[4] + 2 * V * (a(g22 * h1) + a(g12 * h2))
    E_ny = a(h2) * e[0] + a(g11) * e[4] + a(h1) * e[1] + a(g12) * e[3] + 2 * V * (a(g11 * h2) + a(g12 * h1))
    E_num = torch.stack([E_nx, E_ny], dim=-1)
    bound = (E_num + a(flow) * E_det[..., None]) / det[..., None] + 3 * V * a(flow)
    return flow, bound, E_det < det / 2


def farneback_gray(prev_u8, next_u8, dtype=torch.float32):
    """Dense flow between two [H, W] images holding 8-bit values -> [H, W, 2] in (x, y) order: prev(p) ~ next(p + flow(p))."""
    imgs = [prev_u8.to(dtype), next_u8.to(dtype)]
    rows, cols = imgs[0].shape
    levels = pyramid_levels(rows, cols)
    flow = None
    for k in range(levels, -1, -1):
        scale = 1.0
        for _ in range(k):
            scale *= PYR_SCALE
        sigma = (1.0 / scale - 1) * 0.5
        taps = blur_taps(sigma).float().double()
        w, h = _round(cols * scale), _round(rows * scale)
        if flow is None:
            flow = torch.zeros(h, w, 2, dtype=dtype)
        else:
            flow = fb_resize(flow.permute(2, 0, 1), h, w).permute(1, 2, 0) * torch.tensor(1.0 / PYR_SCALE).float().to(dtype)
        R = []
        for im in imgs:
            b = _conv_axis(_conv_axis(im, taps, 1, "reflect"), taps, 0, "reflect")
            R.append(poly_exp(fb_resize(b, h, w)))
        M = update_matrices(R[0], R[1], flow)
        for i in range(ITERATIONS):
            flow = blur_solve(M)
            if i < ITERATIONS - 1:
                M = update_matrices(R[0], R[1], flow)
    return flow


def farneback(im1, im2, dtype=torch.float32):
    """flow/__init__.py:38-55 for images [3, H, W] in [0, 1] -> [H, W, 2]."""
    return farneback_gray(to_gray_u8(im1), to_gray_u8(im2), dtype)


# ------------------------------------------------------------------------------------------------------------------ stage by stage
# What tests/test_gpu_farneback.py holds each kernel to and tests/test_farneback_host.py proves of the float32 restatement: the float64
# result of one stage on the input that stage was given, and the float32 rounding bound of the kernel's own sequence of operations
# (V = 2^-24 per rounding; a float32 sum of n products, in any order and contracted or not, lies within n V sum|terms| of exact).
def level_size(rows, cols, k):
    """(h, w) of pyramid level k, as farneback_gray computes it."""
    scale = 1.0
    for _ in range(k):
        scale *= PYR_SCALE
    return _round(rows * scale), _round(cols * scale)


def level_taps(k):
    """The pyramid blur's taps of level k, rounded to float32, as a float64 tensor."""
    scale = 1.0
    for _ in range(k):
        scale *= PYR_SCALE
    return blur_taps((1.0 / scale - 1) * 0.5).float().double()


def pyr_blur(gray, taps, with_bound=False):
    """[H, W] -> the rows' pass then the columns' pass, reflect-101.  Bound: the first pass leaves n V sum|terms|, the second carries that
    through its taps and adds n V sum|terms| of its own input (the exact first pass and its error)."""
    first = _conv_axis(gray, taps, 1, "reflect")
    out = _conv_axis(first, taps, 0, "reflect")
    if not with_bound:
        return out
    n = taps.shape[0]
    e1 = n * V * _conv_axis(gray.abs(), taps, 1, "reflect")
    return out, _conv_axis(e1, taps, 0, "reflect") + n * V * _conv_axis(first.abs() + e1, taps, 0, "reflect")


def fb_resize_bound(x, h, w, mul=None):
    """-> (fb_resize(x, h, w) [* mul], bound): each way is two products and a sum of a weight 1 - t that is itself rounded, 3 V
    sum|terms|; the second way carries the first's error through its weights; the multiplier, when there is one, one rounding more."""
    x0, x1, tx = _resize_coords(x.shape[-1], w)
    y0, y1, ty = _resize_coords(x.shape[-2], h)
    tx, ty = tx.to(x.dtype), ty.to(x.dtype)[:, None]
    rows = x[..., x0] * (1 - tx) + x[..., x1] * tx
    e_rows = 3 * V * (x[..., x0].abs() * (1 - tx) + x[..., x1].abs() * tx)
    out = rows[..., y0, :] * (1 - ty) + rows[..., y1, :] * ty
    e = e_rows[..., y0, :] * (1 - ty) + e_rows[..., y1, :] * ty
    e = e + 3 * V * ((rows.abs() + e_rows)[..., y0, :] * (1 - ty) + (rows.abs() + e_rows)[..., y1, :] * ty)
    if mul is not None:
        out = out * mul
        e = e * abs(mul) + V * out.abs()
    return out, e


def poly_exp_bound(img):
    """-> (poly_exp(img), bound [5, H, W]).  Each pass is a sum of 8 terms tap * (left +- right): the pair's sum, the product and up to 7
    accumulations, 9 V sum |tap| (|left| + |right|); the horizontal pass carries the vertical one's error through its taps and adds its
    own on that pass's input; the final combinations: a product (V), or two products and their sum (2 V sum|terms|)."""
    g, xg, xxg, (ig11, ig03, ig33, ig55) = poly_setup()
    sym = lambda t: torch.cat([t[1:].flip(0), t])
    anti = lambda t: torch.cat([-t[1:].flip(0), t])
    cv = lambda x, t, ax: _conv_axis(x, t, ax, "replicate")
    a = torch.abs
    T, ET = [], []
    for taps in (sym(g), anti(xg), sym(xxg)):
        T.append(cv(img, taps, 0))
        ET.append(9 * V * cv(a(img), a(taps), 0))

    def second(i, taps):
        return cv(T[i], taps, 1), cv(ET[i], a(taps), 1) + 9 * V * cv(a(T[i]) + ET[i], a(taps), 1)
    (b1, e1), (b2, e2), (b4, e4) = second(0, sym(g)), second(0, anti(xg)), second(0, sym(xxg))
    (b3, e3), (b6, e6) = second(1, sym(g)), second(1, anti(xg))
    b5, e5 = second(2, sym(g))
    out = torch.stack([b2 * ig11, b3 * ig11, b1 * ig03 + b4 * ig33, b1 * ig03 + b5 * ig33, b6 * ig55])
    two = lambda p, ep, q, eq: abs(ig03) * ep + abs(ig33) * eq + 2 * V * (a(p * ig03) + a(q * ig33))
    bound = torch.stack([abs(ig11) * e2 + V * a(out[0]), abs(ig11) * e3 + V * a(out[1]), two(b1, e1, b4, e4), two(b1, e1, b5, e5),
                         abs(ig55) * e6 + V * a(out[4])])
    return out, bound


def worst_ratio(got, ref, bound, valid=None):
    """max |got - ref| / bound over the valid elements (an error where the bound is zero: inf)."""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(err).all()), "a value that is not finite"
    r = torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err))
    if valid is not None:
        r = r[valid]
    return float(r.max()) if r.numel() else 0.0


def restate_level(a, b, k, init=None, iterations=1):
    """One pyramid level of the estimator in float32, stage by stage, for images a / b [3, H, W] -> the dict of tensors the device's
    dumps give (maua_farneback_desc): gray, blur [2, H, W], level [2, h, w], coef [2, 5, h, w], flow_in [2, h, w, 2] (init or zero),
    mat [2, 5, h, w], and flow [2, h, w, 2] after ``iterations``."""
    gray = torch.stack([to_gray_u8(a), to_gray_u8(b)])
    h, w = level_size(gray.shape[1], gray.shape[2], k)
    blur = torch.stack([pyr_blur(g, level_taps(k)) for g in gray])
    level = fb_resize(blur, h, w)
    coef = torch.stack([poly_exp(im) for im in level])
    flow_in = torch.zeros(2, h, w, 2) if init is None else init.clone()
    mat = torch.stack([update_matrices(coef[d], coef[1 - d], flow_in[d]) for d in range(2)])
    flow, M = None, mat
    for i in range(iterations):
        flow = torch.stack([blur_solve(M[d]) for d in range(2)])
        if i < iterations - 1:
            M = torch.stack([update_matrices(coef[d], coef[1 - d], flow[d]) for d in range(2)])
    return dict(gray=gray, blur=blur, level=level, coef=coef, flow_in=flow_in, mat=mat, flow=flow)


# Each check takes such a dict - the device's or the float32 restatement's - and judges one stage on the input that stage was given:
# the float64 result of the dict's own previous stage, inside the bound -> the worst error / bound.
def check_blur(d, k):
    return max(worst_ratio(d["blur"][i], *pyr_blur(d["gray"][i].double(), level_taps(k), True)) for i in range(2))


def check_resize(d):
    h, w = d["level"].shape[1:]
    return worst_ratio(d["level"], *fb_resize_bound(d["blur"].double(), h, w))


def check_poly(d):
    return max(worst_ratio(d["coef"][i], *poly_exp_bound(d["level"][i].double())) for i in range(2))


def check_matrices(d):
    """-> (worst ratio over every pixel of both directions, the in-frame masks [2, h, w])"""
    R = d["coef"].double()
    res = [update_matrices(R[i], R[1 - i], d["flow_in"][i], True) for i in range(2)]
    return max(worst_ratio(d["mat"][i], res[i][0], res[i][1]) for i in range(2)), torch.stack([r[2] for r in res])


def check_iteration(d):
    """The flow after one iteration against the box mean and solve of the dict's matrices -> (worst ratio, share of pixels left out)"""
    res = [blur_solve(d["mat"][i].double(), None, True) for i in range(2)]
    out = 1 - float(torch.stack([r[2] for r in res]).float().mean())
    return max(worst_ratio(d["flow"][i], res[i][0], res[i][1], res[i][2]) for i in range(2)), out


def check_second_iteration(d1, d2):
    """d1: the run with one iteration, d2: the same run with two.  The matrices of d1's flow and their bound, carried through the box
    mean and the solve -> (worst ratio, share of pixels left out)"""
    R = d2["coef"].double()
    worst, valid = 0.0, []
    for i in range(2):
        M, EM, _ = update_matrices(R[i], R[1 - i], d1["flow"][i], True)
        f, bound, ok = blur_solve(M, EM, True)
        worst = max(worst, worst_ratio(d2["flow"][i], f, bound, ok))
        valid.append(ok)
    return worst, 1 - float(torch.stack(valid).float().mean())


def check_upsample(flow_k, flow_in, h, w):
    """flow_k [2, hk, wk, 2] of level k, flow_in [2, h, w, 2] entering level k - 1"""
    ref, bound = fb_resize_bound(flow_k.double().permute(0, 3, 1, 2), h, w, float(torch.tensor(1.0 / PYR_SCALE).float()))
    return worst_ratio(flow_in.permute(0, 3, 1, 2), ref, bound)


# ------------------------------------------------------------------------------------------------------------------ the tests' inputs
def textured_pair(h, w, shift=(1.5, -0.75), seed=0, sigma=1.6):
    """A blurred noise field and the same field displaced by ``shift`` pixels (bilinear samples of the one field, so first(p) ~
    second(p + shift)) -> (first, second) [3, h, w] in [0, 1]: texture at every scale the window sees, unlike sinusoid_pair."""
    m = 8
    g = torch.Generator().manual_seed(seed)
    field = torch.rand(3, h + 2 * m, w + 2 * m, generator=g, dtype=torch.float64)
    r = int(3 * sigma)
    k = torch.exp(-(torch.arange(-r, r + 1, dtype=torch.float64) ** 2) / (2 * sigma * sigma))
    k = k / k.sum()
    for ax in (1, 0):
        field = torch.stack([_conv_axis(c, k, ax, "reflect") for c in field])
    field = (field - field.min()) / (field.max() - field.min())

    def crop(dx, dy):
        x0, y0 = math.floor(dx), math.floor(dy)
        tx, ty = dx - x0, dy - y0
        c = lambda yy, xx: field[:, m + yy:m + yy + h, m + xx:m + xx + w]
        return (c(y0, x0) * (1 - tx) + c(y0, x0 + 1) * tx) * (1 - ty) + (c(y0 + 1, x0) * (1 - tx) + c(y0 + 1, x0 + 1) * tx) * ty
    return crop(0.0, 0.0).float(), crop(-shift[0], -shift[1]).float()


def gray_images(h, w, seed=3):
    """Two images [3, h, w] in [-0.2, 1.2] (both clamps of the luminance are reached) with planted grey pixels (r = g = b) in the first
    rows of the first image whose float32 luminance times 255 is: an integer exactly, that integer less one ulp, 0, and 255 exactly,
    and one whose value depends on the products and sums not being contracted
    -> (a, b, planted) with planted a list of (x, kind, the 8-bit value expected)."""
    g = torch.Generator().manual_seed(seed)
    a, b = (torch.rand(3, h, w, generator=g) * 1.4 - 0.2 for _ in range(2))
    lum255 = lambda v: np.float32(np.float32(np.float32(np.float32(0.2126) * v + np.float32(0.7152) * v) + np.float32(0.0722) * v) * np.float32(255))
    planted, col = [], 0
    for target, kinds in ((100, ("integer", "below")), (37, ("integer", "below")), (255, ("integer",))):
        want = {"integer": np.float32(target), "below": np.nextafter(np.float32(target), np.float32(0))}
        v = np.float32(target / 255)
        for _ in range(16):
            v = np.nextafter(v, np.float32(0))
        found = {}
        for _ in range(64):
            for kind in kinds:
                if lum255(v) == want[kind]:
                    found.setdefault(kind, v)
            v = np.nextafter(v, np.float32(2))
        for kind in kinds:
            a[:, 0, col] = float(found[kind])            # KeyError: no float32 grey level gives this value (none seen)
            planted.append((col, kind, target if kind == "integer" else target - 1))
            col += 1
    a[:, 0, col] = 0.0
    planted.append((col, "zero", 0))
    # a pixel of sinusoid_pair(130, 33): 106 with every product and sum rounded on its own, 105 as soon as 0.7152 g + 0.2126 r is one
    # fused multiply-add (the luminance lands one ulp lower, below the integer)
    a[:, 0, col + 1] = torch.tensor(CONTRACTION_PIXEL)
    planted.append((col + 1, "contraction", 106))
    return a, b, planted


CONTRACTION_PIXEL = (float.fromhex("0x1.014ec4p-1"), float.fromhex("0x1.8af25ap-2"), float.fromhex("0x1.d40032p-2"))


def gray_contracted(rgb):
    """The 8-bit luminance of one pixel with 0.2126 r + 0.7152 g evaluated as a fused multiply-add (one rounding): what a compiler that
    contracts the expression computes.  The product is exact in float64 and the sum's double rounding cannot matter at 29 spare bits."""
    f = np.float32
    r, g, b = (float(f(v)) for v in rgb)
    first = float(f(float(f(0.7152)) * g + float(f(float(f(0.2126)) * r))))
    lum = f(f(first) + f(f(0.0722) * f(b)))
    return int(np.clip(f(lum * f(255)), 0, 255))


def matrices_flows(h, w, seed=5, reach=0.35):
    """Constructed flows entering a level, [2, h, w, 2] float32 (direction a -> b, b -> a): uniform in +- reach (w, h), so that about a
    tenth of the pixels sample beyond each side of the frame; a few of +- 10 w; and planted pixels at the edges of the in-frame
    predicate (positions exact in float32): x + dx = w - 1 exactly and one ulp below it, 0 exactly, and two tiny negatives (-1e-30 in
    column 0; x = 5 with dx = -5 less one ulp), the same along y -> (flows, planted) with planted a list of (direction, y, x, inside)."""
    g = torch.Generator().manual_seed(seed)
    f = (torch.rand(2, h, w, 2, generator=g) - 0.5) * 2 * reach * torch.tensor([w, h], dtype=torch.float32)
    big = torch.randint(0, h * w, (2, 6), generator=g)
    for d in range(2):
        for j, i in enumerate(big[d].tolist()):
            f[d, i // w, i % w] = torch.tensor([10.0 * w, -10.0 * w] if j % 2 else [-10.0 * w, 10.0 * w])[: 2] * (1 if j < 3 else -1)
    below = lambda v: float(np.nextafter(np.float32(v), np.float32(-1e30)))
    planted = []
    for d in range(2):
        # one row each, its y position inside (dy = 0.25); then one column each, its x position inside (dx = 0.5)
        for j, (x, dx, inside) in enumerate(((2, float(w - 1 - 2), False), (0, below(w - 1), True), (3, -3.0, True), (0, -1e-30, False),
                                             (5, below(-5.0), False), (7, float(w - 2 - 7), True))):
            y = 1 + 2 * j + d
            f[d, y, x] = torch.tensor([dx, 0.25])
            planted.append((d, y, x, inside))
        for j, (y, dy, inside) in enumerate(((2, float(h - 1 - 2), False), (0, below(h - 1), True), (3, -3.0, True), (0, -1e-30, False),
                                             (5, below(-5.0), False), (8, float(h - 2 - 8), True))):
            x = 2 + 2 * j + d
            f[d, y, x] = torch.tensor([0.5, dy])
            planted.append((d, y, x, inside))
    assert len({p[:3] for p in planted}) == len(planted)
    return f, planted


def sinusoid_pair(h=80, w=96, shift=(1.5, -0.75), n_waves=20, seed=38):
    """A fixed sum of low-frequency sinusoids on an h x w grid and the same field displaced by ``shift`` pixels, both evaluated
    analytically (no interpolation): first(p) = second(p + shift), so the flow first -> second is ``shift`` everywhere.
    -> (first, second) [3, h, w] in [0, 1]."""
    rng = np.random.default_rng(seed)
    fx = rng.uniform(-0.12, 0.12, (3, n_waves)) * 2 * math.pi
    fy = rng.uniform(-0.12, 0.12, (3, n_waves)) * 2 * math.pi
    ph = rng.uniform(0, 2 * math.pi, (3, n_waves))
    amp = rng.uniform(0.5, 1.0, (3, n_waves))
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")

    def field(dx, dy):
        v = np.zeros((3, h, w))
        for c in range(3):
            for k in range(n_waves):
                v[c] += amp[c, k] * np.sin(fx[c, k] * (x - dx) + fy[c, k] * (y - dy) + ph[c, k])
        return v
    a, b = field(0.0, 0.0), field(shift[0], shift[1])
    lo, hi = min(a.min(), b.min()), max(a.max(), b.max())
    norm = lambda v: torch.from_numpy((v - lo) / (hi - lo)).float()
    return norm(a), norm(b)


def endpoint_error(flow, shift, border=16):
    d = flow[border:-border, border:-border].double() - torch.tensor(shift, dtype=torch.float64)
    return float(d.square().sum(-1).sqrt().mean())


def pipe_inputs(n_frames=5, size=64):
    """The stub frame / flow / consistency sources and the first-frame image of the processor-order fixture (seeded draws shared by
    tests/golden/make_golden_video.py and the tests) -> (frames [n, 1, 3, S, S], flows [n, 1, S, S, 2], consistency [n, 1, 1, S, S], first)."""
    fg = torch.Generator().manual_seed(3802)
    frames = torch.rand(n_frames, 1, 3, size, size, generator=fg) * 2 - 1
    flows = (torch.rand(n_frames, 1, size, size, 2, generator=fg) - 0.5) * 6
    cons = torch.rand(n_frames, 1, 1, size, size, generator=fg)
    first = torch.rand(1, 3, size, size, generator=fg) * 2 - 1
    return frames, flows, cons, first
