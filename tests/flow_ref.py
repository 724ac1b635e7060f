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


def update_matrices(R0, R1, flow):
    """R0 / R1 [5, H, W], flow [H, W, 2] -> M [5, H, W]."""
    _, h, w = R0.shape
    dt = R0.dtype
    y, x = torch.meshgrid([torch.arange(h), torch.arange(w)], indexing="ij")
    dx, dy = flow[..., 0], flow[..., 1]
    fx, fy = x.to(dt) + dx, y.to(dt) + dy
    flx, fly = torch.floor(fx), torch.floor(fy)
    inside = (flx >= 0) & (flx < w - 1) & (fly >= 0) & (fly < h - 1)
    x1, y1 = flx.clamp(0, w - 2).long(), fly.clamp(0, h - 2).long()
    tx, ty = fx - flx, fy - fly
    a00, a01, a10, a11 = (1 - tx) * (1 - ty), tx * (1 - ty), (1 - tx) * ty, tx * ty
    s = a00 * R1[:, y1, x1] + a01 * R1[:, y1, x1 + 1] + a10 * R1[:, y1 + 1, x1] + a11 * R1[:, y1 + 1, x1 + 1]
    zero = torch.zeros_like(dx)
    r2 = torch.where(inside, s[0], zero)
    r3 = torch.where(inside, s[1], zero)
    r4 = torch.where(inside, (R0[2] + s[2]) * 0.5, R0[2])
    r5 = torch.where(inside, (R0[3] + s[3]) * 0.5, R0[3])
    r6 = torch.where(inside, (R0[4] + s[4]) * 0.25, R0[4] * 0.5)
    r2 = (R0[0] - r2) * 0.5
    r3 = (R0[1] - r3) * 0.5
    r2 = r2 + r4 * dx + r6 * dy
    r3 = r3 + r6 * dx + r5 * dy

    def side(n):
        v = torch.ones(n, dtype=dt)
        b = torch.tensor(BORDER, dtype=torch.float32).to(dt)
        for i in range(min(5, n)):
            v[i] = v[i] * b[i]
            v[n - 1 - i] = v[n - 1 - i] * b[i]
        return v
    sc = side(h)[:, None] * side(w)[None, :]
    r2, r3, r4, r5, r6 = r2 * sc, r3 * sc, r4 * sc, r5 * sc, r6 * sc
    return torch.stack([r4 * r4 + r6 * r6, (r4 + r5) * r6, r5 * r5 + r6 * r6, r4 * r2 + r6 * r3, r6 * r2 + r5 * r3])


def blur_solve(M):
    """15 x 15 box mean of M (replicated border) and the 2 x 2 solve -> flow [H, W, 2]."""
    r = WINSIZE // 2
    ones = torch.ones(WINSIZE, dtype=M.dtype)
    x = F.pad(M[:, None], [r, r, r, r], mode="replicate")
    x = F.conv2d(x, ones.reshape(1, 1, 1, -1))
    x = F.conv2d(x, ones.reshape(1, 1, -1, 1))[:, 0]
    g11, g12, g22, h1, h2 = x * torch.tensor(1.0 / (WINSIZE * WINSIZE), dtype=torch.float32).to(M.dtype)
    idet = 1.0 / (g11 * g22 - g12 * g12 + torch.tensor(1e-3, dtype=torch.float32).to(M.dtype))
    return torch.stack([(g22 * h1 - g12 * h2) * idet, (g11 * h2 - g12 * h1) * idet], dim=-1)


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
