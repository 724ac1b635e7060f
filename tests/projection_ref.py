"""What the projection kernels (csrc/project.hip, maua_synth_vjp_ex) and maua_amd/projection.py are held against.

Three kinds of statement, kept apart:
  *_f32       numpy float32 restatements in the kernels' own operation and reduction order: the device must give THESE BITS
  *_f64       the formulae themselves in float64 (torch, with autograd where a gradient is asked for): what is true
  *_bound     first-order rounding bounds between the two, from operation counts: V = 2^-24 per rounding of a float32 result,
              U = 2^-149 (the smallest denormal) where a result may underflow.  tests/test_projection_host.py proves each bound for the
              float32 restatement on the very inputs the device tests use; the device tests then hold the device to the same bound,
              with no further margin.
"""
from math import ceil, sqrt

import numpy as np
import torch
import torch.nn.functional as F

import synth_vjp_ref as R
from oracle import stylegan2 as OS

V = 2.0 ** -24
U = 2.0 ** -149
f32 = np.float32
RED_CHUNK = 4096


# ---------------------------------------------------------------------------------------------------------------- reductions
def red_sum_f32(x):
    """sum over the last axis in project.hip's order: chunks of 4096; in a chunk thread t of 256 adds elements t, t + 256, ... from 0,
    the 256 sums fold a[t] += a[t + s], s = 128 .. 1; the chunks are added in chunk order"""
    x = np.asarray(x, dtype=f32)
    N = x.shape[-1]
    nchunk = max(1, ceil(N / RED_CHUNK))
    pad = np.zeros(x.shape[:-1] + (nchunk * RED_CHUNK,), dtype=f32)
    pad[..., :N] = x
    pad = pad.reshape(x.shape[:-1] + (nchunk, RED_CHUNK // 256, 256))
    acc = np.zeros(x.shape[:-1] + (nchunk, 256), dtype=f32)
    for i in range(RED_CHUNK // 256):
        acc = acc + pad[..., i, :]
    s = 128
    while s >= 1:
        acc[..., :s] = acc[..., :s] + acc[..., s:2 * s]
        s //= 2
    t = acc[..., 0, 0].copy()
    for k in range(1, nchunk):
        t = t + acc[..., k, 0]
    return t


def red_depth(N):
    """roundings a single term passes on its way through red_sum_f32 (at most): trips + tree + chunks"""
    nchunk = max(1, ceil(N / RED_CHUNK))
    return min(RED_CHUNK // 256, ceil(N / 256)) + 8 + (nchunk - 1)


# ---------------------------------------------------------------------------------------------------------------- regulariser
def reg_levels(R_):
    k = 1
    while R_ > 8:
        R_, k = R_ // 2, k + 1
    return k


def noise_reg_f64(n, weight=1.0):
    """(loss [B], weight d sum(loss) / d n) of maps n [B, R, R]: the published regulariser written with torch.roll and avg_pool2d"""
    n = n.double().clone().requires_grad_(True)
    a, loss = n[:, None], 0
    while True:
        loss = loss + (a * torch.roll(a, 1, 3)).mean((1, 2, 3)) ** 2 + (a * torch.roll(a, 1, 2)).mean((1, 2, 3)) ** 2
        if a.shape[-1] <= 8:
            break
        a = F.avg_pool2d(a, 2)
    (g,) = torch.autograd.grad(loss.sum(), n)
    return loss.detach(), weight * g


def noise_reg_f32(n, weight=1.0, grad_in=None):
    """(loss [B], grad [B, R, R]) as maua_noise_reg computes them; grad_in: the buffer's content when it accumulates"""
    n = np.asarray(n, dtype=f32)
    B = n.shape[0]
    levels = [n]
    while levels[-1].shape[-1] > 8:
        a = levels[-1]
        top, bot = a[:, 0::2, 0::2] + a[:, 0::2, 1::2], a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
        levels.append((top + bot) * f32(0.25))
    means, loss = [], np.zeros(B, dtype=f32)
    for a in levels:
        N = f32(a.shape[-1] * a.shape[-1])
        mx = red_sum_f32((a * np.roll(a, 1, 2)).reshape(B, -1)) / N
        my = red_sum_f32((a * np.roll(a, 1, 1)).reshape(B, -1)) / N
        means.append((mx, my))
        loss = loss + mx * mx
        loss = loss + my * my
    g = None
    for a, (mx, my) in zip(reversed(levels), reversed(means)):
        N = f32(a.shape[-1] * a.shape[-1])
        cx, cy = ((f32(2) * mx) / N)[:, None, None], ((f32(2) * my) / N)[:, None, None]
        hx = np.roll(a, 1, 2) + np.roll(a, -1, 2)
        hy = np.roll(a, 1, 1) + np.roll(a, -1, 1)
        v = cx * hx + cy * hy
        if g is not None:
            v = v + f32(0.25) * np.repeat(np.repeat(g, 2, 1), 2, 2)
        g = v
    out = f32(weight) * g
    return loss, (out if grad_in is None else np.asarray(grad_in, dtype=f32) + out)


def noise_reg_bound(n, weight=1.0, grad_in=None):
    """(bound on |loss_f32 - loss_f64| [B], bound on |grad_f32 - grad_f64| [B, R, R]), first order in V.
    Level k's maps carry 3 k roundings of the pooling (two adds and the add of the pairs; the quarter is exact), each relative to the
    pooled magnitudes P_k = avg_pool(|n|); a product n_k roll(n_k) adds one, the sum red_depth, the division by a power of two none:
        |d m_k| <= e_k = V (6 k + 1 + depth_k) mean(P_k roll(P_k))
    loss: 2 |m| e per mean, one rounding per square and per add (2 K adds).  grad: c = 2 m / N is exact but for m; h = left + right
    carries 3 k + 1 roundings; the two products, their sum and the K - 1 - k adds on the way down add one each; the weight one more
    (and the accumulation one)."""
    n = n.double()
    B = n.shape[0]
    K = reg_levels(n.shape[-1])
    a, P, levels = n[:, None], n.abs()[:, None], []
    for k in range(K):
        levels.append((a, P))
        a, P = F.avg_pool2d(a, 2), F.avg_pool2d(P, 2)
    loss_b, loss = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64)
    g_b = None
    g = None
    per_level = []
    for k, (a, P) in enumerate(levels):
        N = a.shape[-1] ** 2
        out = []
        for dim in (3, 2):
            m = (a * torch.roll(a, 1, dim)).mean((1, 2, 3))
            e = V * (6 * k + 1 + red_depth(N)) * (P * torch.roll(P, 1, dim)).mean((1, 2, 3))
            loss_b = loss_b + 2 * m.abs() * e + V * m * m
            loss = loss + m * m
            H = torch.roll(P, 1, dim) + torch.roll(P, -1, dim)
            out.append((m, e, H))
        per_level.append(out)
    loss_b = loss_b + 2 * K * V * loss
    for k in reversed(range(K)):
        N = levels[k][0].shape[-1] ** 2
        gb = torch.zeros_like(levels[k][1])
        for m, e, H in per_level[k]:
            c, ce = (2 * m.abs() / N)[:, None, None, None], (2 * e / N)[:, None, None, None]
            gb = gb + ce * H + V * (3 * k + 1 + 2 + (K - k)) * c * H
        if g_b is not None:
            gb = gb + 0.25 * F.interpolate(g_b, scale_factor=2, mode="nearest")
        g_b = gb
    _, g64 = noise_reg_f64(n, 1.0)
    grad_b = abs(weight) * (g_b[:, 0] + V * g64.abs())
    if grad_in is not None:
        grad_b = grad_b + V * (torch.as_tensor(grad_in).double() + weight * g64).abs()
    return loss_b, grad_b


def planted_map(B, R_, seed):
    """a map with a strong lag-1 correlation in both directions (a smooth field plus a little noise): no level's mean is near zero"""
    g = torch.Generator().manual_seed(seed)
    i = torch.arange(R_, dtype=torch.float32)
    base = torch.sin(2 * np.pi * i / R_)[:, None] + torch.cos(2 * np.pi * i / R_)[None, :] + 1.5
    return (base[None] * (1 + 0.1 * torch.arange(B)[:, None, None]) + 0.1 * torch.randn(B, R_, R_, generator=g)).float()


# ---------------------------------------------------------------------------------------------------------------- Adam, renorm
def adam_scalars_f32(lr, t, beta1=0.9, beta2=0.999, eps=1e-8):
    """the float32 scalars maua_adam_step is handed: (beta1, beta2, eps, lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)), the last two in double first"""
    return f32(beta1), f32(beta2), f32(eps), f32(lr / (1.0 - beta1 ** t)), f32(1.0 / sqrt(1.0 - beta2 ** t))


def adam_f32(p, g, m, v, sc):
    b1, b2, eps, step, inv = sc
    p, g, m, v = (np.asarray(a, dtype=f32) for a in (p, g, m, v))
    omb1, omb2 = f32(1) - b1, f32(1) - b2
    m2 = m + omb1 * (g - m)
    v2 = b2 * v + (omb2 * g) * g
    denom = np.sqrt(v2) * inv + eps
    return p - (step * m2) / denom, m2, v2


def adam_f64(p, g, m, v, sc):
    """the same update in float64 from the same float32 scalars (so the difference is the arithmetic's alone)"""
    b1, b2, eps, step, inv = (float(s) for s in sc)
    p, g, m, v = (np.asarray(a, dtype=np.float64) for a in (p, g, m, v))
    m2 = m + (1 - b1) * (g - m)
    v2 = b2 * v + (1 - b2) * g * g
    return p - step * m2 / (np.sqrt(v2) * inv + eps), m2, v2


def adam_bound(p, g, m, v, sc, dp=0.0, dm=0.0, dv=0.0):
    """bounds (dp2, dm2, dv2) on |float32 - float64| after one step, given bounds on the incoming differences of p, m, v (the same g).
    Per result one rounding V |x| + U.  m2: (g - m), the product with 1 - beta1 (itself one rounding), the sum; v2: 1 - beta2, two
    products, beta2 v, the sum; denom: sqrt, product, sum; then step m2, the quotient, the difference.  sqrt of a perturbed v:
    |sqrt(v + d) - sqrt(v)| <= min(d / (2 sqrt v), sqrt d)."""
    b1, b2, eps, step, inv = (float(s) for s in sc)
    p64, m2, v2 = adam_f64(p, g, m, v, sc)
    g, m, v = (np.asarray(a, dtype=np.float64) for a in (g, m, v))
    a = 1 - b1
    dm2 = (1 - a) * dm + a * dm + V * (3 * np.abs(a * (g - m)) + np.abs(m2)) + 3 * U
    c = 1 - b2
    dv2 = b2 * dv + V * (3 * np.abs(c * g * g) + np.abs(b2 * v) + np.abs(v2)) + 4 * U
    sq = np.sqrt(v2)
    with np.errstate(divide="ignore", invalid="ignore"):
        dsq = np.where(sq > 0, np.minimum(dv2 / (2 * sq), np.sqrt(dv2)), np.sqrt(dv2)) + V * sq + U
    denom = sq * inv + eps
    dden = inv * dsq + V * sq * inv + V * denom + 2 * U
    num = step * m2
    dnum = step * dm2 + V * np.abs(num) + U
    q = num / denom
    dq = dnum / denom + np.abs(q) * dden / denom + V * np.abs(q) + U
    dp2 = dp + dq + V * np.abs(p64) + U
    return dp2, dm2, dv2


def renorm_f32(n):
    """n [maps, N] as maua_noise_renorm leaves it"""
    n = np.asarray(n, dtype=f32)
    N = f32(n.shape[-1])
    x = n - (red_sum_f32(n) / N)[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = f32(1) / np.sqrt(red_sum_f32(x * x) / N)
        return x * c[:, None]


def expand_f32(w, eps, scale, num_ws):
    w = np.asarray(w, dtype=f32)
    v = w if eps is None else w + f32(scale) * np.asarray(eps, dtype=f32)
    return np.repeat(v, num_ws, 1) if w.shape[1] == 1 else v


def reduce_f32(g_ws):
    g_ws = np.asarray(g_ws, dtype=f32)
    t = g_ws[:, 0].copy()
    for r in range(1, g_ws.shape[1]):
        t = t + g_ws[:, r]
    return t


# ---------------------------------------------------------------------------------------------------------------- noise gradient
def synthesis_vjp_noise(p, ws, noise, g_img, nv_compat=False, rnd=None):
    """(g_ws, [g_noise_l], img): tests/synth_vjp_ref.py's hand-walk, which forms g_v = g_out gain mask in every layer, extended by
    g_noise_l = strength sum_co g_v - [B, 1, h, w] for a per-sample map, [1, 1, h, w] (summed over the batch) for a shared map or the
    layer's noise_const.  Works in the dtype of its inputs; ``rnd`` as there."""
    rec, orig = [], R.modconv_vjp

    def spy(g_out, out, x, W, s, d, nz, bias, up, flip, alpha=0.2, gain=sqrt(2), clamp=256.0):
        mask = torch.where(out > 0, torch.ones_like(out), torch.full_like(out, alpha))
        if clamp >= 0:
            mask = mask * (out.abs() < clamp)
        rec.append((g_out * gain * mask).sum(1, keepdim=True))
        return orig(g_out, out, x, W, s, d, nz, bias, up, flip, alpha, gain, clamp)

    R.modconv_vjp = spy
    try:
        g_ws, img = R.synthesis_vjp(p, ws, noise, g_img, nv_compat=nv_compat, rnd=rnd)
    finally:
        R.modconv_vjp = orig
    rec.reverse()
    layers = OS.layer_list(img.shape[-1], *R._channel_args(p))
    g_noise = []
    for l, (prefix, *_rest) in enumerate(layers):
        strength = float(p[prefix + ".noise_strength"].reshape(-1)[0]) if nv_compat and (prefix + ".noise_strength") in p else 1.0
        g = rec[l] * strength
        if noise is None or noise[l] is None or noise[l].shape[0] == 1:
            g = g.sum(0, keepdim=True)
        g_noise.append(g)
    return g_ws, g_noise, img


def autograd_noise(p, ws, noise, g_img, nv_compat=False):
    """(g_ws, [g_noise_l]) by float64 autograd of the oracle; noise entries None: the gradient to the layer's noise_const"""
    p = dict(p)
    wsr = ws.clone().requires_grad_(True)
    layers = OS.layer_list(g_img.shape[-1], *R._channel_args(p))
    leaves, nz = [], None if noise is None else list(noise)
    for l, (prefix, *_rest) in enumerate(layers):
        if noise is None or noise[l] is None:
            leaf = p[prefix + ".noise_const"].clone().requires_grad_(True)
            p[prefix + ".noise_const"] = leaf
        else:
            leaf = noise[l].clone().requires_grad_(True)
            nz[l] = leaf
        leaves.append(leaf)
    img = OS.synthesis_network(p, wsr, noise=nz, nv_compat=nv_compat)
    grads = torch.autograd.grad((img * g_img).sum(), [wsr] + leaves)
    return grads[0], [g.reshape(-1, 1, *g.shape[-2:]) for g in grads[1:]], img.detach()


# ---------------------------------------------------------------------------------------------------------------- the loop in float64
def schedule_f64(step, num_steps, w_std, lr0=0.1, noise_factor=0.05, rampdown=0.25, rampup=0.05, noise_ramp=0.75):
    """the published schedules, written out again (maua_amd.projection.schedule is the code under test)"""
    t = step / num_steps
    scale = w_std * noise_factor * max(0.0, 1.0 - t / noise_ramp) ** 2
    ramp = min(1.0, (1.0 - t) / rampdown)
    ramp = 0.5 - 0.5 * np.cos(ramp * np.pi)
    ramp = ramp * min(1.0, t / rampup)
    return lr0 * ramp, scale


def loop_grads_f64(p, w, noise, eps, scale, target, weight, num_ws, nv_compat=False):
    """float64 autograd of  1/2 sum (img - target)^2 + weight sum_l reg(noise_l)  at ws = expand(w + scale eps): (g_w, [g_noise], [reg
    loss [B] per layer], img).  w, eps [B, rows, w_dim]."""
    wr = w.double().clone().requires_grad_(True)
    nz = [n.double().clone().requires_grad_(True) for n in noise]
    wn = wr + scale * eps.double()
    ws = wn.expand(-1, num_ws, -1) if wn.shape[1] == 1 else wn
    img = OS.synthesis_network(p, ws, noise=nz, nv_compat=nv_compat)
    loss = 0.5 * ((img - target.double()) ** 2).sum()
    grads = torch.autograd.grad(loss, [wr] + nz)
    regs = [noise_reg_f64(n[:, 0], weight) for n in noise]
    return grads[0], [g + r[1][:, None] for g, r in zip(grads[1:], regs)], [r[0] for r in regs], img.detach()


def project_f64(p, target, w0, noise0, eps_of, num_steps, w_std, weight=1e5, num_ws=8, w_noise=True):
    """The whole loop in float64 with torch.optim.Adam: returns the distance 1/2 sum (img - target)^2 per step (measured at the noisy
    ws, as the loop sees it) and after the last update (without w-noise)."""
    w = w0.double().clone().requires_grad_(True)
    nz = [n.double().clone().requires_grad_(True) for n in noise0]
    opt = torch.optim.Adam([w] + nz, betas=(0.9, 0.999), lr=0.1)
    dist = []
    image = lambda wn: OS.synthesis_network(p, wn.expand(-1, num_ws, -1) if wn.shape[1] == 1 else wn, noise=nz)
    for step in range(num_steps):
        lr, scale = schedule_f64(step, num_steps, w_std)
        for gp in opt.param_groups:
            gp["lr"] = lr
        wn = w + (scale * eps_of(step).double() if w_noise else 0.0)
        d = 0.5 * ((image(wn) - target.double()) ** 2).sum()
        reg = 0.0
        for n in nz:
            a = n
            while True:
                reg = reg + ((a * torch.roll(a, 1, 3)).mean((1, 2, 3)) ** 2 + (a * torch.roll(a, 1, 2)).mean((1, 2, 3)) ** 2).sum()
                if a.shape[-1] <= 8:
                    break
                a = F.avg_pool2d(a, 2)
        opt.zero_grad()
        (d + weight * reg).backward()
        opt.step()
        dist.append(float(d.detach()))
        with torch.no_grad():
            for n in nz:
                n -= n.mean((1, 2, 3), keepdim=True)
                n *= n.square().mean((1, 2, 3), keepdim=True).rsqrt()
    with torch.no_grad():
        final = float(0.5 * ((image(w) - target.double()) ** 2).sum())
    return dist, final


# ---------------------------------------------------------------------------------------------------------------- the tests' inputs
REG_CASES = [(R_, B, kind) for R_ in (4, 8, 16, 64) for B in (1, 3) for kind in ("random", "planted")] + [(1024, 1, "planted")]


def reg_input(R_, B, kind):
    """[B, R, R] float32: the map of a case, and what the gradient buffer holds before an accumulating call"""
    g = torch.Generator().manual_seed(1000 * R_ + B)
    n = torch.randn(B, R_, R_, generator=g) if kind == "random" else planted_map(B, R_, R_ + B)
    return n.float(), torch.randn(B, R_, R_, generator=g).float()


ADAM_SIZES = (1, 63, 65541)


def adam_input(n, steps=3):
    """(p, m, v, [g per step]) float32 numpy; the gradients hold zeros and denormals (and the moments start at zero, as a run's do)"""
    r = np.random.RandomState(n)
    p = r.randn(n).astype(f32)
    gs = []
    for s in range(steps):
        g = (r.randn(n) * 10.0 ** r.uniform(-6, 2, n)).astype(f32)
        g[r.rand(n) < 0.1] = 0.0
        den = r.rand(n) < 0.1
        g[den] = (r.randn(n)[den] * 1e-41).astype(f32)      # denormals (below 1.18e-38)
        gs.append(g)
    if n == 1:
        gs[0][:] = 0.0                                       # g = 0 at m = v = 0: the quotient is 0 / eps
        gs[1][:] = f32(3e-42)
    return p, np.zeros(n, f32), np.zeros(n, f32), gs


def adam_lrs(steps=3):
    return [0.02 * (s + 1) for s in range(steps)]


def small_mapper_params(seed=6, layers=2):
    g = torch.Generator().manual_seed(seed)
    mp = {k: v.double() for k, v in OS.init_mapping_params(64, 64, layers, generator=g).items()}
    mp["w_avg"] = torch.zeros(64, dtype=torch.float64)
    return mp


def w_statistics_f64(mp, samples, num_ws=8):
    z = torch.from_numpy(np.random.RandomState(123).randn(samples, 64)).float().double()
    w = OS.mapping_network(mp, z, num_ws_=num_ws)[:, 0]
    w_avg = w.mean(0)
    return w_avg, float(((w - w_avg) ** 2).sum().div(samples).sqrt())


def philox_normal(seed, stream, shape):
    from oracle import rng
    return torch.from_numpy(rng.normal(seed, stream, int(np.prod(shape))).reshape(shape).copy())
