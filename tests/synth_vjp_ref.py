"""Hand-walked gradients of the StyleGAN2 generator to its latents, without autograd: the restatement the device kernels
(csrc/modconv_vjp.hip, csrc/synth_vjp.hip, MappingNetwork.vjp, maua_amd.sampling) are held against.  Every function works in the
dtype of its inputs (the tests feed float64) and is itself compared to torch.autograd on the oracle (tests/test_synth_vjp_host.py).

Layer forward (NCHW here), s = styles, d = demodulation coefficients:
    u = conv(W, s x);  v = d u + noise + bias;  out = clamp(lrelu(v) gain, clamp);  d = rsqrt(sum_ci s^2 Wsq + 1e-8), Wsq = sum_taps W^2
"""
from math import ceil, sqrt

import torch
import torch.nn.functional as F

from oracle import ops as OO, stylegan2 as OS

FIR4 = (0.25, 0.75, 0.75, 0.25)   # [1, 3, 3, 1] / 8 per axis with the up-sampling gain 2 per axis


def fir2d(dtype):
    f = torch.tensor(FIR4, dtype=dtype)
    return torch.outer(f, f)


def styles_of(p, prefix, w, scale=1.0):
    """FullyConnectedLayer (linear): w @ (A / sqrt(w_dim))^T + b, times toRGB's 1 / sqrt(C)"""
    A = p[prefix + ".affine.weight"]
    return (w @ (A / sqrt(A.shape[1])).T + p[prefix + ".affine.bias"]) * scale


def demod_of(W, s):
    wsq = (W * W).sum((2, 3))                             # [Co][Ci]
    return ((s * s) @ wsq.T + 1e-8).rsqrt(), wsq          # [B][Co]


def modconv_forward(x, W, s, d, noise, bias, up, flip, alpha=0.2, gain=sqrt(2), clamp=256.0):
    """the layer from caller-chosen s and d (d None: no demodulation), as maua_modconv_ex documents it"""
    xs = x * s[:, :, None, None]
    if up == 1:
        u = F.conv2d(xs, W, padding=1)
    else:
        Wt = W.flip([2, 3]) if flip else W
        t = F.conv_transpose2d(xs, Wt.transpose(0, 1), stride=2)              # [2H + 1]
        u = F.conv2d(F.pad(t, (1, 1, 1, 1)), fir2d(x.dtype)[None, None].repeat(W.shape[0], 1, 1, 1), groups=W.shape[0])
    v = u if d is None else u * d[:, :, None, None]
    if noise is not None:
        v = v + noise
    if bias is not None:
        v = v + bias[None, :, None, None]
    o = torch.where(v > 0, v, v * alpha) * gain
    return o.clamp(-clamp, clamp) if clamp >= 0 else o


def modconv_vjp(g_out, out, x, W, s, d, noise, bias, up, flip, alpha=0.2, gain=sqrt(2), clamp=256.0):
    """(g_x, g_s) from the kept output: the steps of csrc/modconv_vjp.hip"""
    mask = torch.where(out > 0, torch.ones_like(out), torch.full_like(out, alpha))   # (python scalars would make it float32)
    if clamp >= 0:
        mask = mask * (out.abs() < clamp)
    g_v = g_out * gain * mask
    g_d = None
    if d is not None:
        v = torch.where(out > 0, out / gain, out / gain / alpha)
        if noise is not None:
            v = v - noise
        if bias is not None:
            v = v - bias[None, :, None, None]
        u = torch.where(g_v != 0, v / d[:, :, None, None], torch.zeros_like(v))
        g_d = (g_v * u).sum((2, 3))
    g_u = g_v if d is None else g_v * d[:, :, None, None]
    if up == 1:   # 3x3 correlation with Wt[ci][co][t] = W[co][ci][8 - t]
        g_xm = F.conv2d(g_u, W.transpose(0, 1).flip([2, 3]), padding=1)
    else:         # FIR adjoint (pad 2, the same symmetric filter), then the stride-2 gather over g_t
        Co = W.shape[0]
        g_t = F.conv2d(F.pad(g_u, (2, 2, 2, 2)), fir2d(x.dtype)[None, None].repeat(Co, 1, 1, 1), groups=Co)   # [2H + 1]
        Wt = W.flip([2, 3]) if flip else W
        g_xm = F.conv2d(g_t, Wt.transpose(0, 1), stride=2)     # g_xm[ci][i][j] = sum W[co][ci][kh][kw] g_t[co][2i + kh][2j + kw]
    g_x = g_xm * s[:, :, None, None]
    g_s = (x * g_xm).sum((2, 3))
    if d is not None:
        wsq = (W * W).sum((2, 3))
        g_s = g_s - s * ((g_d * d ** 3) @ wsq)
    return g_x, g_s


def torgb_forward(x, wmod, bias, clamp=256.0):
    y = torch.einsum("bchw,bkc->bkhw", x, wmod) + bias[None, :, None, None]
    return y.clamp(-clamp, clamp) if clamp >= 0 else y


def torgb_vjp(g_y, x, wmod, bias, clamp=256.0):
    """(g_x, g_wmod): y is recomputed for its clamp mask"""
    y = torch.einsum("bchw,bkc->bkhw", x, wmod) + bias[None, :, None, None]
    if clamp >= 0:
        g_y = g_y * (y.abs() < clamp)
    return torch.einsum("bkhw,bkc->bchw", g_y, wmod), torch.einsum("bchw,bkhw->bkc", x, g_y)


def skip_vjp(g_img):
    """upsample2d^T: upfirdn2d with down 2, padding (1, 2, 1, 2), gain 4"""
    c = g_img.shape[1]
    return F.conv2d(F.pad(g_img, (1, 2, 1, 2)), fir2d(g_img.dtype)[None, None].repeat(c, 1, 1, 1), groups=c)[:, :, ::2, ::2]


def to_bf16(t):
    """the value a tensor has once stored as bfloat16"""
    return t.float().bfloat16().to(t.dtype)


def forward_kept(p, ws, noise, nv_compat, rnd):
    """oracle.stylegan2.synthesis_network with every layer's output passed through ``rnd`` before anything reads it"""
    nblocks = ws.shape[1] // 2
    f = OO.setup_filter([1, 3, 3, 1]).to(ws.dtype)
    x = p["bs.0.const"][None].repeat(ws.shape[0], 1, 1, 1)
    feats, img, li = [], None, 0
    for blk in range(nblocks):
        for which, up in (("conv0", 2), ("conv1", 1)):
            if blk == 0 and which == "conv0":
                continue
            x = rnd(OS.synthesis_layer(p, f"bs.{blk}.{which}", x, ws[:, li], up=up, noise=None if noise is None else noise[li],
                                       nv_compat=nv_compat))
            feats.append(x)
            li += 1
        y = OS.torgb_layer(p, f"bs.{blk}.torgb", x, ws[:, li])
        img = y if img is None else OO.upsample2d(img, f) + y
    return img, feats


def synthesis_vjp(p, ws, noise, g_img, nv_compat=False, rnd=None):
    """d loss / d ws of oracle.stylegan2.synthesis_network ('skip'): a forward that keeps every layer's output, then the walk from the
    last block to the first.  ``rnd`` (to_bf16): the emulation of a 16-bit network - the convolution weights, every layer's output
    and every gradient that crosses a layer boundary take the values they have once stored in that type; everything else float64."""
    if rnd is None:
        rnd = lambda v: v
        img, feats = OS.synthesis_network(p, ws, noise=noise, nv_compat=nv_compat, return_features=True)
    else:
        p = {k: (rnd(v) if k.endswith(("conv0.weight", "conv1.weight")) else v) for k, v in p.items()}
        img, feats = forward_kept(p, ws, noise, nv_compat, rnd)
    B, num_ws, w_dim = ws.shape
    layers = OS.layer_list(img.shape[-1], *_channel_args(p))
    g_ws = torch.zeros_like(ws)
    wg = 1 / sqrt(w_dim)
    nblocks = num_ws // 2
    const = p["bs.0.const"][None].repeat(B, 1, 1, 1)

    def layer_vjp(li, g_y):
        prefix, ci, co, res, up = layers[li]
        x = const if li == 0 else feats[li - 1]
        W = p[prefix + ".weight"]
        s = styles_of(p, prefix, ws[:, li])
        d, _ = demod_of(W, s)
        strength = float(p[prefix + ".noise_strength"].reshape(-1)[0]) if nv_compat and (prefix + ".noise_strength") in p else 1.0
        nz = (p[prefix + ".noise_const"] if noise is None or noise[li] is None else noise[li]) * strength
        g_x, g_s = modconv_vjp(g_y, feats[li], x, W, s, d, nz, p[prefix + ".bias"], up, nv_compat)
        g_ws[:, li] += g_s @ p[prefix + ".affine.weight"] * wg
        return g_x

    g_feat = None
    li = len(layers)
    for blk in reversed(range(nblocks)):
        prefix = f"bs.{blk}.torgb"
        x = feats[li - 1]
        C = x.shape[1]
        wrgb = p[prefix + ".weight"][:, :, 0, 0]
        s = styles_of(p, prefix, ws[:, li], 1 / sqrt(C))
        g_x, g_wmod = torgb_vjp(g_img, x, wrgb[None] * s[:, None], p[prefix + ".bias"])
        g_feat = rnd(g_x if g_feat is None else g_feat + g_x)
        g_ws[:, li] += (g_wmod * wrgb[None]).sum(1) @ p[prefix + ".affine.weight"] * (wg / sqrt(C))
        if blk > 0:
            g_img = skip_vjp(g_img)
        g_feat = rnd(layer_vjp(li - 1, g_feat))     # conv1
        li -= 1
        if blk > 0:
            g_feat = rnd(layer_vjp(li - 1, g_feat)) # conv0
            li -= 1
    return g_ws, img


def _channel_args(p):
    """(channel_base, channel_max) that reproduce the parameter dict's channel counts through oracle.stylegan2.layer_list"""
    res, chans, i = 4, {}, 0
    while f"bs.{i}.conv1.weight" in p:
        chans[res] = p[f"bs.{i}.conv1.weight"].shape[0]
        res, i = res * 2, i + 1
    cmax = max(chans.values())
    base = max(r * c for r, c in chans.items())
    assert all(min(base // r, cmax) == c for r, c in chans.items()), chans
    return base, cmax


def mapping_forward_kept(p, z, truncation_psi=1.0, truncation_cutoff=None, num_ws=8, lr_multiplier=0.01, nv_compat=False):
    """(ws, kept): oracle.stylegan2.mapping_network with every layer's pre-activation kept"""
    x = z * ((z * z).mean(1, keepdim=True) + 1e-8).rsqrt()
    pre, i = [], 0
    while f"fcs.{i}.weight" in p:
        w = p[f"fcs.{i}.weight"] * (lr_multiplier / sqrt(p[f"fcs.{i}.weight"].shape[1]))
        y = x @ (w.T if nv_compat else w) + p[f"fcs.{i}.bias"] * lr_multiplier
        pre.append(y)
        x = torch.where(y > 0, y, 0.2 * y) * sqrt(2)
        i += 1
    ws = x[:, None].repeat(1, num_ws, 1)
    if truncation_psi != 1:
        n = num_ws if truncation_cutoff is None else truncation_cutoff
        ws[:, :n] = p["w_avg"] + truncation_psi * (ws[:, :n] - p["w_avg"])
    return ws, dict(z=z, pre=pre, psi=truncation_psi, cutoff=truncation_cutoff)


def mapping_vjp(p, kept, g_ws, lr_multiplier=0.01, nv_compat=False):
    num_ws = g_ws.shape[1]
    scale = torch.ones(num_ws, dtype=g_ws.dtype)
    if kept["psi"] != 1:
        scale[:num_ws if kept["cutoff"] is None else kept["cutoff"]] = kept["psi"]
    g = (g_ws * scale[None, :, None]).sum(1)
    for i in reversed(range(len(kept["pre"]))):
        w = p[f"fcs.{i}.weight"] * (lr_multiplier / sqrt(p[f"fcs.{i}.weight"].shape[1]))
        g = g * torch.where(kept["pre"][i] > 0, torch.ones_like(g), torch.full_like(g, 0.2)) * sqrt(2)
        g = g @ (w if nv_compat else w.T)
    z = kept["z"]
    r = ((z * z).mean(1, keepdim=True) + 1e-8).rsqrt()
    return r * g - z * r ** 3 * (z * g).mean(1, keepdim=True)


def langevin_schedule(rate, decay, decay_steps, steps):
    """[(rate, scaler)] per step: both multiplied by decay after every decay_steps steps (langevin.py:129-131)"""
    out, scaler = [], 1.0
    for i in range(steps):
        out.append((rate, scaler))
        if decay > 0 and decay_steps > 0 and (i + 1) % decay_steps == 0:
            rate, scaler = rate * decay, scaler * decay
    return out


def langevin_reference(zs, loss_grad, eps, bs=8, rate=0.1, decay=0.25, decay_steps=200, pad=None):
    """the update in float64 with the noise draws handed in: zs [l, D], eps [steps, P, D] (P = l padded to a multiple of bs with the
    rows of ``pad``), loss_grad(z) -> d loss / d z.  Returns every step's latents [steps + 1, P, D]."""
    l, P = len(zs), bs * ceil(len(zs) / bs)
    z = torch.zeros((P, zs.shape[1]), dtype=torch.float64)
    if P > l:
        z[l:] = pad[l:].double()
    z[:l] = zs.double()
    traj = [z]
    for (r, sc), e in zip(langevin_schedule(rate, decay, decay_steps, len(eps)), eps.double()):
        z = z - 0.5 * r * (z + loss_grad(z)) + sqrt(r) * sc * e
        traj.append(z)
    return torch.stack(traj)
