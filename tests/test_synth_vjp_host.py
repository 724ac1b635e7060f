"""Without a device: the hand-walked float64 gradients of tests/synth_vjp_ref.py (what the device kernels are compared to) against
torch.autograd on the oracle; the host-only refusals of the gradient entry points; the Langevin update, schedule and padding.

Bound of the float64 comparisons: 1e-10 relative to the largest reference entry.  Both sides are float64 (eps 1.1e-16); the float32
autograd of the same graph sits at 3.3e-7 = 3 eps_32 against float64, so its float64 twin is near 1e-15: five orders of headroom."""
import ctypes
import sys
from math import sqrt
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import synth_vjp_ref as R  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from oracle import ops as OO, stylegan2 as OS  # noqa: E402

RES, W_DIM, CBASE, CMAX, B = 32, 64, 1024, 64, 2
BOUND = 1e-10


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def make_net(seed, dtype=torch.float64, nv=False):
    g = torch.Generator().manual_seed(seed)
    p = OS.init_synthesis_params(RES, W_DIM, 3, CBASE, CMAX, generator=g)
    for k in list(p):
        if k.endswith(".bias") and ".affine" not in k:
            p[k] = 0.3 * torch.randn(p[k].shape, generator=g)
        if nv and k.endswith(".noise_const"):
            p[k.replace("noise_const", "noise_strength")] = 0.5 + torch.rand(1, generator=g)
    p = {k: v.to(dtype) for k, v in p.items()}
    ws = torch.randn(B, OS.num_ws(RES), W_DIM, generator=g).to(dtype)
    noise = [torch.randn(B, 1, r, r, generator=g).to(dtype) for _, _, _, r, _ in OS.layer_list(RES, CBASE, CMAX)]
    g_img = torch.randn(B, 3, RES, RES, generator=g).to(dtype)
    return p, ws, noise, g_img


@pytest.fixture(scope="module", params=[False, True], ids=["in_tree", "nv_compat"])
def net(request):
    nv = request.param
    p, ws, noise, g_img = make_net(5, nv=nv)
    wsr = ws.clone().requires_grad_(True)
    img, feats = OS.synthesis_network(p, wsr, noise=noise, nv_compat=nv, return_features=True)
    (auto,) = torch.autograd.grad((img * g_img).sum(), wsr)
    return dict(nv=nv, p=p, ws=ws, noise=noise, g_img=g_img, img=img.detach(), feats=[f.detach() for f in feats], auto=auto)


def test_network_walk_matches_autograd(net):
    g_ws, img = R.synthesis_vjp(net["p"], net["ws"], net["noise"], net["g_img"], nv_compat=net["nv"])
    assert torch.equal(img, net["img"])
    err = rel(g_ws, net["auto"])
    print(f"nv_compat={net['nv']}: hand-walked vs autograd {err:.2e}")
    assert err <= BOUND
    # the shape exercises what it should: every ws row gets a gradient, no feature sits exactly on the lrelu kink, the 256 clamp is idle
    assert all(float(net["auto"][:, r].abs().max()) > 0 for r in range(net["ws"].shape[1]))
    assert all(float((f == 0).sum()) == 0 for f in net["feats"])
    assert max(float(f.abs().max()) for f in net["feats"]) < 256


@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("flip", [0, 1])
def test_layer_with_active_clamp(up, flip):
    """clamp = 1.0 clips a large share of the outputs: the mask taken from the kept output is the clamp's own"""
    g = torch.Generator().manual_seed(11 + up)
    Bn, Ci, Co, H, W = 2, 8, 6, 5, 7
    x = torch.randn(Bn, Ci, H, W, generator=g, dtype=torch.float64)
    Wt = torch.randn(Co, Ci, 3, 3, generator=g, dtype=torch.float64)
    s = (1 + 0.5 * torch.randn(Bn, Ci, generator=g, dtype=torch.float64))
    noise = torch.randn(Bn, 1, H * up, W * up, generator=g, dtype=torch.float64)
    bias = torch.randn(Co, generator=g, dtype=torch.float64)
    g_out = torch.randn(Bn, Co, H * up, W * up, generator=g, dtype=torch.float64)
    xr, sr = x.clone().requires_grad_(True), s.clone().requires_grad_(True)
    y = OO.modulated_conv2d(xr, Wt, sr, noise=noise, up=up, padding=1, resample_filter=OO.setup_filter([1, 3, 3, 1]).double(),
                            flip_weight=bool(flip))
    out = OO.bias_act(y, bias, act="lrelu", clamp=1.0)
    clipped = float((out.abs() >= 1.0).double().mean())
    assert 0.2 < clipped < 0.9, clipped
    ax, as_ = torch.autograd.grad((out * g_out).sum(), (xr, sr))
    d, _ = R.demod_of(Wt, s)
    mine = R.modconv_forward(x, Wt, s, d, noise, bias, up, flip, clamp=1.0)
    assert rel(mine, out.detach()) <= BOUND
    g_x, g_s = R.modconv_vjp(g_out, out.detach(), x, Wt, s, d, noise, bias, up, flip, clamp=1.0)
    assert rel(g_x, ax) <= BOUND and rel(g_s, as_) <= BOUND, (rel(g_x, ax), rel(g_s, as_))


def test_torgb_and_skip_adjoints():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 8, 6, 10, generator=g, dtype=torch.float64)
    wmod = torch.randn(2, 3, 8, generator=g, dtype=torch.float64)
    bias = torch.randn(3, generator=g, dtype=torch.float64)
    g_y = torch.randn(2, 3, 6, 10, generator=g, dtype=torch.float64)
    xr, wr = x.clone().requires_grad_(True), wmod.clone().requires_grad_(True)
    y = R.torgb_forward(xr, wr, bias, clamp=1.5)
    assert 0.05 < float((y.abs() >= 1.5).double().mean()) < 0.95
    ax, aw = torch.autograd.grad((y * g_y).sum(), (xr, wr))
    g_x, g_w = R.torgb_vjp(g_y, x, wmod, bias, clamp=1.5)
    assert rel(g_x, ax) <= BOUND and rel(g_w, aw) <= BOUND
    img = torch.randn(2, 3, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    g_up = torch.randn(2, 3, 10, 14, generator=g, dtype=torch.float64)
    (a,) = torch.autograd.grad((OO.upsample2d(img, OO.setup_filter([1, 3, 3, 1]).double()) * g_up).sum(), img)
    assert rel(R.skip_vjp(g_up), a) <= BOUND


@pytest.mark.parametrize("nv", [False, True])
def test_mapper_walk_matches_autograd(nv):
    g = torch.Generator().manual_seed(9)
    # (the in-tree x @ w form needs square layers: z_dim == w_dim)
    p = {k: v.double() for k, v in OS.init_mapping_params(48 if nv else 64, 64, 8, generator=g).items()}
    p["w_avg"] = torch.randn(64, generator=g, dtype=torch.float64)
    for i in range(8):
        p[f"fcs.{i}.bias"] = torch.randn(64, generator=g, dtype=torch.float64) * 30
    z = torch.randn(3, p["fcs.0.weight"].shape[1], generator=g, dtype=torch.float64)
    g_ws = torch.randn(3, 8, 64, generator=g, dtype=torch.float64)
    zr = z.clone().requires_grad_(True)
    ws = OS.mapping_network(p, zr, truncation_psi=0.7, num_ws_=8, nv_compat=nv, truncation_cutoff=4)
    (a,) = torch.autograd.grad((ws * g_ws).sum(), zr)
    mine, kept = R.mapping_forward_kept(p, z, 0.7, 4, num_ws=8, nv_compat=nv)
    assert rel(mine, ws.detach()) <= BOUND
    assert rel(R.mapping_vjp(p, kept, g_ws, nv_compat=nv), a) <= BOUND
    # all rows (no cutoff)
    zr = z.clone().requires_grad_(True)
    ws = OS.mapping_network(p, zr, truncation_psi=0.5, num_ws_=8, nv_compat=nv)
    (a,) = torch.autograd.grad((ws * g_ws).sum(), zr)
    _, kept = R.mapping_forward_kept(p, z, 0.5, None, num_ws=8, nv_compat=nv)
    assert rel(R.mapping_vjp(p, kept, g_ws, nv_compat=nv), a) <= BOUND


# ---------------------------------------------------------------------------------------------------------------- refusals, no device
def desc(**kw):
    one = 4096   # any non-NULL address: the checks never dereference
    d = L.ModconvDesc(x=one, x_bstride=4 * 4 * 64, w=one, flip=0, s=one, d=one, noise=None, noise_bstride=0, noise_strength=1.0,
                      noise_scale=None, bias=one, y=one, B=2, H=4, W=4, Ci=64, Co=64, up=1, act=L.ACTS["lrelu"], alpha=0.2,
                      gain=sqrt(2), clamp=256.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def refused(rc):
    assert rc != 0
    return L.lib().maua_last_error().decode()


def test_modconv_vjp_check_refusals():
    lib, one = L.lib(), 4096
    chk = lambda d, g_y=one, g_s=one, dt=L.F32: lib.maua_modconv_vjp_check(ctypes.byref(d), g_y, g_s, dt)
    assert chk(desc()) == 0 and chk(desc(up=2), dt=L.BF16) == 0 and chk(desc(d=None, bias=None, act=L.ACTS["linear"])) == 0
    assert lib.maua_modconv_vjp_check(None, one, one, L.F32) != 0
    assert "MAUA_F16 is not differentiated" in refused(chk(desc(), dt=L.F16))
    assert "dtype must be MAUA_F32 or MAUA_BF16" in refused(chk(desc(), dt=L.F32_SPLIT))
    assert "NULL w / g_y / g_s" in refused(chk(desc(), g_y=None))
    assert "NULL w / g_y / g_s" in refused(chk(desc(), g_s=None))
    assert "NULL w / g_y / g_s" in refused(chk(desc(w=None)))
    assert "noise scales are not differentiated" in refused(chk(desc(noise_scale=one)))
    assert "describe the plain layer" in refused(chk(desc(out_scale=one)))
    assert "describe the plain layer" in refused(chk(desc(rgb_out=one)))
    assert "bad shape" in refused(chk(desc(H=0)))
    assert "up must be 1 or 2" in refused(chk(desc(up=3)))
    assert "multiples of 32" in refused(chk(desc(Ci=48)))
    assert "multiples of 32" in refused(chk(desc(Co=16)))
    assert "NULL x / y / g_y / s / g_s" in refused(chk(desc(y=None)))
    assert "NULL x / y / g_y / s / g_s" in refused(chk(desc(s=None)))
    assert "samples of x overlap" in refused(chk(desc(x_bstride=100)))
    assert chk(desc(x_bstride=0)) == 0
    assert "linear or lrelu" in refused(chk(desc(act=L.ACTS["tanh"])))
    assert "gain must be positive" in refused(chk(desc(gain=0.0)))
    assert "32-bit offsets" in refused(chk(desc(H=4096, W=4096, Ci=512, Co=512, x_bstride=4096 * 4096 * 512)))
    assert "grid too large" in refused(chk(desc(B=70000)))


def test_torgb_vjp_check_refusals():
    lib, one = L.lib(), 4096
    ok = dict(x=one, wmod=one, bias=one, g_img=one, g_x=one, g_wmod=one, B=2, H=4, W=4, C=64, dtype=L.BF16)
    chk = lambda **kw: lib.maua_torgb_vjp_check(*{**ok, **kw}.values())
    assert chk() == 0 and chk(dtype=L.F32) == 0
    assert "MAUA_F16 is not differentiated" in refused(chk(dtype=L.F16))
    assert "dtype must be MAUA_F32 or MAUA_BF16" in refused(chk(dtype=L.F32_SPLIT))
    for k in ("x", "wmod", "bias", "g_img", "g_x", "g_wmod"):
        assert "NULL argument" in refused(chk(**{k: None}))
    assert "bad shape" in refused(chk(W=0))
    assert "multiple of 32" in refused(chk(C=48))
    assert "32-bit offsets" in refused(chk(H=1 << 14, W=1 << 14))


def test_synth_vjp_check_without_a_net():
    assert "net is NULL" in refused(L.lib().maua_synth_vjp_check(None, 2))
    assert "net is NULL" in refused(L.lib().maua_synth_vjp(None, None, None, 2, None, None))


# ---------------------------------------------------------------------------------------------------------------- Langevin
def test_langevin_update_schedule_and_padding():
    from maua_amd import sampling as S
    D, bs, steps = 6, 4, 7
    target = torch.linspace(-1, 1, D)
    loss_grad = lambda z: 0.3 * (z - target.to(z))          # loss = 0.15 |z - target|^2
    zs = torch.randn(5, D, generator=torch.Generator().manual_seed(1))
    gen = torch.Generator().manual_seed(2)
    padded = S.pad_latents(zs, bs, gen)
    assert padded.shape == (8, D) and torch.equal(padded[:5], zs)
    # the same stream drawn here: padding first, then one [P, D] draw per step
    gen2 = torch.Generator().manual_seed(2)
    pad = torch.randn((8, D), generator=gen2)
    assert torch.equal(pad[5:], padded[5:])
    eps = torch.stack([torch.randn((8, D), generator=gen2) for _ in range(steps)]) * sqrt(2.0)
    seen = []
    out = S.langevin_loop(padded.clone(), loss_grad, bs, 0.1, 2.0, 0.25, 3, steps, gen,
                          on_step=lambda i, z, g, e: seen.append((z.clone(), g.clone(), e.clone())))
    traj = R.langevin_reference(zs, loss_grad, eps, bs=bs, rate=0.1, decay=0.25, decay_steps=3, pad=pad)
    assert len(seen) == steps
    for i, (z, g, e) in enumerate(seen):
        assert torch.equal(e, eps[i])
        assert float((z.double() - traj[i]).abs().max()) <= 1e-5
        assert float((g.double() - (traj[i] + loss_grad(traj[i]))).abs().max()) <= 1e-5
    assert float((out.double() - traj[-1]).abs().max()) <= 1e-5
    assert R.langevin_schedule(0.1, 0.25, 3, 7) == [(0.1, 1.0)] * 3 + [(0.025, 0.25)] * 3 + [(0.00625, 0.0625)]
    assert R.langevin_schedule(0.1, 0.0, 3, 4) == [(0.1, 1.0)] * 4
    # no noise: the step is the plain gradient step
    one = S.langevin_loop(padded.clone(), loss_grad, bs, 0.1, 0.0, 0.25, 200, 1, torch.Generator().manual_seed(0))
    assert torch.allclose(one, padded - 0.05 * (padded + loss_grad(padded)), atol=1e-7)


def test_critics_and_strategies_that_are_refused():
    from maua_amd import sampling as S
    with pytest.raises(NotImplementedError, match="discriminator"):
        S.prepare_critic("discriminator")
    with pytest.raises(TypeError):
        S.prepare_critic(3)

    class G:
        z_dim = 8
    with pytest.raises(NotImplementedError):
        S.sample_latents(G, [1, 2], 2, 1.0, "polarity", None)
    zs = S.sample_latents(G, [1, 2], 2, 1.0, "standard", None)
    import numpy as np
    assert zs.shape == (2, 8) and torch.equal(zs[1], torch.from_numpy(np.random.RandomState(2).randn(1, 8)).float()[0])
    assert S.parse_seed_list("1,3,6-9") == [1, 3, 6, 7, 8]
    grid = S.tile_grid(torch.arange(5.0)[:, None, None, None].expand(5, 3, 2, 2), 3)
    assert grid.shape == (1, 3, 4, 6) and float(grid[0, 0, 2, 2]) == 4.0 and float(grid[0, 0, 3, 5]) == 0.0
    from maua.GAN import generate_images as shim
    from maua.GAN.sampling import langevin_with_critic
    assert shim.generate_images is S.generate_images and langevin_with_critic is S.langevin_with_critic
