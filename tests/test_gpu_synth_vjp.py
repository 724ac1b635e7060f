"""On the device: the gradient kernels of one synthesis layer (maua_modconv_vjp_ex, maua_torgb_vjp_ex), the network walk
(SynthesisNetwork.vjp), the mapper's, StyleGAN2.latent_grad, Langevin sampling and the generate_images command line - against the
float64 autograd of the oracle.

Bounds.  float32 (exact-f32 matrix cores): 4e-5 of the largest reference entry - twice the 2e-5 tests/test_gpu_synth.py holds the same
kernels' forward to, because a gradient passes each layer's arithmetic twice.  bfloat16: relative L2 error at most twice a floor the
test computes from the oracle alone (tests/synth_vjp_ref.py with ``rnd=to_bf16``: weights, layer outputs and the gradients that cross
a layer boundary rounded to bfloat16, everything else float64) - the device also rounds the modulated operand and g_u inside its
kernels, which the emulation does not."""
import ctypes as C
import sys
from math import sqrt
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import synth_vjp_ref as R  # noqa: E402
from test_synth_vjp_host import CBASE, CMAX, RES, W_DIM, make_net  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from maua_amd.grad import GradModule  # noqa: E402
from oracle import ops as OO, stylegan2 as OS  # noqa: E402

pytestmark = pytest.mark.gpu
F32_BOUND = 4e-5
DT = {"f32": torch.float32, "bf16": torch.bfloat16}


def rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


def rel_l2(a, b):
    return float((a.double().cpu() - b).norm() / b.norm())


def nhwc(t, dt):
    return t.permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=dt)


def nchw64(t):
    return t.double().cpu().permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- one layer
SHAPES = [(4, 4, 64, 64, 1), (4, 8, 64, 32, 3), (12, 20, 32, 64, 2)]   # H, W, Ci, Co, B: below a tile; H / W and Ci / Co told apart; partial tiles


def layer_case(shape, up, variant, dt, seed=0):
    """A layer's operands (x and g_y already holding values of the network dtype), its forward on the device (the kept output), the
    device gradient, the float64 autograd of the oracle at the same operands, and the float64 walk from the device's kept output."""
    H, W, Ci, Co, B = shape
    g = torch.Generator().manual_seed(100 * H + 10 * up + seed)
    tdt = DT[dt]
    flip = int(variant == "flip")
    clamp = 1.0 if variant == "clamp" else 256.0
    nb = 1 if variant == "noise_bcast" else B
    x = torch.randn(B, Ci, H, W, generator=g).to(tdt).double()
    Wt = torch.randn(Co, Ci, 3, 3, generator=g)
    s = 1 + 0.5 * torch.randn(B, Ci, generator=g)
    noise = torch.randn(nb, 1, H * up, W * up, generator=g)
    bias = torch.randn(Co, generator=g)
    g_y = torch.randn(B, Co, H * up, W * up, generator=g).to(tdt).double()
    d, _ = R.demod_of(Wt.double(), s.double())
    dev = dict(x=nhwc(x, tdt), w=Wt.cuda(), s=s.cuda(), d=d.float().cuda(), noise=noise.cuda(), bias=bias.cuda(),
               y=torch.empty(B, H * up, W * up, Co, dtype=tdt, device="cuda"), g_y=nhwc(g_y, tdt),
               g_x=torch.full((B, H, W, Ci), float("nan"), dtype=tdt, device="cuda"),
               g_s=torch.full((B, Ci), float("nan"), device="cuda"))
    desc = L.ModconvDesc(x=dev["x"].data_ptr(), x_bstride=H * W * Ci, w=dev["w"].data_ptr(), flip=flip, s=dev["s"].data_ptr(),
                         d=dev["d"].data_ptr(), noise=dev["noise"].data_ptr(), noise_bstride=0 if nb == 1 else H * up * W * up,
                         noise_strength=1.0, noise_scale=None, bias=dev["bias"].data_ptr(), y=dev["y"].data_ptr(), B=B, H=H, W=W, Ci=Ci,
                         Co=Co, up=up, act=L.ACTS["lrelu"], alpha=0.2, gain=sqrt(2), clamp=clamp)
    lib = L.lib()
    L.check(lib.maua_modconv_ex(L.ctx(), C.byref(desc), None, L.dtype_id(tdt), L.ROUTES["generic"], 0, 1))
    L.check(lib.maua_modconv_vjp_ex(L.ctx(), C.byref(desc), L.ptr(dev["g_y"]), L.ptr(dev["g_x"]), L.ptr(dev["g_s"]), L.dtype_id(tdt)))
    torch.cuda.synchronize()
    xr, sr = x.clone().requires_grad_(True), s.double().requires_grad_(True)
    out = OO.bias_act(OO.modulated_conv2d(xr, Wt.double(), sr, noise=noise.double(), up=up, padding=1,
                                          resample_filter=OO.setup_filter([1, 3, 3, 1]).double(), flip_weight=bool(flip)),
                      bias.double(), act="lrelu", clamp=clamp)
    ax, as_ = torch.autograd.grad((out * g_y).sum(), (xr, sr))
    # the operator's own contract in float64: the kept output is one of its INPUTS, so its exact result for the device's y is the
    # hand-walk (pinned to autograd at 1e-15 in tests/test_synth_vjp_host.py) evaluated at that y
    y_dev = nchw64(dev["y"])
    hx, hs = R.modconv_vjp(g_y, y_dev, x, Wt.double(), s.double(), d, noise.double(), bias.double(), up, flip, clamp=clamp)
    return dict(dev=dev, desc=desc, out=out.detach(), ax=ax, as_=as_, hx=hx, hs=hs, clamp=clamp)


# bfloat16 bound: relative L2 error against the float64 walk from the device's own kept output.  Between g_y and g_x the kernels
# round four times to bfloat16, each by at most 2^-9 of the value: the weights, g_u, g_t (up 2; up 1 has three) and g_x itself.
# First-order errors add, so 4 * 2^-9 bounds the relative error of every path; g_s sums products of the same rounded quantities in
# float32.  (Against the oracle's autograd a 16-bit layer cannot be held to a rounding bound: its kept output differs from the float64
# one by the forward's own rounding, and the few outputs that change sign or cross the clamp flip their whole mask - at these sizes
# a handful of elements, 2 % of the norm when it is three and 0 when it is none.  The figure is printed; the whole network's test
# holds the bfloat16 gradient against autograd, where the count is large enough for a floor to mean something.)
BF16_LAYER_BOUND = 4 * 2.0 ** -9


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("variant", ["plain", "flip", "clamp", "noise_bcast"])
@pytest.mark.parametrize("up", [1, 2])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d_%dto%d_b%d" % s)
def test_layer_vjp_against_autograd(shape, up, variant, dt):
    c = layer_case(shape, up, variant, dt)
    g_x, g_s = nchw64(c["dev"]["g_x"]), c["dev"]["g_s"]
    assert bool(torch.isfinite(g_x).all()) and bool(torch.isfinite(g_s).all())
    if variant == "clamp":
        assert 0.2 < float((c["out"].abs() >= 1.0).double().mean()) < 0.9
    if dt == "f32":
        ex, es = rel(g_x, c["ax"]), rel(g_s, c["as_"])
        print(f"f32 layer {shape} up{up} {variant}: g_x {ex:.2e} g_s {es:.2e}")
        assert ex <= F32_BOUND and es <= F32_BOUND
    else:
        ex, es = rel_l2(g_x, c["hx"]), rel_l2(g_s, c["hs"])
        print(f"bf16 layer {shape} up{up} {variant}: g_x {ex:.4f} g_s {es:.4f} of the walk from the kept output; "
              f"{rel_l2(g_x, c['ax']):.4f} / {rel_l2(g_s, c['as_']):.4f} of the oracle's autograd")
        assert ex <= BF16_LAYER_BOUND and es <= BF16_LAYER_BOUND


def test_layer_vjp_repeats_its_bits_and_skips_g_x():
    c = layer_case(SHAPES[2], 2, "plain", "bf16")
    dev, desc = c["dev"], c["desc"]
    g_x2, g_s2 = torch.empty_like(dev["g_x"]), torch.empty_like(dev["g_s"])
    L.check(L.lib().maua_modconv_vjp_ex(L.ctx(), C.byref(desc), L.ptr(dev["g_y"]), L.ptr(g_x2), L.ptr(g_s2), L.BF16))
    assert torch.equal(g_x2, dev["g_x"]) and torch.equal(g_s2, dev["g_s"])
    g_s3 = torch.empty_like(g_s2)      # g_x == NULL (the const input's layer): the styles' gradient alone, the same bits
    L.check(L.lib().maua_modconv_vjp_ex(L.ctx(), C.byref(desc), L.ptr(dev["g_y"]), None, L.ptr(g_s3), L.BF16))
    assert torch.equal(g_s3, dev["g_s"])
    assert L.lib().maua_modconv_vjp_ex(L.ctx(), C.byref(desc), L.ptr(dev["g_y"]), None, L.ptr(g_s3), L.F16) != 0
    assert "MAUA_F16 is not differentiated" in L.lib().maua_last_error().decode()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("clamp", [256.0, 1.0])
@pytest.mark.parametrize("shape", [(4, 4, 64, 1), (12, 20, 32, 2)], ids=lambda s: "%dx%d_c%d_b%d" % s)
def test_torgb_vjp_against_autograd(shape, clamp, dt):
    H, W, Cn, B = shape
    tdt = DT[dt]
    g = torch.Generator().manual_seed(H)
    x = torch.randn(B, Cn, H, W, generator=g).to(tdt).double()
    wrgb = torch.randn(3, Cn, 1, 1, generator=g)
    s = (1 + 0.5 * torch.randn(B, Cn, generator=g)) / sqrt(Cn)
    bias = torch.randn(3, generator=g)
    g_img = torch.randn(B, 3, H, W, generator=g)
    prior = torch.randn(B, Cn, H, W, generator=g).to(tdt).double()       # what the next block's conv0 left in g_x
    wmod = (wrgb[None, :, :, 0, 0] * s[:, None]).float()
    xr, sr = x.clone().requires_grad_(True), s.double().requires_grad_(True)
    y = OO.bias_act(OO.modulated_conv2d(xr, wrgb.double(), sr, demodulate=False), bias.double(), clamp=clamp)
    if clamp == 1.0:
        assert 0.05 < float((y.abs() >= 1.0).double().mean()) < 0.95
    ax, as_ = torch.autograd.grad((y * g_img.double()).sum(), (xr, sr))
    xd, g_wmod = nhwc(x, tdt), torch.empty(B, 3, Cn, device="cuda")
    wd, bd, gd = wmod.cuda(), bias.cuda(), g_img.cuda()
    for accumulate in (0, 1):
        g_x = nhwc(prior, tdt)
        L.check(L.lib().maua_torgb_vjp_ex(L.ctx(), L.ptr(xd), L.ptr(wd), L.ptr(bd), L.ptr(gd), L.ptr(g_x),
                                          L.ptr(g_wmod), B, H, W, Cn, clamp, accumulate, L.dtype_id(tdt)))
        want_x = ax + prior if accumulate else ax
        g_s = (g_wmod.double().cpu() * wrgb[None, :, :, 0, 0].double()).sum(1)
        if dt == "f32":
            assert rel(nchw64(g_x), want_x) <= F32_BOUND and rel(g_s, as_) <= F32_BOUND
        else:   # g_x is stored in bfloat16 (relative rounding error at most 2^-9 per element); the sums over exact bf16 x are f32
            assert rel_l2(nchw64(g_x), want_x) <= 2.0 ** -8 and rel(g_s, as_) <= F32_BOUND


# ---------------------------------------------------------------------------------------------------------------- the network
def device_net(p, dt, nv):
    from maua_amd.stylegan2 import SynthesisNetwork
    net = SynthesisNetwork(W_DIM, RES, 3, channel_base=CBASE, channel_max=CMAX, dtype=dt, nv_compat=nv)
    net.load_state_dict({k: v.float() for k, v in p.items()})
    return net


def oracle_grad(p, ws, noise, g_img, nv):
    wsr = ws.clone().requires_grad_(True)
    img = OS.synthesis_network(p, wsr, noise=noise, nv_compat=nv)
    (g,) = torch.autograd.grad((img * g_img).sum(), wsr)
    return g, img.detach()


@pytest.mark.parametrize("nv", [False, True], ids=["in_tree", "nv_compat"])
def test_network_vjp_f32(nv):
    p, ws, noise, g_img = make_net(5, nv=nv)
    want, img_ref = oracle_grad(p, ws, noise, g_img, nv)
    net = device_net(p, torch.float32, nv)
    net.keep_features(True)
    nz = [n.float().cuda() for n in noise]
    img = net(ws.float().cuda(), noise=nz)
    assert rel(img, img_ref) <= 2e-5
    g_ws = net.vjp(g_img.float().cuda(), noise=nz)
    err = rel(g_ws, want)
    print(f"f32 network vjp (nv_compat={nv}): {err:.2e} of the largest entry")
    assert err <= F32_BOUND
    # determinism: the same bits again; the kept forward's image is the image of the plain per-layer forward
    assert torch.equal(net.vjp(g_img.float().cuda(), noise=nz), g_ws)
    assert torch.equal(net(ws.float().cuda(), noise=nz), img)
    net.keep_features(False)
    assert rel(net(ws.float().cuda(), noise=nz), img_ref) <= 2e-5


@pytest.mark.parametrize("seed", [5, 6, 7])
def test_network_vjp_bf16(seed):
    """Measured: relative L2 0.0325 / 0.0370 / 0.0253 on the device, floors 0.0339 / 0.0289 / 0.0246, seeds 5 / 6 / 7."""
    p, ws, noise, g_img = make_net(seed)
    want, _ = oracle_grad(p, ws, noise, g_img, False)
    emu, _ = R.synthesis_vjp(p, ws, noise, g_img, rnd=R.to_bf16)
    floor = rel_l2(emu, want)
    net = device_net(p, torch.bfloat16, False)
    net.keep_features(True)
    nz = [n.float().cuda() for n in noise]
    net(ws.float().cuda(), noise=nz)
    g_ws = net.vjp(g_img.float().cuda(), noise=nz)
    err = rel_l2(g_ws, want)
    print(f"bf16 network vjp seed {seed}: relative L2 {err:.4f}, floor {floor:.4f}")
    assert 0.01 < floor < 0.06
    assert err <= 2 * floor
    assert torch.equal(net.vjp(g_img.float().cuda(), noise=nz), g_ws)


def test_network_vjp_refusals():
    p, ws, noise, g_img = make_net(5)
    net = device_net(p, torch.float32, False)
    wsd, gd = ws.float().cuda(), g_img.float().cuda()
    net(wsd)
    with pytest.raises(L.MauaHipError, match="no kept forward of this batch size"):
        net.vjp(gd)
    net.keep_features(True)
    with pytest.raises(L.MauaHipError, match="no kept forward of this batch size"):
        net.vjp(gd)
    net(wsd)
    with pytest.raises(L.MauaHipError, match="no kept forward of this batch size"):
        net.vjp(gd[:1])
    assert L.lib().maua_synth_vjp_check(net._net, 2) == 0
    L.check(L.lib().maua_synth_set_option(net._net, b"lowres", 0))
    with pytest.raises(L.MauaHipError, match="an option, a weight load or a resize came after the kept forward"):
        net.vjp(gd)
    net(wsd)
    zeros = torch.zeros(CMAX).numpy()
    L.check(L.lib().maua_synth_load(net._net, b"bs.1.conv1.bias", zeros.ctypes.data_as(C.c_void_p), zeros.size))
    with pytest.raises(L.MauaHipError, match="an option, a weight load or a resize came after the kept forward"):
        net.vjp(gd)
    net(wsd)
    minv = torch.tensor([[1.0, 0, 0, 0, 1, 0]] * 2).cuda()
    L.check(L.lib().maua_synth_set_warp(net._net, 0, 3, L.ptr(minv)))
    with pytest.raises(L.MauaHipError, match="a resize or warp hook is installed"):
        net.vjp(gd)
    L.check(L.lib().maua_synth_set_warp(net._net, 0, 3, None))
    net.set_resize(2, "stretch", (12, 12))
    with pytest.raises(L.MauaHipError, match="a resize or warp hook is installed"):
        net.vjp(torch.zeros(2, 3, *net.output_hw).cuda())
    net.set_resize(None)
    net(wsd)
    assert net.vjp(gd).shape == (2, net.num_ws, W_DIM)
    from maua_amd.noise import RawNoise
    with pytest.raises(NotImplementedError, match="RawNoise"):
        net.vjp(gd, noise=RawNoise.__new__(RawNoise))
    sc = torch.ones(net.num_layers, 2).cuda()
    L.check(L.lib().maua_synth_set_noise_scale(net._net, L.ptr(sc), 2))
    out = torch.empty(2, 3, RES, RES).cuda()
    nzl = [torch.randn(2, 1, r, r).cuda() for _, _, _, r, _ in net.layer_shapes()]
    ptrs, strides, keep = net._noise_args(nzl, 2)
    L.check(L.lib().maua_synth_render_rgb8(net._net, L.ptr(wsd), ptrs, strides, 2, L.ptr(out), None))
    with pytest.raises(L.MauaHipError, match="per-sample noise scales"):
        net.vjp(gd, noise=nzl)
    half = device_net(p, torch.float16, False)
    half.keep_features(True)
    half(wsd)
    with pytest.raises(L.MauaHipError, match="MAUA_F16 network is not differentiated"):
        half.vjp(gd)
    from maua_amd.stylegan2 import SynthesisNetwork
    with pytest.raises(NotImplementedError):
        SynthesisNetwork(W_DIM, RES, 3, channel_base=CBASE, channel_max=CMAX, architecture="resnet").vjp(gd)


# ---------------------------------------------------------------------------------------------------------------- mapper, latent_grad, Langevin
def small_generator(seed=5, nv=False):
    """a StyleGAN2-shaped generator on the small networks (the wrappers' random-init networks are 512 channels wide)"""
    from maua_amd.stylegan2 import MappingNetwork, latent_grad
    p, _, _, _ = make_net(seed, nv=nv)
    g = torch.Generator().manual_seed(seed + 1)
    mp = {k: v.double() for k, v in OS.init_mapping_params(64, 64, 8, generator=g).items()}
    mp["w_avg"] = torch.randn(64, generator=g, dtype=torch.float64)

    class Holder:
        pass

    class G:
        z_dim = 64

        def __init__(self):
            self.mapper, self.synthesizer = Holder(), Holder()
            self.mapper.G_map = MappingNetwork(64, 0, 64, 8, nv_compat=nv)
            self.mapper.G_map.load_state_dict({k: v.float() for k, v in mp.items()})
            self.synthesizer.G_synth = device_net(p, torch.float32, nv)

        def latent_grad(self, latents, grad_modules, space="z", noise=None, t=None, truncation=1.0):
            return latent_grad(self.mapper.G_map, self.synthesizer.G_synth, latents, grad_modules, space, noise, t, truncation)

        def forward(self, z):
            return self.synthesizer.G_synth(self.mapper.G_map(z))
    return G(), p, mp


@pytest.mark.parametrize("nv", [False, True])
def test_mapper_vjp(nv):
    G, _, mp = small_generator(nv=nv)
    g = torch.Generator().manual_seed(3)
    z, g_ws = torch.randn(3, 64, generator=g).double(), torch.randn(3, 8, 64, generator=g).double()
    zr = z.clone().requires_grad_(True)
    ws = OS.mapping_network(mp, zr, truncation_psi=0.7, num_ws_=8, nv_compat=nv, truncation_cutoff=4)
    (want,) = torch.autograd.grad((ws * g_ws).sum(), zr)
    M = G.mapper.G_map
    got_ws = M(z.float().cuda(), truncation_psi=0.7, truncation_cutoff=4, keep=True)
    assert rel(got_ws, ws.detach()) <= F32_BOUND
    assert rel(M.vjp(g_ws.float().cuda()), want) <= F32_BOUND
    with pytest.raises(RuntimeError, match="no kept forward"):
        type(M)(64, 0, 64, 8).vjp(g_ws.float().cuda())


class TargetGrads(GradModule):
    """loss = 1/2 |img - target|^2 summed: d loss / d img = img - target"""

    def __init__(self, target):
        super().__init__(1.0)
        self.target = target

    def forward(self, img, t):
        return img - self.target


def oracle_energy_grad(p, mp, z, target, nv=False):
    zr = z.double().cpu().requires_grad_(True)
    img = OS.synthesis_network(p, OS.mapping_network(mp, zr, num_ws_=8, nv_compat=nv), nv_compat=nv)
    e = 0.5 * (zr * zr).sum() + 0.5 * ((img - target) ** 2).sum()
    (g,) = torch.autograd.grad(e, zr)
    return g, float(e.detach())


def test_latent_grad_and_langevin():
    from maua_amd import sampling as S
    G, p, mp = small_generator()
    gen = torch.Generator().manual_seed(8)
    zt = torch.randn(2, 64, generator=gen).double()
    target = OS.synthesis_network(p, OS.mapping_network(mp, zt, num_ws_=8))
    critic = TargetGrads(target.float().cuda())
    zs = torch.randn(3, 64, generator=gen)
    # w space: the synthesis network's gradient alone
    ws = OS.mapping_network(mp, zs[:2].double(), num_ws_=8)
    wr = ws.clone().requires_grad_(True)
    (want_w,) = torch.autograd.grad(0.5 * ((OS.synthesis_network(p, wr) - target) ** 2).sum(), wr)
    g_w, img = G.latent_grad(ws.float().cuda(), critic, space="w")
    assert rel(g_w, want_w) <= F32_BOUND and tuple(img.shape) == (2, 3, RES, RES)
    with pytest.raises(ValueError, match="space must be"):
        G.latent_grad(ws.float().cuda(), critic, space="x")
    # three Langevin steps with noise: each step's gradient against the oracle AT THE DEVICE'S OWN z, the update from that gradient
    seen = []
    run = lambda seed: S.langevin_with_critic(G, zs, critic, bs=2, rate=1e-5, noise_std=1, decay=0.5, decay_steps=2, steps=3,
                                              generator=torch.Generator().manual_seed(seed),
                                              on_step=lambda i, z, g, e: seen.append((z.clone(), g.clone(), e.clone())))
    out = run(4)
    assert tuple(out.shape) == (3, 64) and len(seen) == 3 and seen[0][0].shape == (4, 64)      # padded to a multiple of bs
    assert torch.equal(seen[0][0][:3].cpu(), zs)
    sched = R.langevin_schedule(1e-5, 0.5, 2, 3)
    for i, (z, g, e) in enumerate(seen):
        for b in range(0, 4, 2):
            want, _ = oracle_energy_grad(p, mp, z[b:b + 2], target)
            assert rel(g[b:b + 2], want) <= F32_BOUND, (i, b, rel(g[b:b + 2], want))
        r, sc = sched[i]
        nxt = seen[i + 1][0] if i + 1 < len(seen) else None
        step = z.double().cpu() - 0.5 * r * g.double().cpu() + sqrt(r) * sc * e.double().cpu()
        if nxt is not None:
            assert float((nxt.double().cpu() - step).abs().max()) <= 1e-5
        else:
            assert float((out.double().cpu() - step[:3]).abs().max()) <= 1e-5
    n = len(seen)
    assert torch.equal(run(4), out) and not torch.equal(run(5), out)        # the seed decides the bits
    del seen[n:]
    # no noise, a rate at which the oracle's own energy falls on each of 5 steps: the device's falls too
    z = zs[:2].double()
    energies = []
    for _ in range(6):
        gq, e = oracle_energy_grad(p, mp, z, target)
        energies.append(e)
        z = z - 0.5 * 1e-5 * gq
    assert all(b < a for a, b in zip(energies, energies[1:])), energies
    dev_e = []
    S.langevin_with_critic(G, zs[:2], critic, bs=2, rate=1e-5, noise_std=0, decay=0, steps=6, generator=torch.Generator().manual_seed(0),
                           on_step=lambda i, z, g, e: dev_e.append(oracle_energy_grad(p, mp, z, target)[1]))
    assert all(b < a for a, b in zip(dev_e, dev_e[1:])), dev_e
    assert abs(dev_e[-1] - energies[-1]) <= 1e-3 * energies[-1]


def test_jacobian_norm_rejection():
    from maua_amd import sampling as S
    G, _, _ = small_generator()
    zs = torch.randn(3, 64, generator=torch.Generator().manual_seed(2))
    kept = S.jacobian_norm_rejection(G, zs, ratio=0.7)
    # ceil(3 / 0.7) = 5 candidates (the three latents and two draws seeded from them), ceil(0.7 * 5) = 4 kept
    assert tuple(kept.shape) == (4, 64)
    import numpy as np
    extra = torch.from_numpy(np.random.RandomState(S.latents_seed(zs)).randn(3, 64)[1:]).float()
    cands = torch.cat((zs, extra))
    rows = [int((cands == k.cpu()).all(1).nonzero()) for k in kept]
    assert len(set(rows)) == 4
    assert torch.equal(S.jacobian_norm_rejection(G, zs, ratio=0.7), kept)       # seeded from the latents: the same choice again
    assert torch.equal(S.jacobian_norm_rejection(G, zs, ratio=1.0).cpu().sort(0).values, zs.sort(0).values)   # nothing drawn, nothing dropped


# ---------------------------------------------------------------------------------------------------------------- command line
def test_generate_images_cli(tmp_path):
    import gzip
    from maua_amd import sampling as S
    from test_gpu_clip_text import MERGES
    out = tmp_path / "out"
    torch.manual_seed(0)
    written = S.main(["--model_file", "None", "--seeds", "1,2,4-6", "--out_size", "32,32", "--batch_size", "2", "--out_dir", str(out)])
    assert sorted(p.name for p in out.iterdir()) == ["seed1_None.png", "seed2_None.png", "seed4_None.png", "seed5_None.png"]
    assert [p.name for p in written] == ["seed1_None.png", "seed2_None.png", "seed4_None.png", "seed5_None.png"]
    from PIL import Image
    assert Image.open(written[0]).size == (32, 32)
    grid = S.main(["--model_file", "None", "--seeds", "1,2,4-6", "--out_size", "32,32", "--batch_size", "4", "--grid", "--out_dir", str(out)])
    assert Image.open(grid[0]).size == (3 * 32, 2 * 32) and grid[0].name == "seeds1,2,4-6_None.png"
    with pytest.raises(NotImplementedError, match="discriminator"):
        S.main(["--model_file", "None", "--seeds", "1", "--out_size", "32,32", "--latent_sampling", "langevin", "--out_dir", str(out)])
    with pytest.raises(NotImplementedError):
        S.main(["--model_file", "None", "--seeds", "1", "--out_size", "32,32", "--latent_sampling", "polarity", "--out_dir", str(out)])
    # one Langevin step against a text prompt on a random-init ViT-B/32
    vocab = tmp_path / "merges.txt.gz"
    vocab.write_bytes(gzip.compress(("#version: synthetic\n" + "\n".join(MERGES) + "\n").encode()))
    lg = S.main(["--model_file", "None", "--seeds", "3", "--out_size", "32,32", "--batch_size", "1", "--latent_sampling", "langevin",
                 "--langevin_critic", "hello the city", "--langevin_steps", "1", "--allow_random_init", "--bpe_path", str(vocab),
                 "--out_dir", str(out)])
    assert lg[0].name == "seed3_None_langevin:hello the city.png" and Image.open(lg[0]).size == (32, 32)
