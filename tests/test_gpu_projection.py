"""On the device: the gradient to the noise inputs (maua_synth_vjp_ex), the projection kernels of csrc/project.hip and the loop of
maua_amd/projection.py, stage by stage.

Method (as the "pin" tests): every output the C entries write sits between guard regions that must stay intact, with every element
written; reruns give the same bits; the kernels of project.hip are held to the float32 restatements of tests/projection_ref.py TO THE
BIT and to the float64 formulae inside the bounds that module derives from operation counts - bounds that
tests/test_projection_host.py proves for the restatements on these very inputs.  The noise gradient is held to the float64 autograd of
the oracle: float32 networks within 4e-5 of the largest entry (the bound of the walk it rides in, tests/test_gpu_synth_vjp.py),
bfloat16 networks within twice the floor of the bfloat16-emulated walk."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cabi_guard as G  # noqa: E402
import projection_ref as PR  # noqa: E402
import synth_vjp_ref as R  # noqa: E402
from test_projection_host import F32_BOUND, NOISE_CASES, NOISE_SEEDS, net96, noise_case, self_projection_inputs  # noqa: E402
from test_synth_vjp_host import B, CBASE, CMAX, RES, W_DIM, make_net  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from maua_amd import projection as P  # noqa: E402
from maua_amd.grad import GradModule  # noqa: E402
from oracle import stylegan2 as OS  # noqa: E402

pytestmark = pytest.mark.gpu
f32 = np.float32


def rel(a, b):
    return float((a.double().cpu() - b).abs().max() / b.abs().max())


def device_net(p, dt, nv=False, res=RES, cbase=CBASE, cmax=CMAX):
    from maua_amd.stylegan2 import SynthesisNetwork
    net = SynthesisNetwork(W_DIM, res, 3, channel_base=cbase, channel_max=cmax, dtype=dt, nv_compat=nv)
    net.load_state_dict({k: v.float() for k, v in p.items()})
    net.keep_features(True)
    return net


def to_dev(noise):
    return None if noise is None else [None if n is None else n.float().cuda() for n in noise]


# ---------------------------------------------------------------------------------------------------------------- noise gradient
@functools.lru_cache(maxsize=None)
def noise_reference(case, nv, seed=None):
    p, ws, noise, g_img = make_net(NOISE_SEEDS[case, nv] if seed is None else seed, nv=nv)
    nz = noise_case(p, noise, case)
    want_ws, want, _ = PR.autograd_noise(p, ws, nz, g_img, nv)
    return p, ws, nz, g_img, want_ws, want


def guarded_noise_grads(net, nz, Bn):
    bufs = []
    for l in range(net.num_layers):
        h, w = net.layer_size(l)
        nb = Bn if nz is not None and nz[l] is not None and nz[l].shape[0] == Bn and Bn > 1 else 1
        bufs.append((G.Buf(nb * h * w), (nb, 1, h, w)))
    return bufs, [b.full[G.G:G.G + b.n].view(shape) for b, shape in bufs]


def run_noise_grad(net, ws, nz, g_img):
    """the plain walk, then the walk with guarded noise-gradient buffers: g_ws must have the same bits; the buffers are checked"""
    Bn = ws.shape[0]
    wsd, gd, nzd = ws.float().cuda(), g_img.float().cuda(), to_dev(nz)
    net(wsd, noise=nzd)
    plain = net.vjp(gd, noise=nzd)
    bufs, views = guarded_noise_grads(net, nz, Bn)
    g_ws, g_noise = net.vjp(gd, noise=nzd, noise_grad=views)
    torch.cuda.synchronize()
    assert torch.equal(g_ws, plain), "g_ws differs from maua_synth_vjp's"
    for l, (b, _) in enumerate(bufs):
        b.check(f"g_noise[{l}]")
    # again: the same bits; and with one entry not wanted, the others unchanged and nothing written for it
    bufs2, views2 = guarded_noise_grads(net, nz, Bn)
    skip = 1
    views2[skip] = None
    g_ws2, g_noise2 = net.vjp(gd, noise=nzd, noise_grad=views2)
    torch.cuda.synchronize()
    assert torch.equal(g_ws2, plain) and g_noise2[skip] is None and bufs2[skip][0].untouched()
    assert all(torch.equal(a, b) for l, (a, b) in enumerate(zip(g_noise, g_noise2)) if l != skip)
    assert torch.equal(net.vjp(gd, noise=nzd), plain)
    return g_ws, g_noise


@pytest.mark.parametrize("nv", [False, True], ids=["in_tree", "nv_compat"])
@pytest.mark.parametrize("case", NOISE_CASES)
def test_noise_gradient_f32(case, nv):
    p, ws, nz, g_img, want_ws, want = noise_reference(case, nv)
    net = device_net(p, torch.float32, nv)
    g_ws, g_noise = run_noise_grad(net, ws, nz, g_img)
    assert rel(g_ws, want_ws) <= F32_BOUND
    errs = [rel(a, b) for a, b in zip(g_noise, want)]
    print(f"f32 noise gradient, {case}, nv_compat={nv}: per layer {' '.join(f'{e:.1e}' for e in errs)}")
    for l, (a, b) in enumerate(zip(g_noise, want)):
        assert tuple(a.shape) == tuple(b.shape), l
    assert max(errs) <= F32_BOUND


@pytest.mark.parametrize("case", ["per_sample", "mixed"])
def test_noise_gradient_bf16(case):
    p, ws, nz, g_img, want_ws, want = noise_reference(case, False, 5)
    _, emu, _ = PR.synthesis_vjp_noise(p, ws, nz, g_img, rnd=R.to_bf16)
    flat = lambda gs: torch.cat([g.double().cpu().reshape(-1) for g in gs])
    floor = float((flat(emu) - flat(want)).norm() / flat(want).norm())
    net = device_net(p, torch.bfloat16)
    _, g_noise = run_noise_grad(net, ws, nz, g_img)
    err = float((flat(g_noise) - flat(want)).norm() / flat(want).norm())
    print(f"bf16 noise gradient, {case}: relative L2 {err:.4f}, floor {floor:.4f}")
    assert 0.002 < floor < 0.06
    assert err <= 2 * floor


@pytest.mark.parametrize("shared", [False, True], ids=["per_sample", "shared"])
def test_noise_gradient_three_channel_groups(shared):
    p, ws, noise, g_img = net96()
    nz = [n[:1] for n in noise] if shared else noise
    _, want, _ = PR.autograd_noise(p, ws, nz, g_img)
    net = device_net(p, torch.float32, res=8, cbase=1024, cmax=96)
    assert all(co == 96 for _, _, co, _, _ in net.layer_shapes())
    _, g_noise = run_noise_grad(net, ws, nz, g_img)
    errs = [rel(a, b) for a, b in zip(g_noise, want)]
    print(f"f32 noise gradient, Co = 96 (three groups), shared={shared}: {' '.join(f'{e:.1e}' for e in errs)}")
    assert max(errs) <= F32_BOUND


# ---------------------------------------------------------------------------------------------------------------- regulariser
def workspace(nbytes):
    return G.Buf(max(int(nbytes), 256), torch.uint8)


@pytest.mark.parametrize("case", PR.REG_CASES, ids=lambda c: "%d_b%d_%s" % c)
def test_noise_regulariser(case):
    R_, Bn, kind = case
    n, prior = PR.reg_input(R_, Bn, kind)
    weight = 1e5 if kind == "planted" else 3.0
    lib = L.lib()
    nbytes = lib.maua_noise_reg_workspace_bytes(Bn, R_)
    assert nbytes > 0 and lib.maua_noise_reg_levels(R_) == PR.reg_levels(R_)
    nb, ws = G.inp(n.numpy()), workspace(nbytes)
    loss, grad = G.Buf(Bn), G.Buf(n.numel())
    G.call("maua_noise_reg", nb.ptr, Bn, R_, weight, loss.ptr, grad.ptr, 0, ws.ptr, nbytes)
    for b, what in ((loss, "loss"), (grad, "grad"), (nb, "maps")):
        b.check(what)
    ws.check("workspace", written=False)
    loss32, grad32 = PR.noise_reg_f32(n.numpy(), weight)
    assert G.same(loss.get(), loss32) and G.same(grad.get().reshape(grad32.shape), grad32), "not the restatement's bits"
    loss64, grad64 = PR.noise_reg_f64(n, weight)
    loss_b, grad_b = PR.noise_reg_bound(n, weight)
    rl = G.ratio(loss.get(), loss64.numpy(), loss_b.numpy())
    rg = G.ratio(grad.get().reshape(grad32.shape), grad64.numpy(), grad_b.numpy())
    print(f"regulariser {case}: loss error / bound {rl:.3f}, gradient error / bound {rg:.3f}")
    assert rl <= 1 and rg <= 1
    # again without the loss: the same bits; accumulating onto what the buffer holds; another weight
    grad2 = G.Buf(n.numel())
    G.call("maua_noise_reg", nb.ptr, Bn, R_, weight, None, grad2.ptr, 0, ws.ptr, nbytes)
    grad2.check("grad, rerun")
    assert G.same(grad2.get(), grad.get())
    acc = G.inp(prior.numpy(), guard=0.0)
    G.call("maua_noise_reg", nb.ptr, Bn, R_, weight, loss.ptr, acc.ptr, 1, ws.ptr, nbytes)
    acc.check("grad, accumulated")
    _, acc32 = PR.noise_reg_f32(n.numpy(), weight, grad_in=prior.numpy())
    assert G.same(acc.get().reshape(acc32.shape), acc32)
    if R_ <= 64:
        _, acc_b = PR.noise_reg_bound(n, weight, grad_in=prior)
        assert G.ratio(acc.get().reshape(acc32.shape), (prior.double() + grad64).numpy(), acc_b.numpy()) <= 1
        other = G.Buf(n.numel())
        G.call("maua_noise_reg", nb.ptr, Bn, R_, 0.5 * weight, None, other.ptr, 0, ws.ptr, nbytes)
        assert G.same(other.get().reshape(grad32.shape), PR.noise_reg_f32(n.numpy(), 0.5 * weight)[1])
    G.refused("maua_noise_reg", nb.ptr, Bn, 12, weight, loss.ptr, grad.ptr, 0, ws.ptr, nbytes)


# ---------------------------------------------------------------------------------------------------------------- Adam, renorm, expand
@pytest.mark.parametrize("n", PR.ADAM_SIZES)
def test_adam_step_bits(n):
    p, m, v, gs = PR.adam_input(n)
    pb, mb, vb = G.inp(p, guard=0.0), G.inp(m, guard=0.0), G.inp(v, guard=0.0)
    p64, m64, v64 = (a.astype(np.float64) for a in (p, m, v))
    dp = dm = dv = 0.0
    for s, (g, lr) in enumerate(zip(gs, PR.adam_lrs())):
        sc = PR.adam_scalars_f32(lr, s + 1)
        step, inv = P.adam_scalars(lr, s + 1)
        assert (f32(step), f32(inv)) == (sc[3], sc[4])
        gb = G.inp(g)
        G.call("maua_adam_step", pb.ptr, gb.ptr, mb.ptr, vb.ptr, n, 0.9, 0.999, 1e-8, step, inv)
        dp, dm, dv = PR.adam_bound(p64, g, m64, v64, sc, dp, dm, dv)
        p64, m64, v64 = PR.adam_f64(p64, g, m64, v64, sc)
        p, m, v = PR.adam_f32(p, g, m, v, sc)
        for b, want, w64, d, what in ((pb, p, p64, dp, "param"), (mb, m, m64, dm, "m"), (vb, v, v64, dv, "v")):
            b.check(what)
            assert G.same(b.get(), want), f"step {s}: {what} is not the restatement's bits"
            assert bool((np.abs(b.get().astype(np.float64) - w64) <= d).all())
    assert np.isfinite(pb.get()).all()


@pytest.mark.parametrize("shape", [(3, 16), (2, 4096 + 17), (1, 65541), (2, 1 << 20)], ids=lambda s: "%dx%d" % s)
def test_noise_renorm_bits(shape):
    maps, N = shape
    g = torch.Generator().manual_seed(N)
    n = (torch.randn(maps, N, generator=g) * 2 + 0.7).numpy()
    nbytes = L.lib().maua_noise_renorm_workspace_bytes(maps, N)
    ws = workspace(nbytes)
    outs = []
    for _ in range(2):
        b = G.inp(n, guard=0.0)
        G.call("maua_noise_renorm", b.ptr, maps, N, ws.ptr, nbytes)
        b.check("maps")
        outs.append(b.get().reshape(maps, N))
    ws.check("workspace", written=False)
    assert G.same(outs[0], outs[1]) and G.same(outs[0], PR.renorm_f32(n))
    assert abs(float(outs[0].astype(np.float64).mean())) < 1e-5 and abs(float((outs[0].astype(np.float64) ** 2).mean()) - 1) < 1e-5
    if maps == 3:    # a constant map: 0 x inf, as published - not special-cased
        c = np.stack([n[0], np.full(N, 3.0, f32), n[2]])
        b = G.inp(c, guard=0.0)
        G.call("maua_noise_renorm", b.ptr, maps, N, ws.ptr, nbytes)
        got = b.get().reshape(maps, N)
        assert G.same(got, PR.renorm_f32(c)) and np.isnan(got[1]).all() and np.isfinite(got[0]).all()


@pytest.mark.parametrize("rows", [1, 8], ids=["w", "w_plus"])
@pytest.mark.parametrize("with_eps", [False, True])
def test_latent_expand_and_reduce_bits(rows, with_eps):
    Bn, num_ws, w_dim = 3, 8, 67
    g = torch.Generator().manual_seed(rows)
    w, eps = torch.randn(Bn, rows, w_dim, generator=g).numpy(), torch.randn(Bn, rows, w_dim, generator=g).numpy()
    wb, eb, out = G.inp(w), G.inp(eps), G.Buf(Bn * num_ws * w_dim)
    scale = 0.0371
    G.call("maua_latent_expand", wb.ptr, rows, eb.ptr if with_eps else None, scale, out.ptr, Bn, num_ws, w_dim)
    out.check("ws")
    assert G.same(out.get().reshape(Bn, num_ws, w_dim), PR.expand_f32(w, eps if with_eps else None, scale, num_ws))
    g_ws = torch.randn(Bn, num_ws, w_dim, generator=g).numpy()
    gb, red = G.inp(g_ws), G.Buf(Bn * w_dim)
    G.call("maua_latent_reduce", gb.ptr, red.ptr, Bn, num_ws, w_dim)
    red.check("g_w")
    assert G.same(red.get().reshape(Bn, w_dim), PR.reduce_f32(g_ws))
    G.refused("maua_latent_expand", wb.ptr, 3, None, scale, out.ptr, Bn, num_ws, w_dim)


# ---------------------------------------------------------------------------------------------------------------- the loop
class HalfSquaredError(GradModule):
    """1/2 sum (img - target)^2: the gradient is img - target (a test's module: torch arithmetic is fine here)"""

    def __init__(self, target):
        super().__init__(1)
        self.target = target.float().cuda()

    def forward(self, img, t, return_loss=False):
        g = img - self.target
        return (g, 0.5 * (g * g).sum((1, 2, 3))) if return_loss else g


def small_generator(p, mp, dt=torch.float32):
    from maua_amd.stylegan2 import MappingNetwork

    class Holder:
        pass

    class Gen:
        def __init__(self):
            self.mapper, self.synthesizer = Holder(), Holder()
            self.mapper.G_map = MappingNetwork(64, 0, 64, OS.num_ws(RES), num_layers=2)
            self.mapper.G_map.load_state_dict({k: v.float() for k, v in mp.items()})
            self.synthesizer.G_synth = device_net(p, dt)
            self.synthesizer.G_synth.keep_features(False)

    return Gen()


def cpu(x):
    return [cpu(t) for t in x] if isinstance(x, (list, tuple)) else (x.detach().cpu().clone() if isinstance(x, torch.Tensor) else x)


@pytest.mark.parametrize("space", ["w", "w+"])
def test_loop_stage_by_stage(space):
    p, mp, target = self_projection_inputs()
    gen = small_generator(p, mp)
    seen = []
    steps, weight, num_ws = 5, 1e5, OS.num_ws(RES)
    out = P.project(gen, targets=target.float(), grad_modules=[HalfSquaredError(target)], space=space, num_steps=steps, w_avg_samples=1000,
                    regularize_noise_weight=weight, seed=3, on_step=lambda i, s: seen.append({k: cpu(v) for k, v in s.items()}))
    assert len(seen) == steps and [s["step"] for s in seen] == list(range(steps))
    w_avg, w_std = PR.w_statistics_f64(mp, 1000)
    rows = 1 if space == "w" else num_ws
    assert seen[0]["w"].shape == (B, rows, 64) and rel(seen[0]["w"], w_avg[None, None].expand(B, rows, -1)) <= 1e-4
    for i, s in enumerate(seen):
        # the schedule: the host formulae at the run's own w_std
        assert abs(s["w_std"] - w_std) <= 1e-4 * w_std
        lr, scale = PR.schedule_f64(i, steps, s["w_std"])
        assert s["lr"] == pytest.approx(lr, rel=1e-14) and s["w_noise_scale"] == pytest.approx(scale, rel=1e-14)
        # expansion: the restatement's bits from the device's own w and eps
        assert G.same(s["ws"].numpy(), PR.expand_f32(s["w"].numpy(), s["eps"].numpy(), s["w_noise_scale"], num_ws))
        # gradients: float64 autograd at the device's own w and maps of this step
        nz = [n.double() for n in s["noise"]]
        wr = s["w"].double().clone().requires_grad_(True)
        nr = [n.clone().requires_grad_(True) for n in nz]
        wn = wr + s["w_noise_scale"] * s["eps"].double()
        img = OS.synthesis_network(p, wn.expand(-1, num_ws, -1) if rows == 1 else wn, noise=nr)
        grads = torch.autograd.grad(0.5 * ((img - target) ** 2).sum(), [wr] + nr)
        assert rel(s["img"], img.detach()) <= 2e-5
        assert rel(s["g_w"], grads[0]) <= F32_BOUND, i
        for l, (n, g_net) in enumerate(zip(nz, grads[1:])):
            loss64, reg64 = PR.noise_reg_f64(n[:, 0], weight)
            loss_b, reg_b = PR.noise_reg_bound(n[:, 0], weight, grad_in=g_net[:, 0])
            assert bool(((s["reg_loss"][l].double() - loss64).abs() <= loss_b).all()), (i, l)
            bound = F32_BOUND * g_net.abs().max() + reg_b
            assert bool(((s["g_noise"][l][:, 0].double() - (g_net[:, 0] + reg64)).abs() <= bound).all()), (i, l)
        # the update: the restatement's Adam and renorm applied to the device's own gradients give the next step's state, to the bit
        sc = PR.adam_scalars_f32(s["lr"], i + 1)
        nxt = seen[i + 1] if i + 1 < steps else None
        w2, m2, v2 = PR.adam_f32(s["w"].numpy(), s["g_w"].numpy(), s["m_w"].numpy(), s["v_w"].numpy(), sc)
        if nxt is not None:
            assert G.same(nxt["w"].numpy(), w2) and G.same(nxt["m_w"].numpy(), m2) and G.same(nxt["v_w"].numpy(), v2), i
        else:
            assert G.same(out.ws.cpu().numpy(), PR.expand_f32(w2, None, 0.0, num_ws))
        for l in range(len(nz)):
            n2, mn2, vn2 = PR.adam_f32(s["noise"][l].numpy(), s["g_noise"][l].numpy(), s["m_noise"][l].numpy(), s["v_noise"][l].numpy(), sc)
            n2 = PR.renorm_f32(n2.reshape(B, -1)).reshape(n2.shape)
            after = nxt["noise"][l] if nxt is not None else out.noise[l].cpu()
            assert G.same(after.numpy(), n2), (i, l)
            if nxt is not None:
                assert G.same(nxt["m_noise"][l].numpy(), mn2) and G.same(nxt["v_noise"][l].numpy(), vn2), (i, l)
    assert out.losses["noise_reg"].shape == (steps, B) and out.losses["HalfSquaredError0"].shape == (steps, B)


def test_it_projects():
    """The float64 restatement of this run ends at 0.038 of the initial distance (tests/test_projection_host.py holds it to 0.05)."""
    p, mp, target = self_projection_inputs()
    gen = small_generator(p, mp)
    out = P.project(gen, targets=target.float(), grad_modules=[HalfSquaredError(target)], space="w", num_steps=100, w_avg_samples=1000)
    first = float(out.losses["HalfSquaredError0"][0].sum())
    img = gen.synthesizer.G_synth(out.ws, noise=out.noise)
    final = float(0.5 * ((img.double().cpu() - target) ** 2).sum())
    print(f"self-projection: distance {first:.1f} -> {final:.1f} (ratio {final / first:.4f})")
    assert final <= 0.10 * first
    assert out.ws.shape == (B, OS.num_ws(RES), 64) and bool((out.ws[:, 0] == out.ws[:, 5]).all())
