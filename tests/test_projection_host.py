"""Without a device: the references and bounds of tests/projection_ref.py proved on the inputs the device tests use (the float32
restatements against the float64 formulae, inside the bounds derived from operation counts - the device tests then hold the device to
the restatements' bits and to the same bounds), the float64 projection loop, and the plumbing of maua_amd.projection and
maua_amd.parameterizations (save / load, command line, refusals by name, the running average)."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import projection_ref as PR  # noqa: E402
import synth_vjp_ref as R  # noqa: E402
from test_synth_vjp_host import B, make_net  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from maua_amd import parameterizations as PZ, projection as P  # noqa: E402
from oracle import stylegan2 as OS  # noqa: E402

F32_BOUND = 4e-5    # tests/test_gpu_synth_vjp.py test_network_vjp_f32: of the largest reference entry


def rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


# ---------------------------------------------------------------------------------------------------------------- noise gradient
def noise_case(p, noise, case):
    """the noise list of a case: per-sample maps, one shared map per layer, the layers' noise_const, or a mix"""
    if case == "per_sample":
        return noise
    if case == "shared":
        return [n[:1] for n in noise]
    if case == "const":
        return None
    return [n if l % 3 == 0 else (n[:1] if l % 3 == 1 else None) for l, n in enumerate(noise)]   # "mixed"


NOISE_CASES = ["per_sample", "shared", "const", "mixed"]
# The network is piecewise linear: a feature that the float32 forward leaves on the other side of zero than float64 does flips its
# lrelu slope, and the comparison then reports the FORWARD's rounding as a gradient error of percents (seed 5 with noise_const has a
# feature of 5.6e-7 in its 8 x 8 up-layer, and the device's g_ws - the established walk's - is then 1.3e-2 of its largest entry off).  So every case runs on the
# first seed (from 5 up) whose features all lie at least KINK_MARGIN from zero, and LOW_KINK_MARGIN in the three <= 8 x 8 layers, where
# one element reaches every later pixel.  The margins are set against the forward, not the gradient under test: its float32 features
# differ from float64 by about 1e-6 (2e-5 of the largest is the bound tests/test_gpu_synth.py holds them to; 65536 elements of unit
# scale cannot all keep that distance, so the margin is the attainable one).  test_noise_gradient_walk_matches_autograd asserts them.
KINK_MARGIN, LOW_KINK_MARGIN = 5e-6, 2e-5
NOISE_SEEDS = {("per_sample", False): 7, ("shared", False): 7, ("const", False): 9, ("mixed", False): 5,
               ("per_sample", True): 5, ("shared", True): 5, ("const", True): 5, ("mixed", True): 6}


def net96(seed=8):
    """two resolutions, three layers, every one with Co = 96: three 32-channel groups"""
    g = torch.Generator().manual_seed(seed)
    p = {k: v.double() for k, v in OS.init_synthesis_params(8, 64, 3, 1024, 96, generator=g).items()}
    ws = torch.randn(B, OS.num_ws(8), 64, generator=g).double()
    noise = [torch.randn(B, 1, r, r, generator=g).double() for _, _, _, r, _ in OS.layer_list(8, 1024, 96)]
    g_img = torch.randn(B, 3, 8, 8, generator=g).double()
    return p, ws, noise, g_img


@pytest.mark.parametrize("nv", [False, True], ids=["in_tree", "nv_compat"])
@pytest.mark.parametrize("case", NOISE_CASES)
def test_noise_gradient_walk_matches_autograd(case, nv):
    p, ws, noise, g_img = make_net(NOISE_SEEDS[case, nv], nv=nv)
    nz = noise_case(p, noise, case)
    feats = OS.synthesis_network(p, ws, noise=nz, nv_compat=nv, return_features=True)[1]
    away = [float(f.abs().min()) for f in feats]
    assert min(away) >= KINK_MARGIN and min(away[:3]) >= LOW_KINK_MARGIN, away
    want_ws, want, _ = PR.autograd_noise(p, ws, nz, g_img, nv)
    g_ws, g_noise, _ = PR.synthesis_vjp_noise(p, ws, nz, g_img, nv)
    assert rel(g_ws, want_ws) <= 1e-10
    for l, (a, b) in enumerate(zip(g_noise, want)):
        assert a.shape == b.shape, (l, a.shape, b.shape)
        assert rel(a, b) <= 1e-10, l
    if nv:   # the strengths are not 1: the case means something
        assert all(abs(float(v) - 1) > 0.01 for k, v in p.items() if k.endswith("noise_strength"))
    # the float32 hand-walk sits inside the bound the device is held to
    f = lambda t: None if t is None else t.float()
    _, g32, _ = PR.synthesis_vjp_noise({k: v.float() for k, v in p.items()}, ws.float(), None if nz is None else [f(n) for n in nz],
                                       g_img.float(), nv)
    errs = [rel(a, b) for a, b in zip(g32, want)]
    print(f"float32 hand-walk, {case}, nv_compat={nv}: worst layer {max(errs):.2e} of its largest entry")
    assert max(errs) <= F32_BOUND


def test_noise_gradient_walk_three_groups():
    p, ws, noise, g_img = net96()
    assert all(co == 96 for _, _, co, _, _ in OS.layer_list(8, 1024, 96))
    for nz in (noise, [n[:1] for n in noise]):
        assert min(float(f.abs().min()) for f in OS.synthesis_network(p, ws, noise=nz, return_features=True)[1]) >= LOW_KINK_MARGIN
    _, want, _ = PR.autograd_noise(p, ws, noise, g_img)
    _, g_noise, _ = PR.synthesis_vjp_noise(p, ws, noise, g_img)
    assert max(rel(a, b) for a, b in zip(g_noise, want)) <= 1e-10
    _, g32, _ = PR.synthesis_vjp_noise({k: v.float() for k, v in p.items()}, ws.float(), [n.float() for n in noise], g_img.float())
    assert max(rel(a, b) for a, b in zip(g32, want)) <= F32_BOUND


# ---------------------------------------------------------------------------------------------------------------- regulariser
@pytest.mark.parametrize("case", PR.REG_CASES, ids=lambda c: "%d_b%d_%s" % c)
def test_regulariser_restatement_inside_its_bound(case):
    R_, Bn, kind = case
    n, prior = PR.reg_input(R_, Bn, kind)
    weight = 1e5 if kind == "planted" else 3.0
    loss64, grad64 = PR.noise_reg_f64(n, weight)
    loss_b, grad_b = PR.noise_reg_bound(n, weight)
    loss32, grad32 = PR.noise_reg_f32(n.numpy(), weight)
    el = (torch.from_numpy(loss32).double() - loss64).abs()
    eg = (torch.from_numpy(grad32).double() - grad64).abs()
    print(f"regulariser {case}: loss {float(loss64.max()):.3e}, error / bound {float((el / loss_b).max()):.3f}; "
          f"gradient error / bound {float((eg / grad_b).max()):.3f}")
    assert bool((el <= loss_b).all()) and bool((eg <= grad_b).all())
    assert PR.reg_levels(R_) == {4: 1, 8: 1, 16: 2, 64: 4, 1024: 8}[R_]
    if kind == "planted":   # every level's means are far from zero: the gradient is not noise
        assert float(loss64.min()) > 1.0
    if R_ <= 64:
        _, acc32 = PR.noise_reg_f32(n.numpy(), weight, grad_in=prior.numpy())
        _, acc_b = PR.noise_reg_bound(n, weight, grad_in=prior)
        assert bool(((torch.from_numpy(acc32).double() - (prior.double() + grad64)).abs() <= acc_b).all())


def test_regulariser_and_other_refusals_without_a_device():
    lib, one = L.lib(), 4096
    msg = lambda rc: (rc != 0) and lib.maua_last_error().decode()
    big = 1 << 40
    ok = lambda R_: lib.maua_noise_reg_check(one, 2, R_, one, one, one, big)
    assert ok(4) == 0 and ok(8) == 0 and ok(1024) == 0
    for bad in (12, 2, 0, 3, 32768):
        assert "power of two, at least 4" in msg(ok(bad)), bad
    assert lib.maua_noise_reg_workspace_bytes(2, 12) == 0 and lib.maua_noise_reg_levels(12) == 0
    assert [lib.maua_noise_reg_levels(r) for r in (4, 8, 16, 64, 1024)] == [1, 1, 2, 4, 8]
    assert "neither loss nor grad" in msg(lib.maua_noise_reg_check(one, 2, 8, None, None, one, big))
    assert "workspace" in msg(lib.maua_noise_reg_check(one, 2, 64, one, one, one, lib.maua_noise_reg_workspace_bytes(2, 64) - 1))
    assert "256-byte aligned" in msg(lib.maua_noise_reg_check(one, 2, 64, one, one, one + 4, big))
    assert lib.maua_noise_reg_check(one, 2, 64, one, one, one, lib.maua_noise_reg_workspace_bytes(2, 64)) == 0
    assert "ctx is NULL" in msg(lib.maua_noise_reg(None, one, 2, 8, 1.0, one, one, 0, one, big))
    adam = lambda **kw: lib.maua_adam_step_check(*{**dict(p=one, g=one, m=one, v=one, n=5, b1=0.9, b2=0.999, eps=1e-8), **kw}.values())
    assert adam() == 0 and adam(n=0, p=None) == 0
    assert "NULL argument" in msg(adam(v=None)) and "betas" in msg(adam(b1=1.0)) and "eps" in msg(adam(eps=-1.0))
    assert "bad element count" in msg(adam(n=-1))
    assert lib.maua_noise_renorm_check(one, 3, 16, one, big) == 0
    assert "between 1 and 2^31" in msg(lib.maua_noise_renorm_check(one, 3, 0, one, big))
    assert "workspace" in msg(lib.maua_noise_renorm_check(one, 3, 1 << 20, one, lib.maua_noise_renorm_workspace_bytes(3, 1 << 20) - 1))
    assert lib.maua_latent_expand_check(one, 1, None, one, 2, 8, 64) == 0 and lib.maua_latent_expand_check(one, 8, one, one, 2, 8, 64) == 0
    assert "one row (space w) or num_ws rows" in msg(lib.maua_latent_expand_check(one, 3, None, one, 2, 8, 64))
    assert "NULL argument" in msg(lib.maua_latent_expand_check(None, 1, None, one, 2, 8, 64))
    assert lib.maua_latent_reduce_check(one, one, 2, 8, 64) == 0
    assert "bad shape" in msg(lib.maua_latent_reduce_check(one, one, 2, 0, 64))
    assert "net is NULL" in msg(lib.maua_synth_vjp_ex(None, None, None, 2, None, None, None, None))


# ---------------------------------------------------------------------------------------------------------------- Adam, renorm, expand
@pytest.mark.parametrize("n", PR.ADAM_SIZES)
def test_adam_restatement_inside_its_bound_and_near_torch(n):
    p, m, v, gs = PR.adam_input(n)
    assert any((g == 0).any() for g in gs) and any(((g != 0) & (np.abs(g) < 1.17e-38)).any() for g in gs)
    p32, m32, v32 = p, m, v
    p64, m64, v64 = (a.astype(np.float64) for a in (p, m, v))
    dp = dm = dv = 0.0
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=0.1, betas=(0.9, 0.999), eps=1e-8)
    worst = 0.0
    for s, (g, lr) in enumerate(zip(gs, PR.adam_lrs())):
        sc = PR.adam_scalars_f32(lr, s + 1)
        dp, dm, dv = PR.adam_bound(p64, g, m64, v64, sc, dp, dm, dv)
        p64, m64, v64 = PR.adam_f64(p64, g, m64, v64, sc)
        p32, m32, v32 = PR.adam_f32(p32, g, m32, v32, sc)
        for a32, a64, d in ((p32, p64, dp), (m32, m64, dm), (v32, v64, dv)):
            assert a32.dtype == np.float32 and bool((np.abs(a32.astype(np.float64) - a64) <= d).all()), s
        opt.param_groups[0]["lr"] = lr
        tp.grad = torch.from_numpy(g.copy())
        opt.step()
        worst = max(worst, float(np.abs(tp.detach().numpy().astype(np.float64) - p32).max()))
    assert np.isfinite(p32).all()
    print(f"Adam n = {n}: after 3 steps the restatement and torch.optim.Adam (CPU, float32) differ by at most {worst:.3e} "
          f"(bound to float64: {float(np.max(dp)):.3e})")
    assert worst <= 1e-5      # (the same update; not held to the bit: torch fuses and orders its operations differently)


def test_renorm_and_expand_restatements():
    g = torch.Generator().manual_seed(2)
    for N in (16, 1024, 65541):
        n = (torch.randn(3, N, generator=g) * 2 + 0.7).numpy()
        out = PR.renorm_f32(n)
        d = n.astype(np.float64)
        d = d - d.mean(1, keepdims=True)
        d = d / np.sqrt((d * d).mean(1, keepdims=True))
        assert np.abs(out - d).max() <= 1e-5
        assert np.abs(PR.red_sum_f32(n) - n.astype(np.float64).sum(1)).max() <= PR.red_depth(N) * PR.V * np.abs(n).sum(1).max()
    const = PR.renorm_f32(np.full((1, 64), 3.0, np.float32))
    assert np.isnan(const).all()      # 0 x inf, as the published buf *= buf.square().mean().rsqrt() gives
    w, eps = torch.randn(2, 1, 8, generator=g).numpy(), torch.randn(2, 1, 8, generator=g).numpy()
    ws = PR.expand_f32(w, eps, 0.3, 5)
    assert ws.shape == (2, 5, 8) and np.array_equal(ws[:, 3], (w + np.float32(0.3) * eps)[:, 0])
    assert np.array_equal(PR.expand_f32(w, None, 0.3, 5)[:, 4], w[:, 0])
    gw = torch.randn(2, 5, 8, generator=g).numpy()
    assert np.abs(PR.reduce_f32(gw) - gw.astype(np.float64).sum(1)).max() <= 1e-6


def test_schedule_is_the_published_one():
    for num_steps in (5, 100, 1000):
        for step in range(0, num_steps, max(1, num_steps // 50)):
            assert P.schedule(step, num_steps, 0.7) == pytest.approx(PR.schedule_f64(step, num_steps, 0.7), rel=1e-15, abs=0)
    lr0, s0 = P.schedule(0, 1000, 2.0)
    assert lr0 == 0.0 and s0 == pytest.approx(0.1)                      # ramp-up starts at zero; noise = w_std * 0.05
    assert P.schedule(50, 1000, 2.0)[0] == pytest.approx(0.1)            # full rate after 5 %
    assert P.schedule(750, 1000, 2.0) == pytest.approx((0.1, 0.0))       # the w-noise is gone after 75 %, the rate starts down
    assert P.schedule(999, 1000, 2.0)[0] < 1e-5
    step, inv = P.adam_scalars(0.1, 1)
    assert step == pytest.approx(1.0) and inv == pytest.approx(1 / np.sqrt(0.001))


# ---------------------------------------------------------------------------------------------------------------- it projects
def self_projection_inputs():
    """what tests/test_gpu_projection.py runs on the device: the seed-5 network, a two-layer mapper, the target = the image of a mapper
    draw with its own noise maps"""
    p, _, _, _ = make_net(5)
    mp = PR.small_mapper_params()
    g = torch.Generator().manual_seed(77)
    z = torch.randn(B, 64, generator=g).double()
    ws_t = OS.mapping_network(mp, z, num_ws_=OS.num_ws(32))
    noise_t = [torch.randn(B, 1, r, r, generator=g).double() for _, _, _, r, _ in OS.layer_list(32, 1024, 64)]
    target = OS.synthesis_network(p, ws_t, noise=noise_t)
    return p, mp, target


@pytest.mark.parametrize("space,w_noise", [("w", True), ("w+", False)])
def test_float64_loop_projects(space, w_noise):
    p, mp, target = self_projection_inputs()
    w_avg, w_std = PR.w_statistics_f64(mp, 1000)
    rows = 1 if space == "w" else OS.num_ws(32)
    w0 = w_avg[None, None].expand(B, rows, -1)
    noise0 = [PR.philox_normal(0, P.NOISE_STREAM0 + l, (B, 1, r, r)) for l, (_, _, _, r, _) in enumerate(OS.layer_list(32, 1024, 64))]
    eps_of = lambda step: PR.philox_normal(0, step, (B, rows, 64))
    dist, final = PR.project_f64(p, target, w0, noise0, eps_of, 100, w_std, weight=1e5, num_ws=OS.num_ws(32), w_noise=w_noise)
    print(f"float64 loop, space {space}, w-noise {w_noise}: distance {dist[0]:.3f} -> {final:.3f} (ratio {final / dist[0]:.4f})")
    assert final <= 0.05 * dist[0]


# ---------------------------------------------------------------------------------------------------------------- plumbing
def test_projection_save_load_round_trip(tmp_path):
    g = torch.Generator().manual_seed(0)
    out = P.Projection(torch.randn(2, 8, 64, generator=g), [torch.randn(2, 1, r, r, generator=g) for r in (4, 8, 8)],
                       {"LPIPSGrads0": torch.rand(5, 2, generator=g), "noise_reg": torch.rand(5, 2, generator=g)})
    path = out.save(tmp_path / "p.npz")
    back = P.load(path)
    assert torch.equal(back.ws, out.ws) and len(back.noise) == 3 and all(torch.equal(a, b) for a, b in zip(back.noise, out.noise))
    assert set(back.losses) == {"LPIPSGrads0", "noise_reg"} and torch.equal(back.losses["noise_reg"], out.losses["noise_reg"])
    assert list(back.noise_kwargs()) == ["noise0", "noise1", "noise2"]


def test_command_line_arguments():
    a = P.parser().parse_args(["--model_file", "net.pt", "--target", "a.png", "b.png", "--space", "w+", "--num_steps", "7", "--no_noise",
                               "--out_dir", "o"])
    assert (a.target, a.text, a.space, a.num_steps, a.no_noise, a.out_dir) == (["a.png", "b.png"], None, "w+", 7, True, "o")
    a = P.parser().parse_args(["--model_file", "None", "--text", "a prompt", "--allow_random_init", "--bpe_path", "vocab.bpe"])
    assert (a.text, a.target, a.allow_random_init, a.bpe_path, a.space, a.num_steps, a.no_noise) == ("a prompt", None, True, "vocab.bpe", "w", 1000, False)
    for bad in (["--model_file", "x"], ["--model_file", "x", "--target", "a.png", "--text", "t"], ["--target", "a.png"],
                ["--model_file", "x", "--text", "t", "--space", "z"]):
        with pytest.raises(SystemExit):
            P.parser().parse_args(bad)
    with pytest.raises(SystemExit, match="allow_random_init"):
        P.main(["--model_file", "None", "--text", "t"])


def test_project_refusals_by_name():
    class Net:
        architecture, _resize, dtype = "skip", None, torch.bfloat16

    class G:
        def __init__(self, **kw):
            self.mapper, self.synthesizer = type("M", (), {"G_map": None})(), type("S", (), {})()
            self.synthesizer.G_synth = Net()
            for k, v in kw.items():
                setattr(self.synthesizer.G_synth, k, v)

    tg = torch.zeros(1, 3, 32, 32)
    with pytest.raises(NotImplementedError, match="architecture 'resnet'"):
        P.project(G(architecture="resnet"), tg)
    with pytest.raises(NotImplementedError, match="output_size installs a resize hook"):
        P.project(G(_resize=dict(layer=0)), tg)
    with pytest.raises(NotImplementedError, match="MAUA_F16 network is not differentiated"):
        P.project(G(dtype=torch.float16), tg)
    with pytest.raises(ValueError, match="space must be"):
        P.project(G(), tg, space="z")
    with pytest.raises(ValueError, match="give targets or grad_modules"):
        P.project(G())


def test_parameterization_running_average_and_names():
    g = torch.Generator().manual_seed(4)
    xs = [torch.randn(2, 3, generator=g) for _ in range(4)]
    decay = 0.9
    pz = PZ.Parameterization(8, 8, xs[0].clone(), ema=True, decay=decay)
    # the reference's arithmetic, written out: accum, biased, average
    accum, biased = 1.0, torch.zeros(2, 3)
    accum, biased = accum * decay, biased * decay + (1 - decay) * xs[0]
    assert torch.allclose(pz.average, biased / (1 - accum)) and torch.allclose(pz.average, xs[0], atol=1e-6)
    for x in xs[1:]:
        with torch.no_grad():
            pz.tensor.copy_(x)
        pz.update_ema()
        accum, biased = accum * decay, biased * decay + (1 - decay) * x
        assert float(pz.accum) == pytest.approx(accum) and torch.allclose(pz.biased, biased) and torch.allclose(pz.average, biased / (1 - accum))
    pz.reset_ema()
    assert float(pz.accum) == pytest.approx(decay) and torch.allclose(pz.average, xs[-1], atol=1e-6)
    plain = PZ.Parameterization(8, 8, xs[0].clone())
    plain.update_ema()
    assert not hasattr(plain, "average")
    with pytest.raises(NotImplementedError):
        plain.decode_average()
    assert PZ.load_parameterization("stylegan") is PZ.StyleGANParameterization
    for name in ("rgb", "vqgan"):
        with pytest.raises(NotImplementedError, match=name):
            PZ.load_parameterization(name)
    with pytest.raises(Exception, match="not recognized"):
        PZ.load_parameterization("fourier")
    import maua.parameterizations as shim
    from maua.parameterizations.stylegan import StyleGANParameterization, project
    assert shim.load_parameterization is PZ.load_parameterization and StyleGANParameterization is PZ.StyleGANParameterization
    assert project is P.project

    class Synth:
        num_ws, w_dim, img_resolution = 8, 64, 32

    class G:
        synthesizer = type("S", (), {"G_synth": Synth()})()

    sp = PZ.StyleGANParameterization(G(), ema=True)
    assert sp.tensor.shape == (1, 8, 64) and (sp.h, sp.w) == (32, 32) and sp.noise is None
