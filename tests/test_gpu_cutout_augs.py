"""GPU tests of the augmented "normal" / "dango" cutouts (maua/ops/cutouts.py:53-206, skip_augs=False; csrc/cutout_augs.hip): the
forward against the REFERENCE's outputs (g36), the adjoint by dot products and against torch.autograd through the CPU restatement
(tests/torchvision_augs_ref.py), bit-for-bit reruns, CLIPGrads end to end, and the guided sampler."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import torchvision_augs_ref as TA  # noqa: E402
from oracle import clip as OC  # noqa: E402
from oracle import grads as OG  # noqa: E402

pytestmark = pytest.mark.gpu


def g36():
    z = np.load(Path(__file__).resolve().parent / "golden" / "g36_cutout_augs.npz")
    return {k: z[k] for k in z.files}


def rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def fwd(img, rects, augs, key, per_call, cs, mul=1.0, add=0.0, mean=(0.0,) * 3, std=(1.0,) * 3):
    from maua_amd.grad import _run_cutouts_aug
    return _run_cutouts_aug(img, rects, augs, key, per_call, cs, mul, add, mean, std)


def vjp(d, B, H, W, rects, augs, per_call, cs, mul=1.0, std=(1.0,) * 3):
    from maua_amd import _lib as L
    r = np.ascontiguousarray(np.asarray(rects, dtype=np.int32).reshape(-1, 3))
    a = np.ascontiguousarray(np.asarray(augs, dtype=np.float32).reshape(-1, 17))
    dd = d.cuda().float().contiguous()
    out = torch.empty(B, 3, H, W, device="cuda")
    L.check(L.lib().maua_cutouts_aug_vjp(L.ctx(), L.ptr(dd), B, H, W, r.ctypes.data_as(C.c_void_p), len(r), cs, C.c_float(mul),
                                         (C.c_float * 3)(*std), a.ctypes.data_as(C.c_void_p), int(per_call), L.ptr(out)))
    return out


def affine_ties(rec, s, tol=1e-3):
    """Whether the nearest affine sampling of record rec on an s x s image has a source coordinate within tol px of k + 1/2."""
    grid = TA.affine_grid([float(v) for v in rec[1:7]], s, s)[0]
    ix = ((grid + 1) * s - 1) / 2
    frac = (ix - torch.floor(ix) - 0.5).abs()
    return bool((frac < tol).any())


def check_forward(got, want, recs_of_image, side_of_image):
    """>= 99.9 % of the values within 1e-5; every image holding a larger difference has a nearest-neighbour tie in its affine grid."""
    d = (got.cpu() - torch.as_tensor(want)).abs()
    bad = d > 1e-5
    assert float(bad.float().mean()) <= 1e-3, float(bad.float().mean())
    for i in torch.nonzero(bad.flatten(1).any(1)).flatten().tolist():
        assert affine_ties(recs_of_image(i), side_of_image(i)), (i, float(d[i].max()))


def test_forward_matches_the_reference_fixture():
    from maua_amd.grad import DangoCutouts
    g = g36()
    for k in range(2):
        S, cs, cutn, seed = (int(v) for v in g[f"normal{k}_cfg"])
        img = torch.from_numpy(g[f"normal{k}_img"])
        p = S // 4
        padded = torch.nn.functional.pad(img, (p,) * 4)
        rects, augs = g[f"normal{k}_rects"], g[f"normal{k}_augs"]
        got = fwd(padded, rects, augs, int(g[f"normal{k}_key"]), False, cs)
        check_forward(got, g[f"normal{k}_out"], lambda i: augs[i // 2], lambda i: int(rects[i // 2][0]))
    for k in range(2):
        S, cs, t, seed, overview, inner = (int(v) for v in g[f"dango{k}_cfg"])
        torch.manual_seed(seed)
        rects = DangoCutouts(cs, skip_augs=True).rects(S, S, t)
        augs = g[f"dango{k}_augs"]
        got = fwd(torch.from_numpy(g[f"dango{k}_img"]), rects, augs, int(g[f"dango{k}_key"]), True, cs)
        check_forward(got, g[f"dango{k}_out"], lambda i: augs[0], lambda i: cs)


def records(seed, n, side):
    """n records drawn like the reference's, then every combination of (flip, perspective on / off, grey) forced in turn."""
    from maua_amd.grad import draw_augs
    torch.manual_seed(seed)
    out = []
    for i in range(n):
        r = draw_augs(side, side)
        while not r[7]:            # (a perspective to switch off when the combination asks for it)
            r = draw_augs(side, side)
        r[0], r[16] = i & 1, (i >> 2) & 1
        if (i >> 1) & 1:
            r[7], r[8:16] = 0, 0
        out.append(r)
    return np.stack(out)


def test_adjoint_dot_products_and_autograd():
    """<A x, y> = <x, A^T y> (float64 sums) for both modes and all of (flip, perspective on / off, grey); A x = out(x) - out(0): the noise
    is the affine part.  And the VJP against torch.autograd through the CPU restatement (no noise: it drops out of the gradient)."""
    g = torch.Generator().manual_seed(7)
    B, S, cs = 2, 40, 24
    std = (0.3, 0.5, 0.7)
    rects = [(40, 0, 0), (30, 4, 6), (28, 12, 0), (36, 2, 3), (25, 15, 15), (33, 7, 1), (40, 0, 0), (31, 9, 9)]
    augs = np.stack([records(11 + i, 8, r[0])[i] for i, r in enumerate(rects)])
    x = torch.rand(B, 3, S, S, generator=g)
    y = torch.randn(len(rects) * B, 3, cs, cs, generator=g)
    ax = fwd(x, rects, augs, 5, False, cs, std=std) - fwd(torch.zeros_like(x), rects, augs, 5, False, cs, std=std)
    aty = vjp(y, B, S, S, rects, augs, False, cs, std=std)
    lhs, rhs = float((ax.cpu().double() * y.double()).sum()), float((x.double() * aty.cpu().double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (lhs, rhs)
    with torch.enable_grad():
        xx = x.clone().requires_grad_()
        outs = []
        for (s, t, l), rec in zip(rects, augs):
            outs.append(OC.resize(TA.augment(xx[:, :, t:t + s, l:l + s], rec), (cs, cs)))
        ref = (torch.cat(outs) - 0) / torch.tensor(std).view(1, 3, 1, 1)
        want = torch.autograd.grad(ref, xx, y)[0]
    assert rel(aty, want) <= 1e-4, rel(aty, want)
    assert rel(ax, ref.detach()) <= 1e-4, rel(ax, ref.detach())
    # "dango": one record over the whole resized batch, each combination in turn
    from maua_amd.grad import DangoCutouts
    S2 = 48
    x2 = torch.rand(1, 3, S2, S2, generator=g)
    dc = DangoCutouts(32, skip_augs=True)
    torch.manual_seed(3)
    plan = dc.plan(S2, S2, 700)
    torch.manual_seed(3)
    drects = dc.rects(S2, S2, 700)
    for i, rec in enumerate(records(21, 8, 32)):
        y2 = torch.randn(len(drects), 3, 32, 32, generator=g)
        ax = fwd(x2, drects, rec[None], 9, True, 32, std=std) - fwd(torch.zeros_like(x2), drects, rec[None], 9, True, 32, std=std)
        aty = vjp(y2, 1, S2, S2, drects, rec[None], True, 32, std=std)
        lhs, rhs = float((ax.cpu().double() * y2.double()).sum()), float((x2.double() * aty.cpu().double()).sum())
        assert abs(lhs - rhs) <= 1e-5 * abs(lhs), (i, lhs, rhs)
        with torch.enable_grad():
            xx = x2.clone().requires_grad_()
            ref = TA.augment(OG.dango_cutouts(xx, plan, 32, OC.resize), rec) / torch.tensor(std).view(1, 3, 1, 1)
            want = torch.autograd.grad(ref, xx, y2)[0]
        assert rel(aty, want) <= 1e-4, (i, rel(aty, want))


def test_reruns_are_bit_identical():
    g = torch.Generator().manual_seed(8)
    B, S, cs = 2, 40, 24
    rects = [(40, 0, 0), (30, 4, 6), (28, 12, 0), (36, 2, 3)]
    augs = np.stack([records(31 + i, 4, r[0])[i] for i, r in enumerate(rects)])
    x = torch.rand(B, 3, S, S, generator=g)
    y = torch.randn(len(rects) * B, 3, cs, cs, generator=g)
    for per_call, a in ((False, augs), (True, augs[:1])):
        rr = rects if not per_call else [(r[0], r[1], r[2]) for r in rects]
        side = cs
        if per_call:
            a = records(41, 1, side)
        o1, o2 = fwd(x, rr, a, 77, per_call, cs), fwd(x, rr, a, 77, per_call, cs)
        d1, d2 = vjp(y, B, S, S, rr, a, per_call, cs), vjp(y, B, S, S, rr, a, per_call, cs)
        assert torch.equal(o1, o2) and torch.equal(d1, d2)


def _tiny_clip():
    from maua_amd.clip import CLIPImageModel, VisionTransformer
    cfg = dict(input_resolution=32, patch_size=8, width=64, layers=2, heads=2, output_dim=32)
    p = OC.init_vit_params(cfg, torch.Generator().manual_seed(2))
    vt = VisionTransformer(32, 8, 64, 2, 2, 32, dtype=torch.float32)
    vt.load_state_dict(p, strict=True)
    return cfg, p, CLIPImageModel(vt)


def test_clipgrads_with_augmented_cutouts_matches_autograd():
    """CLIPGrads(cutouts="normal") and (cutouts="dango") at their defaults (skip_augs=False), exact f32: the module's recorded plan and
    noise keys, then torch.autograd through the CPU restatement, oracle.clip and the loss."""
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    cfg, p, model = _tiny_clip()
    gen = torch.Generator().manual_seed(19)
    emb = torch.randn(2, 32, generator=gen)
    w = OC.normalise_weights(torch.tensor([1.0, 0.5]))
    for mode, kw, S, t in (("normal", dict(cutn=8), 40, 400), ("dango", dict(cutn=16), 48, 300), ("dango", dict(cutn=16), 48, 700)):
        m = CLIPGrads(scale=90.0, cutouts=mode, cutout_kwargs=kw, cutout_batches=2, clip_models=[model])
        m.set_targets([EmbeddingPrompt(emb[0], 1.0), EmbeddingPrompt(emb[1], 0.5)])
        B = 2
        img = torch.rand(B, 3, S, S, generator=gen) * 2 - 1
        torch.manual_seed(23)
        grad = m.forward(img, torch.tensor([float(t)] * B))
        rects, augs, keys = m.last_aug_plan[0]
        want = torch.zeros_like(img)
        for k in range(rects.shape[0]):
            with torch.enable_grad():
                x = img.clone().requires_grad_()
                u = x.add(1).div(2)
                if mode == "normal":
                    pad = S // 4
                    u = torch.nn.functional.pad(u, (pad,) * 4)
                    outs = []
                    for j, ((s, y0, x0), rec) in enumerate(zip(rects[k], augs[k])):
                        crop = u[:, :, y0:y0 + s, x0:x0 + s]
                        outs.append(OC.resize(TA.augment(crop, rec, TA.philox_noise(keys[k], j, crop.shape)), (32, 32)))
                    cuts = torch.cat(outs)
                else:   # (the crops of batch k: the plans re-drawn in the module's order - crops, then the call's record)
                    from maua_amd.grad import draw_augs
                    torch.manual_seed(23)
                    plans = []
                    for _ in range(rects.shape[0]):
                        plans.append(m.cutouts[0].plan(S, S, t))
                        assert np.array_equal(draw_augs(32, 32), augs[len(plans) - 1][0])
                    base = OG.dango_cutouts(u, plans[k], 32, OC.resize)
                    cuts = TA.augment(base, augs[k][0], TA.philox_noise(keys[k], 0, base.shape))
                e = OC.encode_image(p, cfg, OC.normalize(cuts)).float()
                dists = OC.spherical_dist_loss(e.unsqueeze(1), emb.unsqueeze(0))
                loss = dists.view((-1, B, dists.shape[-1])).mul(w).sum(2).mean(0)
                want += torch.autograd.grad(loss.sum() * 90.0, x)[0] / rects.shape[0]
        assert rel(grad, want) <= 5e-4, (mode, t, rel(grad, want))
        assert m.graph_spec() is None


def test_guided_sampler_with_augmented_cutouts():
    """A few guided steps of GuidedDiffusion with CLIPGrads(cutouts="normal") at its defaults: finite, repeatable under
    torch.manual_seed, and different from the same module with skip_augs=True."""
    from maua_amd.diffusion import GuidedDiffusion, SpacedDiffusion, UNetModel, space_timesteps
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    from oracle import diffusion as OD
    gen = torch.Generator().manual_seed(15)
    ucfg = OD.unet_config(image_size=64, model_channels=32, num_res_blocks=1, attention_resolutions=(16, 8), channel_mult=(1, 2, 2), num_head_channels=32)
    net = UNetModel(image_size=64, in_channels=3, model_channels=32, out_channels=ucfg["out_channels"], num_res_blocks=1,
                    attention_resolutions=ucfg["attention_ds"], channel_mult=(1, 2, 2), num_head_channels=32, use_scale_shift_norm=True,
                    resblock_updown=True, dtype=torch.float32)
    net.load_state_dict(OD.init_unet_params(ucfg, torch.Generator().manual_seed(0)))
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    _, _, model = _tiny_clip()
    prompt = EmbeddingPrompt(torch.randn(32, generator=gen), 1.0)
    img, nz = torch.randn(2, 3, 64, 64, generator=gen), torch.randn(2, 3, 64, 64, generator=gen)
    outs = {}
    for skip in (False, True):
        cg = CLIPGrads(scale=2000.0, cutouts="normal", cutout_kwargs=dict(cutn=8, skip_augs=skip), cutout_batches=2, clip_models=[model])
        assert cg.graph_spec() is None
        gd = GuidedDiffusion([cg], timesteps=20, model=net, diffusion=sd, speed="hyper")
        torch.manual_seed(4)
        a = gd.forward(img, [prompt], 0.3, t_end=0.6, noise=nz)
        torch.manual_seed(4)
        b = gd.forward(img, [prompt], 0.3, t_end=0.6, noise=nz)
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), skip
        outs[skip] = a
    assert rel(outs[False], outs[True]) > 1e-4
