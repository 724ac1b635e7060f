"""The optical-flow video pipeline on the device (csrc/flow.hip through maua_amd/flow.py and maua_amd/video_diffusion.py) against
tests/flow_ref.py and g38 (the reference's own results), at the project's exact-float32 bar unless a test states its own."""
import json
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flow_ref as FR  # noqa: E402
from oracle import diffusion as OD  # noqa: E402
from test_video_pipeline_host import FB_SIZES, SHIFT, farneback_bar, farneback_references  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-5


@pytest.fixture(scope="module")
def g38(golden):
    g = golden("g38_video_pipeline")
    g["meta"] = json.loads(str(g["meta_json"]))
    return g


def smooth_images(B, H, W, seed):
    """images in [-1, 1] with moderate gradients (a few sinusoids and a little noise): an off-by-one sample shows, a last-bit
    difference in a sampling position does not"""
    g = torch.Generator().manual_seed(seed)
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = torch.zeros(B, 3, H, W)
    for b in range(B):
        for c in range(3):
            p = torch.rand(6, generator=g)
            img[b, c] = 0.45 * torch.sin(x * (0.2 + 0.3 * p[0]) + 6 * p[1]) * torch.cos(y * (0.2 + 0.3 * p[2]) + 6 * p[3]) + 0.4 * (p[4] - 0.5)
    return img + 0.05 * (torch.rand(B, 3, H, W, generator=g) - 0.5)


def wide_flow(B, H, W, seed, reach=1.6):
    """flows that reach beyond one image width / height (the reflection rule is exercised)"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(B, H, W, 2, generator=g) - 0.5) * 2 * reach * torch.tensor([W, H], dtype=torch.float32)


@pytest.mark.parametrize("H,W", [(5, 7), (33, 18), (64, 64)])
def test_warp(H, W):
    import maua_amd.flow as F
    img, flow, e = smooth_images(2, H, W, 1), wide_flow(2, H, W, 2), 1.3
    assert float(flow.abs()[..., 0].max()) > W and float(flow.abs()[..., 1].max()) > H
    want = FR.warp_flow(img, flow, e)
    got = F.warp_flow(img, flow, e).cpu()
    err = float((got - want).abs().max())
    print(f"warp {H}x{W}: max abs {err:.3e}")
    assert err <= TOL
    # through the materialised grid, as the reference's callers go
    assert float((F.warp(img.cuda(), F.flow_warp_map(flow.cuda() * e)).cpu() - want).abs().max()) <= 5 * TOL


def pair_17x13():
    """An odd-sized pair with every class well populated: reliable on the lower left, a 2.2 px step at x = 9.5 (motion boundary), the
    right columns and the top rows pointing out of the frame (overshoot), and a patch where the forward flow disagrees (missed)."""
    g = torch.Generator().manual_seed(5)
    y, x = torch.meshgrid(torch.arange(13, dtype=torch.float32), torch.arange(17, dtype=torch.float32), indexing="ij")
    bx = 0.6 + 0.15 * torch.sin(x * 0.3) * torch.cos(y * 0.25) + 2.2 * (x > 9.5).float()
    by = -0.4 + 0.15 * torch.cos(x * 0.2 + y * 0.3)
    bwd = torch.stack([bx, by], -1)[None] + 0.02 * torch.rand(1, 13, 17, 2, generator=g)
    fwd = -bwd.clone()
    fwd[:, 2:6, 2:7] += torch.tensor([1.6, -1.2])
    return fwd, bwd


@pytest.mark.parametrize("name", ["smooth", "edge", "out", "17x13"])
def test_consistency(g38, name):
    import maua_amd.flow as F
    if name == "17x13":
        fwd, bwd = pair_17x13()
        want = FR.check_consistency(fwd, bwd)
        classes, masks = FR.consistency_classes(fwd, bwd)
        assert all(int(m.sum()) >= 10 for m in masks.values()) and int((classes == 1).sum()) >= 50 and int((classes == -0.75).sum()) >= 10
    else:
        fwd, bwd, want = g38[f"cc_{name}_fwd"], g38[f"cc_{name}_bwd"], g38[f"cc_{name}_map"]
    exclude, frac = FR.near_threshold(fwd, bwd)
    excluded = float(exclude.float().mean())          # the close pixels and the neighbours the blur spreads them over: all that is left out
    assert frac <= excluded <= 0.005, (frac, excluded)
    got = F.check_consistency(fwd, bwd).cpu()
    assert tuple(got.shape) == tuple(want.shape)
    err = float((got - want).abs()[0][~exclude].max())
    print(f"consistency {name}: max abs {err:.3e}, {excluded:.4f} of pixels excluded")
    assert err <= TOL
    assert torch.equal(F.get_consistency_map(fwd, bwd).cpu(), got)


@pytest.mark.parametrize("src,dst", [((9, 7), (64, 64)), ((48, 40), (16, 24))])
def test_bilinear_resize(src, dst):
    import maua_amd.flow as F
    g = torch.Generator().manual_seed(7)
    flow = (torch.rand(1, *src, 2, generator=g) - 0.5) * 14
    mult, clamp = float(np.mean((dst[1] / src[0], dst[0] / src[1]))), 5.0
    got = F.resize_bilinear(flow, dst, multiplier=mult, clamp=clamp).cpu()
    want = FR.resize_bilinear(flow, dst, mult, clamp)
    err = float((got - want).abs().max())
    print(f"bilinear resize {src} -> {dst}: max abs {err:.3e} (values up to {float(want.abs().max()):.1f})")
    assert err <= TOL and float(flow.abs().max()) > clamp
    cons = torch.rand(1, *src, generator=g)
    assert float((F.resize_bilinear(cons, dst).cpu() - FR.resize_bilinear(cons[..., None], dst)[..., 0]).abs().max()) <= TOL


COMPOSE_CASES = {"trust": dict(trust=0.75, fade=None, noise=0.02), "no_trust": dict(trust=0.0, fade=None, noise=0.02),
                 "fade": dict(trust=0.6, fade=math.sqrt(0.5), noise=0.02), "no_noise": dict(trust=0.75, fade=0.3, noise=0.0)}


@pytest.mark.parametrize("name", list(COMPOSE_CASES))
def test_composition(name):
    import maua_amd.flow as F
    from maua_amd.rng import philox_normal
    c = COMPOSE_CASES[name]
    H = W = 64
    img = smooth_images(3, H, W, 11)
    frame, prev, cached = img[0:1], img[1:2], img[2:3]
    flow = wide_flow(1, H, W, 12, reach=0.2)
    cons = torch.rand(1, 1, H, W, generator=torch.Generator().manual_seed(13))
    seed = 0x1234567890ab
    noise = philox_normal((1, 3, H, W), seed, 0).cpu()
    kw = dict(flow_exaggeration=1.2, consistency_trust=c["trust"], blend=2.0, fade=c["fade"] if c["fade"] is not None else 1.0,
              noise_injection=c["noise"], seed=seed)
    args = (frame, prev, flow, cons if c["trust"] > 0 else None, cached if c["fade"] is not None else None)
    got = F.compose(*args, **kw)
    want = FR.compose(frame, prev, flow, cons, cached if c["fade"] is not None else None, 1.2, c["trust"], 2.0, kw["fade"], c["noise"], noise)
    err = float((got.cpu() - want).abs().max())
    print(f"composition {name}: max abs {err:.3e}")
    assert err <= TOL
    assert torch.equal(F.compose(*args, **kw), got)                     # a rerun is bit-identical
    if c["noise"]:
        # the noise step alone (what runs after pre_hook / hist_persist) adds the same stream
        alone = F.compose(frame, noise_injection=c["noise"], seed=seed).cpu()
        assert float((alone - (frame + c["noise"] * noise)).abs().max()) <= 1e-6


def test_injected_noise_statistics_and_seeding():
    import maua_amd.flow as F
    sigma, n = 0.02, 64 * 64 * 3
    zero = torch.zeros(1, 3, 64, 64)
    torch.manual_seed(99)
    k1 = F.draw_noise_key()
    torch.manual_seed(99)
    k2 = F.draw_noise_key()
    k3 = F.draw_noise_key()
    assert k1 == k2 != k3                                               # the draw repeats under the same torch seed
    z = F.compose(zero, noise_injection=sigma, seed=k1).cpu().double().flatten()
    mean, var = float(z.mean()), float(z.var())
    print(f"injected noise: mean {mean:.3e} (se {sigma / math.sqrt(n):.3e}), var {var:.4e} (sigma^2 {sigma ** 2:.4e})")
    assert abs(mean) <= 5 * sigma / math.sqrt(n)
    assert abs(var - sigma ** 2) <= 5 * sigma ** 2 * math.sqrt(2 / (n - 1))
    assert torch.equal(F.compose(zero, noise_injection=sigma, seed=k2).cpu().double().flatten(), z)
    assert not torch.equal(F.compose(zero, noise_injection=sigma, seed=k3).cpu().double().flatten(), z)


def test_turbo_step():
    import maua_amd.flow as F
    img = smooth_images(2, 16, 16, 21)
    prev, nxt, flow = img[0:1], img[1:2], wide_flow(1, 16, 16, 22, reach=0.3)
    for warp_next in (False, True):                                     # t == 0: the next image is not warped
        p, n, im = F.turbo_step(prev, nxt, flow, 1.4, warp_next, 1 / 3)
        wp, wn, wi = FR.turbo(prev, nxt, flow, 1.4, warp_next, torch.tensor(1 / 3))
        assert float((p.cpu() - wp).abs().max()) <= TOL and float((n.cpu() - wn).abs().max()) <= TOL and float((im.cpu() - wi).abs().max()) <= TOL
        if not warp_next:
            assert torch.equal(n.cpu(), nxt)
    p, n, im = F.turbo_step(None, nxt, flow, 1.4, True, 0.5)
    assert p is None and torch.equal(im, n) and float((n.cpu() - FR.warp_flow(nxt, flow, 1.4)).abs().max()) <= TOL


@pytest.mark.parametrize("rows,cols", FB_SIZES)
def test_farneback_against_the_restatement(rows, cols):
    """One batched forward / backward pair against tests/flow_ref.py in float64; the bar is four times the restatement's own float32
    / float64 spread on these inputs, computed here.  Then the known-shift check on the device output."""
    import maua_amd.flow as F
    r = farneback_references(rows, cols)
    spread, bar = farneback_bar(rows, cols)
    assert F.farneback_levels(rows, cols) == FR.pyramid_levels(rows, cols) + 1
    model = F.get_flow_model()
    ab, ba = model.pair(r["a"], r["b"])
    assert tuple(ab.shape) == (1, rows, cols, 2)
    e_ab, e_ba = float((ab[0].cpu().double() - r["ab64"]).abs().max()), float((ba[0].cpu().double() - r["ba64"]).abs().max())
    print(f"farneback {cols}x{rows}: device vs float64 restatement max abs {e_ab:.3e} / {e_ba:.3e}; restatement spread {spread:.3e}, bar {bar:.3e}")
    for flow, shift in ((ab, SHIFT), (ba, (-SHIFT[0], -SHIFT[1]))):
        epe = FR.endpoint_error(flow[0].cpu(), shift, 16)
        print(f"farneback {cols}x{rows}: device mean endpoint error {epe:.4f} px")
        assert epe < 0.375
    ab2, ba2 = model.pair(r["a"], r["b"])
    assert torch.equal(ab, ab2) and torch.equal(ba, ba2)                # bit-identical rerun
    assert torch.equal(model(r["a"], r["b"]), ab)
    assert max(e_ab, e_ba) <= bar


def test_farneback_at_the_pipeline_size():
    """512 x 512, the size the pre-pass runs at: 13 pyramid levels, the widest blur (35 taps).  No CPU restatement at this size (it
    would take most of a minute): the device flow is held to the known shift alone."""
    import maua_amd.flow as F
    a, b = FR.sinusoid_pair(512, 512)
    assert F.farneback_levels(512, 512) == 13 == FR.pyramid_levels(512, 512) + 1
    ab, ba = F.get_flow_model().pair(a, b)
    for flow, shift in ((ab, SHIFT), (ba, (-SHIFT[0], -SHIFT[1]))):
        epe = FR.endpoint_error(flow[0].cpu(), shift, 16)
        print(f"farneback 512x512: device mean endpoint error {epe:.4f} px")
        assert bool(torch.isfinite(flow).all()) and epe < 0.375


SMALL = dict(image_size=64, model_channels=32, num_res_blocks=1, attention_resolutions=(16, 8), channel_mult=(1, 2, 2), num_head_channels=32)


def small_guided(timesteps=3):
    from maua_amd.diffusion import GuidedDiffusion, SpacedDiffusion, UNetModel, space_timesteps
    cfg = OD.unet_config(**SMALL)
    p = OD.init_unet_params(cfg, torch.Generator().manual_seed(0))
    net = UNetModel(image_size=cfg["image_size"], in_channels=3, model_channels=cfg["model_channels"], out_channels=cfg["out_channels"],
                    num_res_blocks=cfg["num_res_blocks"], attention_resolutions=cfg["attention_ds"], channel_mult=cfg["channel_mult"],
                    num_head_channels=cfg["num_head_channels"], use_scale_shift_norm=True, resblock_updown=True, dtype=torch.float32)
    net.load_state_dict(p)
    sd = SpacedDiffusion(space_timesteps(1000, str(timesteps)), OD.linear_betas(1000), rescale_timesteps=True)
    return GuidedDiffusion([], sampler="plms", timesteps=timesteps, model=net, diffusion=sd)


def test_end_to_end_clip():
    """A 6-frame 64 x 64 synthetic clip through video_sample with a random-init guided network: deterministic under constant_seed, N
    finite frames, and the blend matters."""
    import maua_amd.video_diffusion as VD
    frames = []
    for i in range(6):
        a, _ = FR.sinusoid_pair(64, 64, shift=(1.5 * i, -0.75 * i), seed=40)
        frames.append(_)
    clip = (torch.stack(frames) * 255).round().byte()
    gd = small_guided()
    kw = dict(size=(64, 64), turbo=2, wrap_around=1, constant_seed=17, skip=0.5, first_skip=0.3)
    a = VD.video_sample(gd, clip, **kw)
    b = VD.video_sample(gd, clip, **kw)
    assert tuple(a.shape) == (6, 3, 64, 64) and bool(torch.isfinite(a).all())
    assert torch.equal(a, b)
    c = VD.video_sample(gd, clip, blend=0, **kw)
    assert not torch.equal(a, c)


# ------------------------------------------------------------------------------------------------------------------ batches, tails, guards
# Two samples with different content against the per-sample reference (the per-batch offsets of the kernels), the composition's ragged
# last counter, the warp at other channel counts, and every operator's outputs between guard regions (tests/test_gpu_farneback.py's Buf).
def pair_batch():
    """pair_17x13 and its vertical mirror (the y flow negated): two different samples, neither with a comparison near its threshold"""
    fwd, bwd = pair_17x13()
    m = torch.tensor([1.0, -1.0])
    return torch.cat([fwd, fwd.flip(1) * m]), torch.cat([bwd, bwd.flip(1) * m])


def test_consistency_of_a_batch():
    import maua_amd.flow as F
    fwd, bwd = pair_batch()
    got = F.check_consistency(fwd, bwd).cpu()
    assert tuple(got.shape) == (2, 13, 17)
    for i in range(2):
        exclude, frac = FR.near_threshold(fwd[i:i + 1], bwd[i:i + 1])
        assert frac == 0 and not bool(exclude.any())
        err = float((got[i] - FR.check_consistency(fwd[i:i + 1], bwd[i:i + 1])[0]).abs().max())
        print(f"consistency, sample {i} of 2: max abs {err:.3e}")
        assert err <= TOL
    assert not torch.equal(got[0], got[1].flip(0))


def test_bilinear_resize_of_a_batch():
    import maua_amd.flow as F
    g = torch.Generator().manual_seed(8)
    flow = (torch.rand(2, 9, 7, 2, generator=g) - 0.5) * 14
    got = F.resize_bilinear(flow, (20, 13), multiplier=1.7, clamp=5.0).cpu()
    for i in range(2):
        err = float((got[i:i + 1] - FR.resize_bilinear(flow[i:i + 1], (20, 13), 1.7, 5.0)).abs().max())
        print(f"bilinear resize, sample {i} of 2: max abs {err:.3e}")
        assert err <= TOL
    cons = torch.rand(2, 9, 7, generator=g)
    got = F.resize_bilinear(cons, (5, 16)).cpu()
    for i in range(2):
        assert float((got[i] - FR.resize_bilinear(cons[i:i + 1, ..., None], (5, 16))[0, ..., 0]).abs().max()) <= TOL


@pytest.mark.parametrize("B", [1, 2])
def test_composition_with_a_ragged_last_counter(B):
    """5 x 7: B 3 H W = 105 / 210, no multiple of the four elements a thread takes, with the noise on"""
    import maua_amd.flow as F
    from maua_amd.rng import philox_normal
    H, W, sigma, seed = 5, 7, 0.02, 0x1234567890ab
    assert (B * 3 * H * W) % 4
    img = smooth_images(3 * B, H, W, 31)
    frame, prev, cached = img[:B], img[B:2 * B], img[2 * B:]
    flow = wide_flow(B, H, W, 32, reach=0.6)
    cons = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(33))
    noise = philox_normal((B, 3, H, W), seed, 0).cpu()
    got = F.compose(frame, prev, flow, cons, cached, flow_exaggeration=1.2, consistency_trust=0.75, blend=2.0, fade=0.3, noise_injection=sigma,
                    seed=seed).cpu()
    for i in range(B):
        s = slice(i, i + 1)
        want = FR.compose(frame[s], prev[s], flow[s], cons[s], cached[s], 1.2, 0.75, 2.0, 0.3, sigma, noise[s])
        err = float((got[s] - want).abs().max())
        print(f"composition 7x5, sample {i} of {B}: max abs {err:.3e}")
        assert err <= TOL
    alone = F.compose(frame, noise_injection=sigma, seed=seed).cpu()
    want = frame + sigma * noise
    tail = (B * 3 * H * W) % 4
    print(f"composition 7x5 B {B}: noise step alone max abs {float((alone - want).abs().max()):.3e}")
    assert torch.equal(alone.flatten()[-tail:], want.flatten()[-tail:]) and float((alone - want).abs().max()) <= 1e-6


def test_turbo_step_of_a_batch():
    import maua_amd.flow as F
    img = smooth_images(4, 9, 11, 41)
    prev, nxt, flow = img[:2], img[2:], wide_flow(2, 9, 11, 42, reach=0.3)
    p, n, im = F.turbo_step(prev, nxt, flow, 1.4, True, 1 / 3)
    for i in range(2):
        s = slice(i, i + 1)
        wp, wn, wi = FR.turbo(prev[s], nxt[s], flow[s], 1.4, True, torch.tensor(1 / 3))
        assert float((p[s].cpu() - wp).abs().max()) <= TOL and float((n[s].cpu() - wn).abs().max()) <= TOL and float((im[s].cpu() - wi).abs().max()) <= TOL


@pytest.mark.parametrize("C", [1, 4])
def test_warp_at_other_channel_counts(C):
    import maua_amd.flow as F
    H, W = 9, 11
    img = smooth_images(4, H, W, 51)[:, :1].reshape(1, 4, H, W).repeat(2, 1, 1, 1)[:, :C].contiguous()
    img[1] = img[1].flip(-1)
    flow = wide_flow(2, H, W, 52)
    err = float((F.warp_flow(img, flow, 1.3).cpu() - FR.warp_flow(img, flow, 1.3)).abs().max())
    print(f"warp C {C}: max abs {err:.3e}")
    assert err <= TOL


def test_outputs_between_guard_regions():
    """each of the five operators writes its outputs whole and nothing else: B = 2 at 5 x 7, sizes that fill no workgroup"""
    import maua_amd.flow as F
    from test_gpu_farneback import Buf
    B, H, W = 2, 5, 7
    img = smooth_images(3 * B, H, W, 61)
    frame, prev, cached = img[:B], img[B:2 * B], img[2 * B:]
    flow = wide_flow(B, H, W, 62, reach=0.6)
    cons = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(63))
    o = Buf((B, 3, H, W))
    assert torch.equal(F.warp_flow(frame, flow, 1.3, out=o.t).cpu(), F.warp_flow(frame, flow, 1.3).cpu())
    o.check("warp")
    fwd, bwd = pair_batch()
    cl, res = Buf((2, 13, 17)), Buf((2, 13, 17))
    assert torch.equal(F.check_consistency(fwd, bwd, out=(cl.t, res.t)).cpu(), F.check_consistency(fwd, bwd).cpu())
    cl.check("consistency classes")
    res.check("consistency map")
    o = Buf((B, 9, 4, 2))
    assert torch.equal(F.resize_bilinear(flow, (9, 4), 1.5, 5.0, out=o.t).cpu(), F.resize_bilinear(flow, (9, 4), 1.5, 5.0).cpu())
    o.check("bilinear resize")
    o = Buf((B, 3, H, W))
    kw = dict(flow_exaggeration=1.2, consistency_trust=0.75, blend=2.0, fade=0.3, noise_injection=0.02, seed=77)
    assert torch.equal(F.compose(frame, prev, flow, cons, cached, out=o.t, **kw).cpu(), F.compose(frame, prev, flow, cons, cached, **kw).cpu())
    o.check("composition")
    outs = [Buf((B, 3, H, W)) for _ in range(3)]
    p, n, im = F.turbo_step(prev, frame, flow, 1.4, True, 0.25, out=tuple(b.t for b in outs))
    q = F.turbo_step(prev, frame, flow, 1.4, True, 0.25)
    assert all(torch.equal(x.cpu(), y.cpu()) for x, y in zip((p, n, im), q))
    for b, what in zip(outs, ("turbo prev", "turbo next", "turbo img")):
        b.check(what)
