"""GPU tests of the 14-pixel-patch image towers (CLIP ViT-L/14, 224 and 336 px): patch rows of 3 * 14^2 = 588 values held at a padded
stride of 640, the memory-aware group size (maua_clip_set_workspace_limit), the towers at the public interface.

Small towers (res 28: a 2 x 2 grid, 5 tokens, head width 32; res 42: an odd 3 x 3 grid, 10 tokens, head width 64) carry the parity
argument against the CPU oracle (oracle/clip.py, torch.autograd on it), at the bars the 16-pixel tower is held to: exact-f32 embedding
<= 1e-4, input gradient <= 2e-4, CLIPGrads <= 3e-4 of the gradient's maximum (tests/test_gpu_clip.py), augmented end to end <= 5e-4
(tests/test_gpu_cutout_augs.py), bf16 gradient cosine >= 0.98.  The full-size towers run once each, bf16 against float32 on the device."""
import ctypes as C
import re
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

T28 = dict(input_resolution=28, patch_size=14, width=64, layers=2, heads=2, output_dim=32)   # 2 x 2 patches, head width 32
T42 = dict(input_resolution=42, patch_size=14, width=64, layers=2, heads=1, output_dim=32)   # 3 x 3 patches, head width 64
P16 = dict(input_resolution=32, patch_size=16, width=64, layers=2, heads=2, output_dim=32)
TOWERS = [T28, T42]
IDS = ["res28-hc32", "res42-hc64"]


def rel(a, b):
    a, b = torch.as_tensor(a).detach().float().cpu(), torch.as_tensor(b).detach().float().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def cos(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))


def _tower(cfg, dt, seed=0):
    from maua_amd.clip import VisionTransformer
    p = OC.init_vit_params(cfg, torch.Generator().manual_seed(seed))
    vt = VisionTransformer(cfg["input_resolution"], cfg["patch_size"], cfg["width"], cfg["layers"], cfg["heads"], cfg["output_dim"], dtype=dt)
    vt.load_state_dict(p, strict=True)
    return vt, p


def _targets(E, P, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(P, E, generator=g), OC.normalise_weights(torch.rand(P, generator=g) + 0.2)


def _guide_grad(vt, img, rects, tgt, w, scale, clamp=0.0):
    """maua_clip_guide_grad on host rectangles [batches][cutn][3] (no merging) -> gradient on the device."""
    from maua_amd import _lib as L
    lib = L.lib()
    tn, wn = np.ascontiguousarray(tgt.numpy()), np.ascontiguousarray(w.numpy())
    L.check(lib.maua_clip_set_targets(vt._handle(), tn.ctypes.data_as(C.c_void_p), wn.ctypes.data_as(C.c_void_p), 1, tgt.shape[0], None, 0))
    r = np.ascontiguousarray(np.asarray(rects, dtype=np.int32))
    imgd = img.cuda()
    out = torch.empty_like(imgd)
    B, _, H, W = img.shape
    L.check(lib.maua_clip_guide_grad(vt._handle(), L.ptr(imgd), B, H, W, r.ctypes.data_as(C.c_void_p), None, r.shape[1], r.shape[0],
                                     C.c_float(scale), C.c_float(clamp), L.ptr(out)))
    return out


# ------------------------------------------------------------------------------------------------ the tower
@pytest.mark.parametrize("cfg", TOWERS, ids=IDS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_p14_tower_forward_and_input_gradient_match_the_oracle(cfg, dt):
    vt, p = _tower(cfg, dt)
    R = cfg["input_resolution"]
    g = torch.Generator().manual_seed(5)
    x = torch.randn(5, 3, R, R, generator=g)
    de = torch.randn(5, cfg["output_dim"], generator=g)
    with torch.enable_grad():
        xx = x.clone().requires_grad_()
        ref = OC.encode_image(p, cfg, xx)
        want = torch.autograd.grad(ref, xx, de)[0]
    out = vt(x, keep=True)
    gx = vt.vjp(de)
    print(f"p14 tower {R} {dt}: embedding rel {rel(out, ref):.3e} cos {cos(out, ref):.6f}; input gradient rel {rel(gx, want):.3e} cos {cos(gx, want):.6f}")
    if dt == torch.float32:
        assert rel(out, ref) <= 1e-4 and rel(gx, want) <= 2e-4
    else:
        assert cos(out, ref) >= 0.999 and cos(gx, want) >= 0.99
    assert torch.equal(vt(x), out)


@pytest.mark.parametrize("cfg", TOWERS, ids=IDS)
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_p14_clip_guide_grad_matches_autograd_on_the_oracle(cfg, dt):
    vt, p = _tower(cfg, dt, seed=1)
    cs = cfg["input_resolution"]
    tgt, w = _targets(cfg["output_dim"], 3, 4)
    B, H, W, cutn, batches = 2, 40, 48, 8, 2
    img = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(6)) * 2 - 1
    torch.manual_seed(12)
    rects = [OC.cutout_rects(H, W, cs, cutn, OC.maua_cutouts_pow(620)) for _ in range(batches)]
    want = OC.clip_grads(p, cfg, img, rects, tgt, w, scale=150.0)
    out = _guide_grad(vt, img, rects, tgt, w, 150.0)
    print(f"p14 CLIPGrads res {cs} {dt}: rel {rel(out, want):.3e} cos {cos(out, want):.6f}")
    if dt == torch.float32:
        assert rel(out, want) <= 3e-4
    else:
        assert cos(out, want) >= 0.98


@pytest.mark.parametrize("cfg", TOWERS, ids=IDS)
def test_p14_clipgrads_module_with_maua_cutouts(cfg):
    """CLIPGrads.forward drawing its own cutouts (cut_size from visual.input_resolution) against the oracle under the same seed."""
    from maua_amd.clip import CLIPImageModel
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    vt, p = _tower(cfg, torch.float32, seed=2)
    cs, E = cfg["input_resolution"], cfg["output_dim"]
    g = torch.Generator().manual_seed(8)
    e0, e1 = torch.randn(E, generator=g), torch.randn(E, generator=g)
    gm = CLIPGrads(scale=80.0, clip_models=[CLIPImageModel(vt)], cutout_kwargs=dict(cutn=8), cutout_batches=2)
    assert gm.cutouts[0].cut_size == cs
    B, H, W = 2, 48, 48
    img = torch.rand(B, 3, H, W, generator=g) * 2 - 1
    t = torch.tensor([437.0, 437.0])
    gm.set_targets([EmbeddingPrompt(e0, 1.0), EmbeddingPrompt(e1, 3.0)])
    torch.manual_seed(77)
    got = gm(img, t)
    torch.manual_seed(77)
    rects = [OC.cutout_rects(H, W, cs, 8, OC.maua_cutouts_pow(t[[0]].long())) for _ in range(2)]
    want = OC.clip_grads(p, cfg, img, rects, torch.stack([e0, e1]), OC.normalise_weights([1.0, 3.0]), scale=80.0)
    print(f"p14 CLIPGrads module res {cs}: rel {rel(got, want):.3e}")
    assert rel(got, want) <= 3e-4
    assert gm.graph_spec() is not None


@pytest.mark.parametrize("mode,kw,S,t", [("normal", dict(cutn=8), 40, 400), ("dango", dict(cutn=16), 48, 300)], ids=["normal", "dango"])
def test_p14_clipgrads_with_augmented_cutouts_matches_autograd(mode, kw, S, t):
    """tests/test_gpu_cutout_augs.py's end-to-end check on the 3 x 3-patch tower: the augmented cutouts' output pass writes patch rows
    at the padded stride ("dango"), the resize does ("normal"); torch.autograd through the CPU restatement, <= 5e-4."""
    from maua_amd.clip import CLIPImageModel
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt, draw_augs
    cfg = T42
    cs = cfg["input_resolution"]
    vt, p = _tower(cfg, torch.float32, seed=2)
    gen = torch.Generator().manual_seed(19)
    emb = torch.randn(2, 32, generator=gen)
    w = OC.normalise_weights(torch.tensor([1.0, 0.5]))
    m = CLIPGrads(scale=90.0, cutouts=mode, cutout_kwargs=kw, cutout_batches=2, clip_models=[CLIPImageModel(vt)])
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
                    outs.append(OC.resize(TA.augment(crop, rec, TA.philox_noise(keys[k], j, crop.shape)), (cs, cs)))
                cuts = torch.cat(outs)
            else:
                torch.manual_seed(23)
                plans = []
                for _ in range(rects.shape[0]):
                    plans.append(m.cutouts[0].plan(S, S, t))
                    assert np.array_equal(draw_augs(cs, cs), augs[len(plans) - 1][0])
                base = OG.dango_cutouts(u, plans[k], cs, OC.resize)
                cuts = TA.augment(base, augs[k][0], TA.philox_noise(keys[k], 0, base.shape))
            e = OC.encode_image(p, cfg, OC.normalize(cuts)).float()
            dists = OC.spherical_dist_loss(e.unsqueeze(1), emb.unsqueeze(0))
            loss = dists.view((-1, B, dists.shape[-1])).mul(w).sum(2).mean(0)
            want += torch.autograd.grad(loss.sum() * 90.0, x)[0] / rects.shape[0]
    print(f"p14 augmented CLIPGrads {mode}: rel {rel(grad, want):.3e}")
    assert rel(grad, want) <= 5e-4, (mode, rel(grad, want))


# ------------------------------------------------------------------------------------------------ pad columns
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_pad_columns_stay_zero_on_a_reused_workspace(dt):
    """The patch rows' 52 pad columns are zeroed when the buffer is allocated and never written: a handle that ran many images and then
    few gives the bits of a fresh handle on the few; and the gradient of a zero upstream gradient is exactly zero."""
    g = torch.Generator().manual_seed(31)
    R = T42["input_resolution"]
    many, few = torch.randn(24, 3, R, R, generator=g) * 3, torch.randn(3, 3, R, R, generator=g)
    de = torch.randn(3, T42["output_dim"], generator=g)
    used, _ = _tower(T42, dt, seed=4)
    used(many, keep=True)
    used.vjp(torch.randn(24, T42["output_dim"], generator=g))
    e1 = used(few, keep=True).clone()
    g1 = used.vjp(de).clone()
    fresh, _ = _tower(T42, dt, seed=4)
    e2 = fresh(few, keep=True)
    g2 = fresh.vjp(de)
    assert torch.equal(e1, e2) and torch.equal(g1, g2)
    used(many[:7], keep=True)
    z = used.vjp(torch.zeros(7, T42["output_dim"]))
    assert bool((z == 0).all())
    # the same through the guidance call (cutout resize writes the rows): many cutouts, then few, against a fresh handle
    tgt, w = _targets(T42["output_dim"], 2, 3)
    img = torch.rand(2, 3, 48, 56, generator=g) * 2 - 1
    torch.manual_seed(5)
    big = [OC.cutout_rects(48, 56, R, 12, OC.maua_cutouts_pow(500))]
    small = [OC.cutout_rects(48, 56, R, 3, OC.maua_cutouts_pow(500))]
    _guide_grad(used, img, big, tgt, w, 10.0)
    a = _guide_grad(used, img, small, tgt, w, 10.0).clone()
    b = _guide_grad(fresh, img, small, tgt, w, 10.0)
    assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ group size
def _bytes_of_one_cutout(gm, img, t):
    """A limit below one cutout of the batch is refused, and the message says how many bytes one cutout needs."""
    gm.clip_models[0].visual.set_workspace_limit(1)
    with pytest.raises(RuntimeError, match=r"one cutout of this batch \(\d+ images\) needs \d+ bytes") as e:
        gm(img, t)
    return int(re.search(r"needs (\d+) bytes", str(e.value)).group(1))


def _images_of_last_pass(vt, n):
    """True when the last pass through the tower had at least n images (maua_clip_last_image_losses refuses more than it had)."""
    from maua_amd import _lib as L
    out = torch.empty(max(n, 1), device="cuda")
    return L.lib().maua_clip_last_image_losses(vt._handle(), n, L.ptr(out)) == 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_workspace_limit_splits_the_cutouts_and_the_gradient_stays(dt):
    """maua_clip_set_workspace_limit forcing 1, 2 and all cutouts per pass: the gradient is the same sum over cutouts, accumulated
    into the image in groups.  float32: <= 3e-4 of the maximum against the unsplit call and the oracle (the bar of the unsplit call).
    bf16: every image goes through the same kernels whatever the group, so only the float32 accumulation into the image gradient
    changes its order: a pixel's value is a sum of N <= cutn * 16 (resize taps) products, and two orders of a float32 sum of N terms
    differ by at most 2 (N - 1) 2^-24 sum |terms|; with sum |terms| <= 8 max |gradient| (cancellation between cutouts), cutn = 8:
    2 * 127 * 2^-24 * 8 = 1.2e-4 of the maximum.  Measured on an MI355X: groups of 1 / 2 cutouts against the unsplit call 1.4e-7 /
    1.0e-7 (bf16), 1.4e-7 / 1.4e-7 (float32); against the oracle 8.9e-7 (float32), cosine 0.99996 (bf16), split or not."""
    from maua_amd.clip import CLIPImageModel
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    cfg = T42
    vt, p = _tower(cfg, dt, seed=6)
    cs, E, cutn, B = cfg["input_resolution"], cfg["output_dim"], 8, 2
    g = torch.Generator().manual_seed(41)
    e0 = torch.randn(E, generator=g)
    gm = CLIPGrads(scale=60.0, clip_models=[CLIPImageModel(vt)], cutout_kwargs=dict(cutn=cutn), cutout_batches=2)
    gm.merge_cutouts = False
    gm.set_targets([EmbeddingPrompt(e0, 1.0)])
    img = torch.rand(B, 3, 48, 48, generator=g) * 2 - 1
    t = torch.tensor([500.0] * B)
    torch.manual_seed(3)
    whole = gm(img, t).clone()
    assert _images_of_last_pass(vt, cutn * B)
    torch.manual_seed(3)
    rects = [OC.cutout_rects(48, 48, cs, cutn, OC.maua_cutouts_pow(500)) for _ in range(2)]
    want = OC.clip_grads(p, cfg, img, rects, e0[None], torch.ones(1), scale=60.0)
    one = _bytes_of_one_cutout(gm, img, t)
    bar = 3e-4 if dt == torch.float32 else 2 * (cutn * 16 - 1) * 2.0 ** -24 * 8
    for per_pass in (1, 2, cutn):
        vt.set_workspace_limit(one * per_pass + one // 2)
        torch.manual_seed(3)
        got = gm(img, t)
        assert _images_of_last_pass(vt, per_pass * B) and not _images_of_last_pass(vt, per_pass * B + 1)
        print(f"group of {per_pass} cutouts, {dt}: vs unsplit {rel(got, whole):.3e}, vs oracle rel {rel(got, want):.3e} cos {cos(got, want):.6f}")
        assert rel(got, whole) <= bar
        if dt == torch.float32:
            assert rel(got, want) <= 3e-4
        else:
            assert cos(got, want) >= 0.98
        if per_pass == cutn:
            assert torch.equal(got, whole)
    # lifted: the automatic budget again, the handle works as before
    vt.set_workspace_limit(0)
    torch.manual_seed(3)
    assert torch.equal(gm(img, t), whole)


def test_p16_tower_is_unchanged_by_a_limit_that_does_not_bind():
    from maua_amd.clip import CLIPImageModel
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    vt, _ = _tower(P16, torch.bfloat16, seed=7)
    g = torch.Generator().manual_seed(43)
    gm = CLIPGrads(scale=60.0, clip_models=[CLIPImageModel(vt)], cutout_kwargs=dict(cutn=8), cutout_batches=2)
    gm.set_targets([EmbeddingPrompt(torch.randn(P16["output_dim"], generator=g), 1.0)])
    img = torch.rand(2, 3, 48, 48, generator=g) * 2 - 1
    t = torch.tensor([500.0, 500.0])
    torch.manual_seed(9)
    free = gm(img, t).clone()
    vt.set_workspace_limit(1 << 30)
    torch.manual_seed(9)
    assert torch.equal(gm(img, t), free)


# ------------------------------------------------------------------------------------------------ the captured loop
def test_p14_text_guided_sampler_loop_graph_equals_step_by_step():
    """tests/test_gpu_clip.py's captured-loop check with a single 14-pixel-patch perceptor: the short guided loop as one hipGraph
    against the step-by-step path under the same seed, twice (the second call replays the graph with new rectangles)."""
    from maua_amd.clip import CLIPImageModel
    from maua_amd.diffusion import GuidedDiffusion, SecondaryDiffusionImageNet2, SpacedDiffusion, UNetModel, space_timesteps
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    from oracle import diffusion as OD
    vt, _ = _tower(T42, torch.bfloat16, seed=2)
    E = T42["output_dim"]
    g = torch.Generator().manual_seed(3)
    net = UNetModel(image_size=64, in_channels=3, model_channels=32, out_channels=6, num_res_blocks=1, attention_resolutions=(4, 8),
                    channel_mult=(1, 2, 2), num_head_channels=32, use_scale_shift_norm=True, resblock_updown=True, dtype=torch.bfloat16,
                    generator=g)
    sec = SecondaryDiffusionImageNet2(dtype=torch.float32, generator=g, exact=False)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim6"), OD.linear_betas(1000), rescale_timesteps=True)
    prompts = [EmbeddingPrompt(torch.randn(E, generator=g)), EmbeddingPrompt(torch.randn(E, generator=g), 0.5)]
    outs = {}
    for use_graph in (True, False):
        gm = CLIPGrads(scale=500.0, clip_models=[CLIPImageModel(vt)], cutout_kwargs=dict(cutn=8), cutout_batches=2, clamp_gradient=0.05)
        gd = GuidedDiffusion([gm], timesteps=6, model=net, diffusion=sd, speed="fast", secondary_model=sec)
        gd.use_graph = use_graph
        res = []
        for rep in range(2):
            gg = torch.Generator().manual_seed(40 + rep)
            x0, nz = torch.randn(2, 3, 64, 64, generator=gg), torch.randn(2, 3, 64, 64, generator=gg)
            torch.manual_seed(90 + rep)
            res.append(gd.run(x0, prompts, 5, 6, noise=nz).clone())
        outs[use_graph] = res
        if use_graph:
            assert net.guided_graph_active()
    for a, b in zip(outs[True], outs[False]):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert not torch.equal(outs[True][0], outs[True][1])


# ------------------------------------------------------------------------------------------------ the full shapes
@pytest.mark.parametrize("name", ["ViT-L/14", "ViT-L/14@336px"])
def test_full_size_tower_bf16_against_float32_on_the_device(name):
    """Random-init ViT-L/14 at its real shape (24 layers, width 1024, 257 / 577 tokens), 2 images x 4 cutouts, one CLIPGrads call: finite,
    non-zero, and the bf16 gradient's cosine against the same tower in float32 mode >= 0.98.  (The CPU oracle at this size takes
    minutes; the small towers above carry the parity argument.)"""
    from maua_amd import clip as CL
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    g = torch.Generator().manual_seed(11)
    m16, _ = CL.load(name, dtype=torch.bfloat16, allow_random_init=True, generator=torch.Generator().manual_seed(1), text_tower=False)
    m32, _ = CL.load(name, dtype=torch.float32, allow_random_init=True, generator=torch.Generator().manual_seed(1), text_tower=False)
    R = CL.VISION_CONFIGS[name][0]
    e0 = torch.randn(768, generator=g)
    img = torch.rand(2, 3, 256, 320, generator=g) * 2 - 1
    t = torch.tensor([400.0, 400.0])
    res = []
    for m in (m16, m32):
        gm = CLIPGrads(scale=100.0, clip_models=[m], cutout_kwargs=dict(cutn=4), cutout_batches=1)
        assert gm.cutouts[0].cut_size == R
        gm.set_targets([EmbeddingPrompt(e0, 1.0)])
        torch.manual_seed(21)
        res.append(gm(img, t).clone())
        m.visual._destroy()
    a, b = res
    print(f"{name}: bf16 vs f32 gradient cosine {cos(a, b):.5f}, max |g| {float(b.abs().max()):.3e}")
    assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()) and float(a.abs().max()) > 0 and float(b.abs().max()) > 0
    assert cos(a, b) >= 0.98


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_768_wide_text_tower_matches_the_restatement(dt):
    """The text half of the ViT-L/14 checkpoints (width 768, 12 heads, embedding 768) at its real shape against the float32 CPU
    restatement of CLIP.encode_text that tests/test_gpu_clip_text.py uses, at that test's bars."""
    import test_gpu_clip_text as TT
    from maua_amd import clip as CL
    cfg = CL.TEXT_CONFIGS["ViT-L/14"]
    assert cfg == CL.TEXT_CONFIGS["ViT-L/14@336px"]
    p = TT.text_params(cfg, seed=768)
    tt = TT.tower(cfg, dt, p)
    tokens = TT.make_tokens(cfg, [cfg[0] - 1, 3, 17, 1, cfg[0] // 2], seed=5)
    got = tt(tokens)
    want = TT.encode_text_ref(p, cfg, tokens)
    print(f"768-wide text tower {dt}: rel {TT.rel(got, want):.3e} cos {TT.cos(got, want):.6f}")
    assert tuple(got.shape) == (5, 768)
    if dt == torch.float32:
        assert TT.rel(got, want) <= 1e-4
    else:
        assert TT.cos(got, want) >= 0.999
