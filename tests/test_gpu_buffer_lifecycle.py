"""The grow paths of the handles' device buffers (csrc/devbuf.h: one owner per buffer, workspace sets carved from one block): each test
walks ONE handle small -> large -> small and requires every result to equal, bit for bit, what a FRESH handle gives at that shape - the
large call moves or re-places every workspace, the second small call runs in the large call's block.  A piece placed short of its size,
a capacity that outlived its buffer or a stale pointer changes bits here.  The handles whose own test files already walk a grow path
(the perceptor, the up-scalers, the synthesis forward, the UNet arena, the context scratch) are covered there.

The image tower's buffer generation (maua_clip::epoch) has no reader in the C ABI - the sampler compares it inside the library before
it replays a captured loop - so it is observed the way tests/test_gpu_grads.py observes the perceptor's: a captured guided loop, a
larger and then a smaller call on the same tower in between, and the loop's result after each
(test_captured_loop_follows_the_towers_buffer_generation)."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_gpu_clip import SMALL, _targets, _tower  # noqa: E402
from test_gpu_clip_text import SMALL_CFGS, make_tokens, text_params, tower  # noqa: E402
from test_synth_vjp_host import RES, W_DIM, make_net  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from oracle import clip as OC, diffusion as OD, stylegan2 as OS  # noqa: E402

pytestmark = pytest.mark.gpu


def same(got, want):
    got, want = (list(v) if isinstance(v, (list, tuple)) else [v] for v in (got, want))
    return len(got) == len(want) and all(torch.equal(a, b) for a, b in zip(got, want))


def walk(make, run, shapes):
    """``run(handle, shape)`` on one handle over ``shapes`` against a fresh handle's result at each distinct shape (computed once)."""
    fresh = {}
    for s in shapes:
        if s not in fresh:
            fresh[s] = run(make(), s)
    h = make()
    for i, s in enumerate(shapes):
        assert same(run(h, s), fresh[s]), (i, s)


def test_secondary_model_forward_and_input_gradient():
    """B = 1 at 32 x 32 (the smallest size at which the deepest level still has a pixel), B = 2 at 64 x 64, B = 1 at 32 x 32 again."""
    from maua_amd.diffusion import SecondaryDiffusionImageNet2
    p = OD.secondary_random_params(3)

    def make():
        net = SecondaryDiffusionImageNet2(dtype=torch.float32)
        net.load_state_dict(p)
        return net

    def run(net, shape):
        B, S = shape
        g = torch.Generator().manual_seed(S)
        x, t, gv = torch.randn(B, 3, S, S, generator=g), torch.rand(B, generator=g), torch.randn(B, 3, S, S, generator=g)
        out = net(x, t)
        return [out.v.clone(), out.pred.clone(), out.eps.clone(), net.vjp(gv).clone()]

    walk(make, run, [(1, 32), (2, 64), (1, 32)])


def test_synthesis_gradient_with_the_noise_gradient_in_the_middle():
    """latent_grad at B = 1, 3, 1 on the smallest network of test_gpu_synth_vjp.py; the middle call also asks the kept forward for the
    gradient to the noise maps, which allocates the per-group channel sums (npart) on their own."""
    from maua_amd.grad import GradModule
    from maua_amd.stylegan2 import SynthesisNetwork, latent_grad
    from test_synth_vjp_host import CBASE, CMAX
    p, _, _, _ = make_net(5)

    class TargetGrads(GradModule):
        def __init__(self, target):
            super().__init__(1.0)
            self.target = target

        def forward(self, img, t):
            return img - self.target

    def make():
        net = SynthesisNetwork(W_DIM, RES, 3, channel_base=CBASE, channel_max=CMAX, dtype=torch.float32)
        net.load_state_dict({k: v.float() for k, v in p.items()})
        net.keep_features(True)   # (stays on, so that the kept forward outlives latent_grad)
        return net

    def run(net, shape):
        B, with_noise = shape
        g = torch.Generator().manual_seed(B)
        ws = torch.randn(B, OS.num_ws(RES), W_DIM, generator=g).cuda()
        noise = [torch.randn(B, 1, r, r, generator=g).cuda() for _, _, _, r, _ in OS.layer_list(RES, CBASE, CMAX)]
        critic = TargetGrads(torch.randn(B, 3, RES, RES, generator=g).cuda())
        g_ws, img = latent_grad(None, net, ws, critic, space="w", noise=noise)
        out = [g_ws.clone(), img.clone()]
        if with_noise:
            g_ws2, g_noise = net.vjp(img - critic.target, noise=noise, noise_grad=True)
            out += [g_ws2.clone()] + [t.clone() for t in g_noise if t is not None]
        return out

    walk(make, run, [(1, False), (3, True), (1, False)])


def _clip_case(cutn):
    B, H, W = 2, 40, 48
    g = torch.Generator().manual_seed(100 + cutn)
    img = (torch.rand(B, 3, H, W, generator=g) * 2 - 1).cuda()
    torch.manual_seed(cutn)
    rects = np.ascontiguousarray(np.asarray([OC.cutout_rects(H, W, 32, cutn, OC.maua_cutouts_pow(620))], dtype=np.int32))
    return img, rects, B, H, W


def test_clip_guidance_as_the_cutout_count_grows_and_shrinks():
    """maua_clip_guide_grad on the smallest tower of test_gpu_clip.py with cutn 2, 5, 2: the tower's workspace set and the cutout
    scratch grow on the second call and are re-used by the third."""
    tgt, w = _targets(SMALL["output_dim"], 3, 4)
    tn, wn = np.ascontiguousarray(tgt.numpy()), np.ascontiguousarray(w.numpy())

    def make():
        vt, _ = _tower(SMALL, torch.float32, seed=1)
        L.check(L.lib().maua_clip_set_targets(vt._handle(), tn.ctypes.data_as(C.c_void_p), wn.ctypes.data_as(C.c_void_p), 1, 3, None, 0))
        return vt

    def run(vt, cutn):
        img, rects, B, H, W = _clip_case(cutn)
        out = torch.empty_like(img)
        L.check(L.lib().maua_clip_guide_grad(vt._handle(), L.ptr(img), B, H, W, rects.ctypes.data_as(C.c_void_p), None, cutn, 1, C.c_float(150.0),
                                             C.c_float(0.0), L.ptr(out)))
        losses = torch.empty(cutn * B, device="cuda")
        L.check(L.lib().maua_clip_last_image_losses(vt._handle(), cutn * B, L.ptr(losses)))
        return [out, losses]

    walk(make, run, [2, 5, 2])


def test_clip_guidance_with_augmented_cutouts_as_the_cutout_count_grows_and_shrinks():
    """The same through maua_clip_guide_grad_aug (CLIPGrads with augmented "dango" cutouts: the module draws rectangles, augmentation
    records and noise keys from torch's seeded generators): cutn 2, 5, 2 on one tower."""
    from maua_amd.clip import CLIPImageModel
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    emb = torch.randn(2, SMALL["output_dim"], generator=torch.Generator().manual_seed(13))

    def make():
        return _tower(SMALL, torch.float32, seed=2)[0]

    def run(vt, cutn):
        m = CLIPGrads(scale=120.0, cutouts="dango", cutout_kwargs=dict(cutn=cutn, skip_augs=False), cutout_batches=1, clip_models=[CLIPImageModel(vt)])
        m.set_targets([EmbeddingPrompt(emb[0], 1.0), EmbeddingPrompt(emb[1], 0.5)])
        B, S = 2, 48
        img = torch.rand(B, 3, S, S, generator=torch.Generator().manual_seed(cutn)) * 2 - 1
        torch.manual_seed(21 + cutn)
        grad = m.forward(img, torch.tensor([300.0] * B))
        assert m.last_aug_plan[0] is not None, "the call did not take the augmented entry point"
        return grad.clone()

    walk(make, run, [2, 5, 2])


def test_captured_loop_follows_the_towers_buffer_generation():
    """The short text-guided loop of tests/test_gpu_clip.py as one hipGraph, three times on the same inputs.  Between the first and the
    second a direct maua_clip_guide_grad with more cutouts (12 against the loop's 8) regrows the tower's workspace set and the cutout
    scratch, which moves every piece the captured launches point into: the tower's generation has to move, or the second run replays
    launches into memory that is gone and cannot give the first run's bits.  Between the second and the third a call with fewer cutouts
    (2) fits what is there: no buffer moves.  All three results are equal bit for bit and the loop is a graph each time.  (Whether a
    run replayed or recaptured has no observer outside the library, and a direct call also re-fixes the tower's cutout group size,
    which moves the generation on its own account.)

    Not stable, and not from the buffers: on one MI355X, alone in fresh processes, this test failed 1 time in 10 on this library and 1
    time in 20 on the library as it was before the owners (same source of the test), each time at "after the tower's workspaces
    grew", with finite results; a probe of the same sequence gave equal bits in all of four runs on both.  The captured text-guided
    loop does not always repeat its bits - test_gpu_clip_vitl.py's graph-against-step-by-step test fails about 1 run in 30 on both
    libraries too - which is a defect of the guided loop that is older than this test and not found yet."""
    from maua_amd.clip import CLIPImageModel
    from maua_amd.diffusion import GuidedDiffusion, SecondaryDiffusionImageNet2, SpacedDiffusion, UNetModel, space_timesteps
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    vt, _ = _tower(SMALL, torch.bfloat16, seed=2)
    E = SMALL["output_dim"]
    g = torch.Generator().manual_seed(3)
    net = UNetModel(image_size=64, in_channels=3, model_channels=32, out_channels=6, num_res_blocks=1, attention_resolutions=(4, 8),
                    channel_mult=(1, 2, 2), num_head_channels=32, use_scale_shift_norm=True, resblock_updown=True, dtype=torch.bfloat16,
                    generator=g)
    sec = SecondaryDiffusionImageNet2(dtype=torch.float32, generator=g, exact=False)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim6"), OD.linear_betas(1000), rescale_timesteps=True)
    prompts = [EmbeddingPrompt(torch.randn(E, generator=g)), EmbeddingPrompt(torch.randn(E, generator=g), 0.5)]
    gm = CLIPGrads(scale=500.0, clip_models=[CLIPImageModel(vt)], cutout_kwargs=dict(cutn=8), cutout_batches=2, clamp_gradient=0.05)
    gd = GuidedDiffusion([gm], timesteps=6, model=net, diffusion=sd, speed="fast", secondary_model=sec)
    gd.use_graph = True

    def loop():
        gg = torch.Generator().manual_seed(40)
        x0, nz = torch.randn(2, 3, 64, 64, generator=gg), torch.randn(2, 3, 64, 64, generator=gg)
        torch.manual_seed(90)
        out = gd.run(x0, prompts, 5, 6, noise=nz).clone()
        assert net.guided_graph_active() and bool(torch.isfinite(out).all())
        return out

    def direct(cutn):
        img, rects, B, H, W = _clip_case(cutn)
        out = torch.empty_like(img)
        L.check(L.lib().maua_clip_guide_grad(vt._handle(), L.ptr(img), B, H, W, rects.ctypes.data_as(C.c_void_p), None, cutn, 1, C.c_float(150.0),
                                             C.c_float(0.0), L.ptr(out)))
        torch.cuda.synchronize()

    first = loop()
    direct(12)
    assert torch.equal(loop(), first), "after the tower's workspaces grew"
    direct(2)
    assert torch.equal(loop(), first), "after a smaller call on the tower"


def test_text_tower_as_the_batch_grows_and_shrinks():
    """1, 3, 1 sequences through one text tower."""
    cfg = SMALL_CFGS[0]
    p = text_params(cfg, 7)
    walk(lambda: tower(cfg, torch.float32, p), lambda tt, n: tt(make_tokens(cfg, [5, 20, 76][:n], seed=n)).clone(), [1, 3, 1])


def test_colormatch_guide_as_the_batch_grows_and_shrinks():
    """The ColorMatch grad module as a library object (maua_guide_grad) at B = 1, 3, 1."""
    from maua_amd.grad import GUIDE_COLORMATCH, ColorMatchGrads, _Guide
    gen = torch.Generator().manual_seed(41)
    target = ColorMatchGrads(scale=1e4).histogram(torch.rand(1, 3, 32, 32, generator=gen))

    def run(g, B):
        img = (torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(B)) * 2 - 1).cuda()
        out = torch.empty_like(img)
        L.check(L.lib().maua_guide_grad(g.h, L.ptr(img), B, 32, 32, L.ptr(out)))
        return out

    walk(lambda: _Guide(GUIDE_COLORMATCH, [target], targets=[target], strides=[0], scale=1e4, nbins=255, sat=1), run, [1, 3, 1])


def test_cellular_automaton_as_the_batch_grows_and_shrinks():
    """Two steps of one automaton at B = 1, 3, 1: the second state buffer grows with the batch."""
    from maua_amd import nca
    first = nca.CA(12, 96, seed=3)
    sd = {k: v.clone() for k, v in first.state_dict().items()}
    sd["w2.weight"] = 0.1 * torch.randn(sd["w2.weight"].shape, generator=torch.Generator().manual_seed(3))   # (initialised to zero: no update)

    def make():
        ca = nca.CA(12, 96, seed=3)
        ca.load_state_dict(sd)
        return ca.cuda()

    def run(ca, B):
        x = torch.rand(B, 12, 16, 32, generator=torch.Generator().manual_seed(B)).cuda()
        return ca.step(x, n=2, step0=0).clone()

    walk(make, run, [1, 3, 1])


def test_farneback_handle_created_again():
    """create, run, destroy, create, run at the smallest plan (15 x 15): the second handle gives what the first gave."""
    import maua_amd.flow as F
    g = torch.Generator().manual_seed(15)
    a, b = torch.rand(3, 15, 15, generator=g), torch.rand(3, 15, 15, generator=g)
    got = []
    for _ in range(2):
        fb = F.Farneback(15, 15)
        got.append([f.clone() for f in fb.pair(a, b)])
        fb.close()
    assert same(got[0], got[1])


def test_video_feature_handle_created_again():
    """create, push, destroy, create, push: the second analyzer gives what the first gave."""
    from maua_amd.video_features import VideoAnalyzer
    frames = torch.randint(0, 256, (3, 37, 53, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(37)).cuda()
    got = []
    for _ in range(2):
        an = VideoAnalyzer(37, 53, bins=32, max_batch=4)
        f = an.push(frames).features()
        got.append([f[k].clone() for k in sorted(f)])
        an.close()
    assert same(got[0], got[1])
