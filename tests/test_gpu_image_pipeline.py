"""GPU checks of the multi-resolution image pipeline: every image operator of csrc/image_ops.hip through the C ABI against g37 (the
reference's own functions) or tests/image_pipeline_ref.py (restated torchvision / resize_right, parity unpinned) at the exact-f32 bar,
match_histogram at four times the reference's own float32-vs-float64 spread, and the pipeline on a small random-init UNet against
the same library calls made by hand, bit for bit.  Nothing here retries: a failing step fails the test."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import image_pipeline_ref as H  # noqa: E402
from oracle import diffusion as OD  # noqa: E402
from test_image_pipeline_host import PIPE_CASES, Stub, match_histogram_bar, run_pipeline_case  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
BAR = 2e-5          # the project's exact-f32 bar
CHILD_TIMEOUT = 900  # seconds: the command-line run builds a full-size random-init network on the host first


@pytest.fixture(scope="module")
def g37(golden):
    g = golden("g37_image_pipeline")
    g["meta"] = json.loads(str(g["meta_json"]))
    return g


def err(a, b):
    return float((a.detach().cpu().double() - b.detach().cpu().double()).abs().max())


@pytest.mark.parametrize("kernel", ["lanczos3", "cubic"])
@pytest.mark.parametrize("shape,out", [((1, 3, 64, 64), (128, 192)), ((2, 3, 96, 80), (64, 48)), ((1, 3, 37, 53), (64, 53)),
                                       ((1, 3, 128, 192), (64, 192)), ((1, 3, 300, 20), (17, 64))])
def test_resize_matches_the_restated_resize_right(kernel, shape, out):
    import maua_amd.image as I
    x = torch.rand(shape, generator=torch.Generator().manual_seed(5)) * 2 - 1
    want = H.resize(x, out_shape=out, interp_method=getattr(H, kernel))
    got = I.resize(x, out, interp_method=kernel)
    e = err(got, want)
    print(f"resize {kernel} {shape[2:]} -> {out}: {e:.3e}")
    assert tuple(got.shape) == (*shape[:2], *out) and e <= BAR
    assert torch.equal(I.resize(x, out, interp_method=kernel), got)                  # bit-identical from run to run
    acc = I.resize(x, out, interp_method=kernel, out=got.clone(), accumulate=True, add=-1.0)
    assert torch.equal(acc, (got + got) + (-1.0))                                   # (out + resized) + add, each rounded once


def test_destitch_restitch_against_the_reference(g37):
    import maua_amd.image as I
    for name in ("s23", "s33"):
        m = g37["meta"][name]
        img = g37[f"{name}_img"]
        tiles = I.destitch(img, m["T"])
        assert torch.equal(tiles.cpu(), g37[f"{name}_tiles"])
        e1 = err(I.restitch(g37[f"{name}_rnd"], m["H"], m["W"]), g37[f"{name}_rnd_out"])
        back = I.restitch(tiles, m["H"], m["W"])
        e2, e3 = err(back, g37[f"{name}_back"]), err(back, img)
        print(f"restitch {name}: random tiles {e1:.3e}, destitched {e2:.3e}, partition of unity {e3:.3e}")
        assert max(e1, e2, e3) <= BAR
        assert torch.equal(I.restitch(tiles, m["H"], m["W"]), back)
    # a batch of two images: tile-major, then batch (torch.cat of the slices)
    x = torch.rand(2, 3, 128, 192, generator=torch.Generator().manual_seed(6))
    t = I.destitch(x, 64)
    ys, xs = I.tile_origins(128, 64), I.tile_origins(192, 64)
    assert torch.equal(t.cpu(), torch.cat([x[..., a:a + 64, b:b + 64] for a in ys for b in xs]))
    big = torch.rand(1, 3, 192, 256, generator=torch.Generator().manual_seed(7)) * 2 - 1
    assert err(I.restitch(I.destitch(big, 128), 192, 256), big) <= BAR


@pytest.mark.parametrize("strength", [0.0, 0.5, 1.0, 2.5])
def test_sharpen_matches_the_restated_adjust_sharpness(strength):
    import maua_amd.image as I
    x = torch.rand(2, 3, 37, 300, generator=torch.Generator().manual_seed(8)) * 2.4 - 1.2
    e = err(I.sharpen(x, strength), H.sharpen(x, strength))
    print(f"sharpen {strength}: {e:.3e}")
    assert e <= BAR
    tiny = torch.rand(1, 3, 2, 5) * 3 - 1.5                    # no interior: returned as it is, values outside [-1, 1] included
    assert err(I.sharpen(tiny, 2.0), H.sharpen(tiny, 2.0)) <= BAR and float(I.sharpen(tiny, 2.0).max()) > 1.0


def test_perlin_against_the_reference(g37):
    import maua_amd.image as I
    for name in ("pc", "pg"):
        m = g37["meta"][name]
        grads = [g37[f"{name}_grad{k:02d}"] for k in range(m["n_grads"])]
        img, raw = I.create_perlin_noise(list(g37[f"{name}_octaves"].numpy()), m["width"], m["height"], m["grayscale"], gradients=grads,
                                         return_raw=True)
        want_raw = g37[f"{name}_raw"].reshape(raw.shape)
        e_raw, e_img = err(raw, want_raw), err(img, g37[f"{name}_img"])
        print(f"perlin {name}: perlin_ms {e_raw:.3e}, image {e_img:.3e}")
        assert e_raw <= BAR and e_img <= BAR
    g = g37["perlin_single_grad"]
    _, raw = I.create_perlin_noise([1.0, 0.0], 3, 2, True, gradients=[g, torch.zeros(2, 7, 5)], return_raw=True)
    assert err(raw[0] - 0.5, g37["perlin_single"]) <= BAR          # perlin(3, 2, scale 4) alone
    torch.manual_seed(11)
    a = I.initialize_image("perlin", (64, 128))
    torch.manual_seed(11)
    b = I.initialize_image("perlin", (64, 128))
    assert tuple(a.shape) == (1, 3, 64, 128) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    assert -1.0 - 1e-3 <= float(a.min()) and float(a.max()) <= 1.0 + 1e-3 and float(a.std()) > 0.05


def test_match_histogram_against_the_reference(g37):
    """Bar: four times the spread between the reference's float32 result and the same function in float64 on the fixture's inputs
    (measured here from the fixture; both numbers are recorded in DESIGN §5d)."""
    import maua_amd.image as I
    spread, bar = match_histogram_bar(g37)
    got = I.match_histogram(g37["mh_target"], g37["mh_source"], noise=(g37["mh_noise_t"], g37["mh_noise_s"]))
    e32, e64 = err(got, g37["mh_out32"]), err(got, g37["mh_out64"])
    print(f"match_histogram: vs reference f32 {e32:.3e}, vs reference f64 {e64:.3e}; reference f32 vs f64 {spread:.3e}, bar {bar:.3e}")
    assert e32 <= bar
    assert torch.equal(I.match_histogram(g37["mh_target"], g37["mh_source"], noise=(g37["mh_noise_t"], g37["mh_noise_s"])), got)
    # the library's own Philox perturbation: same statistics, clamped to the source's range, finite
    own = I.match_histogram(g37["mh_target"], g37["mh_source"])
    assert err(own, got) < 0.05 and float(own.min()) >= float(g37["mh_source"].min()) and float(own.max()) <= float(g37["mh_source"].max())
    # its key: drawn from torch's host generator (torch.manual_seed fixes a run, successive calls differ), or given
    torch.manual_seed(5)
    a1, a2 = I.match_histogram(g37["mh_target"], g37["mh_source"]), I.match_histogram(g37["mh_target"], g37["mh_source"])
    torch.manual_seed(5)
    b1 = I.match_histogram(g37["mh_target"], g37["mh_source"])
    assert torch.equal(a1, b1) and not torch.equal(a1, a2)
    assert torch.equal(I.match_histogram(g37["mh_target"], g37["mh_source"], seed=9), I.match_histogram(g37["mh_target"], g37["mh_source"], seed=9))
    # the RuntimeError fall-back: a non-finite target leaves the input (clamped), as the reference does
    bad = g37["mh_target"].clone()
    bad[0, 0, 0, 0] = float("nan")
    fb = I.match_histogram(bad, g37["mh_source"])
    lo, hi = float(g37["mh_source"].min()), float(g37["mh_source"].max())
    assert torch.equal(fb.cpu()[1], bad[1].clamp(lo, hi))


@pytest.mark.parametrize("name", PIPE_CASES)
def test_pipeline_with_a_stub_processor_against_the_reference(g37, name):
    """the reference's whole MultiResolutionDiffusionProcessor.forward (recorded around a stub processor) with the real device operators"""
    import maua_amd.image as I
    stub = Stub()
    stub.device = "cuda"
    res = run_pipeline_case(I, g37, name, stub)
    c = g37["meta"][f"pipe_{name}"]
    assert stub.calls == c["calls"] and list(res.shape) == c["shape"] and res.is_cuda
    e = err(res[:, :, 1::3, ::3], g37[f"pipe_{name}"])
    print(f"pipeline {name}: {e:.3e}")
    assert e <= BAR


SMALL = dict(image_size=64, model_channels=32, num_res_blocks=1, attention_resolutions=(16, 8), channel_mult=(1, 2, 2), num_head_channels=32)


def small_guided(sampler="plms", timesteps=20):
    from maua_amd.diffusion import GuidedDiffusion, SpacedDiffusion, UNetModel, space_timesteps
    cfg = OD.unet_config(**SMALL)
    p = OD.init_unet_params(cfg, torch.Generator().manual_seed(0))
    net = UNetModel(image_size=cfg["image_size"], in_channels=3, model_channels=cfg["model_channels"], out_channels=cfg["out_channels"],
                    num_res_blocks=cfg["num_res_blocks"], attention_resolutions=cfg["attention_ds"], channel_mult=cfg["channel_mult"],
                    num_head_channels=cfg["num_head_channels"], use_scale_shift_norm=True, resblock_updown=True, dtype=torch.float32)
    net.load_state_dict(p)
    sd = SpacedDiffusion(space_timesteps(1000, str(timesteps)), OD.linear_betas(1000), rescale_timesteps=True)
    return GuidedDiffusion([], sampler=sampler, timesteps=timesteps, model=net, diffusion=sd)


def test_one_tile_schedule_is_a_direct_sampler_call():
    import maua_amd.image as I
    gd = small_guided()
    torch.manual_seed(21)
    got = I.image_sample(init="random", sizes=[(64, 64)], skips=[0.4], super_res=None, diffusion=gd, stitch=True)
    torch.manual_seed(21)
    img = torch.randn((1, 3, 64, 64)).to("cuda")
    want = gd(img, [], 0.4, verbose=False)
    assert torch.equal(got, want) and bool(torch.isfinite(got).all())


def test_two_scale_stitched_pipeline_is_the_same_library_calls_by_hand():
    import maua_amd.image as I
    gd = small_guided()

    def run():
        torch.manual_seed(22)
        return I.image_sample(init="random", sizes=[(64, 64), (128, 192)], skips=[0.0, 0.5], super_res=None, diffusion=gd, stitch=True,
                              tile_size=64, max_batch=4, sharpness=1.5)
    a, b = run(), run()
    assert tuple(a.shape) == (1, 3, 128, 192) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    torch.manual_seed(22)
    img = torch.randn((1, 3, 64, 64)).to("cuda")
    img = I.sharpen(gd(img, [], 0.0, verbose=False), 1.5)
    img = I.destitch(I.resize(img, (128, 192), interp_method="lanczos3"), 64)
    assert img.shape[0] == 12
    img = torch.cat([gd(t, [], 0.5, verbose=False) for t in img.split(4)])
    img = I.sharpen(I.restitch(img, 128, 192), 1.5)
    assert torch.equal(a, img)


def test_realesrgan_between_scales_and_its_checkpoint_check():
    """super_res = a RealESRGAN name: the up-scaler is built when the run is set up (a missing checkpoint raises before any sampling),
    and with random-init weights the x 4 up-scale + lanczos3 resize run between the scales."""
    import maua_amd.image as I
    gd = small_guided()
    calls = []
    gd.register_forward_pre_hook(lambda *_: calls.append(1))
    I._upscalers.clear()
    with pytest.raises(FileNotFoundError):
        I.image_sample(init="random", sizes=[(64, 64), (128, 128)], skips=[0.0, 0.5], super_res="x4plus-anime", diffusion=gd)
    assert not calls
    torch.manual_seed(23)
    out = I.image_sample(init="random", sizes=[(64, 64), (128, 128)], skips=[0.0, 0.5], super_res="x4plus-anime", diffusion=gd,
                         guided_kwargs=dict(allow_random_init=True))
    assert tuple(out.shape) == (1, 3, 128, 128) and bool(torch.isfinite(out).all()) and len(calls) == 2
    # by hand: the same calls
    torch.manual_seed(23)
    img = gd(torch.randn((1, 3, 64, 64)).to("cuda"), [], 0.0, verbose=False)
    img = I.upscale_image(img.add(1).div(2), "x4plus-anime").mul(2).sub(1)
    assert tuple(img.shape) == (1, 3, 256, 256)
    assert torch.equal(out, gd(I.resize(img, (128, 128), interp_method="lanczos3"), [], 0.5, verbose=False))
    I._upscalers.clear()


def test_join_batches_is_torch_cat():
    import maua_amd.image as I
    parts = [torch.rand(4, 3, 8, 8, device="cuda"), torch.rand(4, 3, 8, 8, device="cuda"), torch.rand(1, 3, 8, 8, device="cuda")]
    assert torch.equal(I.join_batches(parts), torch.cat(parts))
    assert torch.equal(I.join_batches([parts[0].transpose(2, 3), parts[1]]), torch.cat([parts[0].transpose(2, 3), parts[1]]))


def test_unsupported_sizes_and_text_prompts_are_refused_up_front():
    import maua_amd.image as I
    from maua_amd.diffusion import get_diffusion_model
    gd = small_guided()
    calls = []
    gd.register_forward_pre_hook(lambda *_: calls.append(1))
    with pytest.raises(ValueError, match="tile size 66"):
        I.MultiResolutionDiffusionProcessor()(gd, "random", schedule={(64, 64): 0.0, (128, 128): 0.5}, tile_size=66, stitch=True, verbose=False)
    assert not calls                                                   # refused before any sampling
    with pytest.raises(ValueError, match="text encoder"):
        get_diffusion_model("guided", clip_scale=100.0, text="a prompt", clip_models=[object_with_visual()],
                            guided_kwargs=dict(model=gd.model, diffusion=gd.diffusion, allow_random_init=True))


def object_with_visual():
    from maua_amd import clip as CL
    vt = CL.load("ViT-B/32", allow_random_init=True, text_tower=False)[0]
    assert vt.text is None and vt.text_encoder is None
    return vt


def test_command_line_writes_a_png(tmp_path):
    """``python -m maua.diffusion.image`` in a child process (random-init weights: there are no checkpoints), under its own time limit."""
    from PIL import Image
    env = dict(os.environ, MAUA_ALLOW_RANDOM_INIT="1", PYTHONPATH=str(ROOT))
    cmd = [sys.executable, "-m", "maua.diffusion.image", "--diffusion", "guided", "--init", "perlin", "--sizes", "128,128", "384,256",
           "--skips", "0", "0.6", "--timesteps", "10", "--stitch", "--tile-size", "128", "--super-res", "None", "--out-dir", str(tmp_path)]
    r = subprocess.run(cmd, env=env, cwd=str(ROOT), capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    pngs = sorted(tmp_path.glob("guided_perlin_*0.png"))
    assert len(pngs) == 1
    assert Image.open(pngs[0]).size == (384, 256)
