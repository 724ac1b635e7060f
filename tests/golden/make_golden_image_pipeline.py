"""Generate tests/golden/g37_image_pipeline.npz by IMPORTING the reference (authoring container only, like make_golden.py; the tests
consume the committed .npz).  This script holds no reference code: it runs the reference's own

  * ``destitch`` / ``restitch`` (maua/ops/image.py:15-62) on odd sizes, overtile = 1, 2 x 3 and 3 x 3 tile grids;
  * ``match_histogram`` (:105-173) with ``torch.randn`` recorded, in float32 and - the same function, same inputs and noise - float64;
  * ``get_start_steps``, ``round64``, ``build_output_name(unique=False)`` (maua/diffusion/image.py:30-58);
  * ``perlin`` / ``perlin_ms`` / ``create_perlin_noise`` (maua/ops/noise.py:94-132) with the gradient draws recorded;
  * ``MultiResolutionDiffusionProcessor.forward`` (:132-214) around a stub processor that records every call (input shape, t_start,
    prompt classes) and returns a fixed affine function of its input.

torchvision and resize_right are absent from the reference tree and the image: ``adjust_sharpness`` / ``to_pil_image`` / ``to_tensor``
and ``resize`` with its kernels are the restatements of tests/image_pipeline_ref.py.  The processors other than "guided" and the
up-scaler module import packages that are absent too; their modules are stubbed, none of the captured functions calls into them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_image_pipeline.py
"""
import json
import sys
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
import make_golden as MG  # noqa: E402
import image_pipeline_ref as H  # noqa: E402

MG.ABSENT.update({"ldm", "glide_text2im", "transformers", "omegaconf", "pytorch_lightning", "k_diffusion", "einops", "requests", "tqdm",
                  "scipy", "timm", "basicsr", "realesrgan", "guided_diffusion", "taming", "dalle_pytorch", "encoding", "ftfy", "regex"})


class Recorder:
    """torch.randn stand-in: the real draw (without the device argument), kept."""

    def __init__(self, dtype=None):
        self.real, self.log, self.dtype = torch.randn, [], dtype

    def __call__(self, *a, **k):
        k.pop("device", None)
        t = self.real(*a, **k)
        self.log.append(t.clone())
        return t if self.dtype is None else t.to(self.dtype)


class Replay:
    def __init__(self, log, dtype):
        self.log, self.dtype, self.i = log, dtype, 0

    def __call__(self, *a, **k):
        t = self.log[self.i].to(self.dtype)
        self.i += 1
        return t


def main():
    MG.import_reference()
    for m in ("maua.diffusion.processors.glid3xl", "maua.diffusion.processors.glide", "maua.diffusion.processors.latent",
              "maua.diffusion.processors.stable", "maua.super.image.single"):
        sys.modules[m] = MagicMock(name=m)
    import maua.ops.image as RI
    import maua.ops.noise as RN
    import maua.diffusion.image as RD
    from maua.diffusion.processors.base import BaseDiffusionProcessor
    out, meta = {}, {}
    g = torch.Generator().manual_seed(3700)

    # ---- destitch / restitch
    for name, (Hh, Ww, T) in {"s23": (29, 45, 17), "s33": (41, 39, 15)}.items():
        img = torch.rand(1, 3, Hh, Ww, generator=g) * 2 - 1
        tiles = RI.destitch(img, T)
        rnd = torch.rand(tiles.shape, generator=g) * 2 - 1
        out[f"{name}_img"], out[f"{name}_tiles"] = img, tiles
        out[f"{name}_back"] = RI.restitch(tiles, Hh, Ww)
        out[f"{name}_rnd"], out[f"{name}_rnd_out"] = rnd, RI.restitch(rnd, Hh, Ww)
        meta[name] = dict(H=Hh, W=Ww, T=T, n_tiles=int(tiles.shape[0]))

    # ---- match_histogram: smooth-ish images with mixed channels (covariance condition number well below 1e4, checked by the tests)
    mix_t = torch.tensor([[0.5, 0.2, 0.1], [0.1, 0.4, 0.2], [0.05, 0.1, 0.45]])
    mix_s = torch.tensor([[0.3, 0.1, 0.3], [0.2, 0.5, 0.0], [0.1, 0.1, 0.3]])
    tgt = torch.einsum("dc,bchw->bdhw", mix_t, torch.rand(2, 3, 24, 20, generator=g) * 2 - 1)
    src = torch.einsum("dc,bchw->bdhw", mix_s, torch.rand(2, 3, 16, 18, generator=g) * 2 - 1) + 0.1
    torch.manual_seed(3701)
    rec = Recorder()
    torch.randn = rec
    try:
        o32 = RI.match_histogram(tgt, src, mode="avg")
    finally:
        torch.randn = rec.real
    torch.randn = Replay(rec.log, torch.float64)
    try:
        o64 = RI.match_histogram(tgt.double(), src.double(), mode="avg")
    finally:
        torch.randn = rec.real
    # the reference draws in its (b, w, h, c) layout: back to image layout; per target frame one target and one source draw
    out["mh_target"], out["mh_source"], out["mh_out32"], out["mh_out64"] = tgt, src, o32, o64
    out["mh_noise_t"] = torch.cat([rec.log[2 * b] for b in range(2)]).permute(0, 3, 2, 1).contiguous()
    out["mh_noise_s"] = torch.cat([rec.log[2 * b + 1] for b in range(2)]).permute(0, 3, 2, 1).contiguous()
    assert len(rec.log) == 4
    out["mh_identity"] = RI.match_histogram(tgt, src, mode="False")

    # ---- small pure functions
    class D:
        original_num_steps = 1000
        timestep_map = list(range(0, 1000, 20))
    skips = [0.0, 0.3, 0.5, 0.75, 0.98]
    out["start_steps_skips"], out["start_steps"] = np.array(skips), RD.get_start_steps(skips, D())
    meta["round64"] = [[x, RD.round64(x)] for x in (1, 31, 32, 33, 95, 96, 97, 500, 512, 544)]
    meta["width_height"] = [["640,384", list(RD.width_height("640,384"))]]
    meta["output_names"] = [[kw, RD.build_output_name(unique=False, **kw)] for kw in (
        dict(), dict(text="a red fox"), dict(init="in/start.png", style="s/van gogh.jpg"),
        dict(init="perlin", style="a/b.png", text="x y", image="c/d.e.png"))]

    # ---- perlin
    RN.perlin.__defaults__ = (10, "cpu")
    for name, (octs, w, h, gray) in {"pc": ([1.0, 0.5, 0.25], 2, 2, False), "pg": ([0.5 * 1.5 ** -i for i in range(4)], 1, 3, True)}.items():
        torch.manual_seed(3702)
        rec = Recorder()
        torch.randn = rec
        try:
            raw = RN.perlin_ms(octs, w, h, gray)
        finally:
            torch.randn = rec.real
        RN.to_pil_image, RN.to_tensor = H.to_pil_image, H.to_tensor
        torch.randn = Replay(rec.log, torch.float32)
        try:
            full = RN.create_perlin_noise(octs, w, h, gray)
        finally:
            torch.randn = rec.real
        out[f"{name}_raw"], out[f"{name}_img"], out[f"{name}_octaves"] = raw, full, np.array(octs, dtype=np.float64)
        for k, t in enumerate(rec.log):
            out[f"{name}_grad{k:02d}"] = t.reshape(t.shape[:3])
        meta[name] = dict(width=w, height=h, grayscale=gray, n_grads=len(rec.log))
    p1 = Recorder()
    torch.randn = p1
    try:
        torch.manual_seed(3703)
        out["perlin_single"] = RN.perlin(3, 2, 4)
    finally:
        torch.randn = p1.real
    out["perlin_single_grad"] = p1.log[0].reshape(2, 4, 3)

    # ---- the whole MultiResolutionDiffusionProcessor.forward around a recording stub
    RD.resize, RD.lanczos3 = H.resize, H.lanczos3
    RD.tqdm = lambda x: x

    class Stub(BaseDiffusionProcessor if isinstance(BaseDiffusionProcessor, type) else torch.nn.Module):
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.image_size, self.device, self.calls = 64, "cpu", []

        def forward(self, img, prompts, t_start, verbose=True):
            self.calls.append(dict(shape=list(img.shape), t_start=float(t_start), prompts=[type(p).__name__ for p in prompts]))
            return img * 0.75 + 0.125

    def pre(x):
        return x * 0.5 - 0.1

    def post(x):
        return x.flip(-1) * 0.9

    # 128 x 192 in tiles of 64: 3 x 4 tiles.  Six tiles (2 x 3) with sizes that are multiples of 64 need 192 x 256 in tiles of 128: the
    # reference fades both axes over tile_size - ys[1] samples and fails when that exceeds half a tile on an axis with three tiles.
    big = {(64, 64): 0.0, (192, 256): 0.5}
    cases = {"tile64": dict(tile_size=64, max_batch=4, hooks=False), "six_b4": dict(tile_size=128, max_batch=4, hooks=False, schedule=big),
             "tile64_hooks": dict(tile_size=64, max_batch=4, hooks=True), "nostitch": dict(tile_size=64, max_batch=4, hooks=True, stitch=False)}
    for name, c in cases.items():
        torch.manual_seed(3704)
        stub = Stub()
        res = RD.MultiResolutionDiffusionProcessor()(
            diffusion=stub, init="random", text="a prompt", schedule=c.get("schedule", {(64, 64): 0.0, (128, 192): 0.5}),
            pre_hook=pre if c["hooks"] else None, post_hook=post if c["hooks"] else None, super_res_model=None,
            tile_size=c["tile_size"], stitch=c.get("stitch", True), max_batch=c["max_batch"], verbose=False)
        # the result is as large as the image and does not compress: every third sample of both axes and two sums are kept
        out[f"pipe_{name}"] = res[:, :, 1::3, ::3].contiguous()
        c = {k: v for k, v in c.items() if k != "schedule"}
        meta[f"pipe_{name}"] = dict(calls=stub.calls, shape=list(res.shape), sum=float(res.double().sum()), abs_sum=float(res.double().abs().sum()), **c)
    torch.manual_seed(3704)
    out["pipe_init"] = torch.randn((1, 3, 64, 64))

    # ---- the drop-in surface as data (as g25): argument names and default expressions, the command line's flags and help strings
    import ast
    tree = ast.parse(Path(RD.__file__).read_text())
    sigs, flags = {}, []
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in ("round64", "width_height", "build_output_name", "get_start_steps",
                                                                "initialize_image", "forward", "image_sample"):
            a = node.args
            d = [None] * (len(a.args) - len(a.defaults)) + [ast.unparse(x) for x in a.defaults]
            sigs[node.name] = [[x.arg, dv] for x, dv in zip(a.args, d)]
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: ast.unparse(k.value) for k in node.keywords if k.arg in ("default", "action", "nargs")}
            hlp = [k.value.value for k in node.keywords if k.arg == "help"]
            flags.append([node.args[0].value, kw, hlp[0] if hlp else None])
    meta["signatures"], meta["cli"] = sigs, flags

    out["meta_json"] = np.array(json.dumps(meta))
    MG.save("g37_image_pipeline", **{k: (v.float() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
