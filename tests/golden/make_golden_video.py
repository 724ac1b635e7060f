"""Generate tests/golden/g38_video_pipeline.npz by IMPORTING the reference (authoring container only, like make_golden_image_pipeline.py;
the tests consume the committed .npz).  This script holds no reference code: it runs the reference's own

  * ``flow_warp_map`` (maua/flow/lib.py:51-63) on 5 x 7 and 12 x 9 flows;
  * ``encode_mflo`` / ``decode_mflo`` (:18-48) round trips;
  * ``check_consistency`` (maua/flow/consistency.py:85-127) on three flow pairs - smooth, with a motion discontinuity, pointing out of the
    frame - with the restated 3-tap ``gaussian_blur`` of tests/flow_ref.py standing in for torchvision's;
  * ``VideoFlowDiffusionProcessor.forward`` (maua/diffusion/video.py:165-301) around a recording stub processor and stub frame / flow
    sources: the sequence of calls, the skip per call, the prompt kinds and the cache index of every insert, for turbo in {1, 3},
    wrap_around in {0, 2}, with and without first_frame_init, and hist_persist;
  * the signatures of ``video_sample`` / ``forward`` and the command line's flags, read with ``ast``.

decord, cv2, easydict, torchvision and npy_append_array are absent from the image: their modules are stubbed, and so are the neural flow
models' modules; none of the captured functions calls into them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_video.py
"""
import ast
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
import flow_ref as FR  # noqa: E402

MG.ABSENT.update({"ldm", "glide_text2im", "transformers", "omegaconf", "pytorch_lightning", "k_diffusion", "einops", "requests", "tqdm",
                  "scipy", "timm", "basicsr", "realesrgan", "guided_diffusion", "taming", "dalle_pytorch", "encoding", "ftfy", "regex",
                  "easydict", "mmflow", "mmcv"})

N_FRAMES, SIZE = 5, 64


def consistency_pairs():
    """Three flow pairs [1, H, W, 2] (forward, backward), 24 x 20: every class of check_consistency is populated over the three."""
    H, W = 20, 24
    y, x = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    g = torch.Generator().manual_seed(3800)
    wob = lambda: 0.3 * torch.sin(x * 0.37 + torch.rand((), generator=g) * 6) * torch.cos(y * 0.29 + torch.rand((), generator=g) * 6)
    pairs = {}
    # smooth: a gentle field and (nearly) its inverse
    bx, by = 1.3 + wob(), -0.8 + wob()
    pairs["smooth"] = (torch.stack([-bx + 0.05 * wob(), -by + 0.05 * wob()], -1)[None], torch.stack([bx, by], -1)[None])
    # a motion discontinuity: the right part moves, the left rests; the forward flow disagrees in a band
    step = (x > 11.5).float()
    bx, by = 2.6 * step + 0.1 * wob(), 0.1 * wob()
    fx = -2.6 * (x > 8.5).float() + 0.1 * wob()
    pairs["edge"] = (torch.stack([fx, 0.1 * wob()], -1)[None], torch.stack([bx, by], -1)[None])
    # pointing out of the frame
    bx, by = 5.4 + wob(), -3.3 + wob()
    pairs["out"] = (torch.stack([-bx, -by], -1)[None], torch.stack([bx, by], -1)[None])
    return pairs


def main():
    MG.import_reference()
    for m in ("maua.diffusion.processors.glid3xl", "maua.diffusion.processors.glide", "maua.diffusion.processors.latent",
              "maua.diffusion.processors.stable", "maua.super.image.single", "maua.flow.mm", "maua.flow.sniklaus", "maua.flow.utils"):
        sys.modules[m] = MagicMock(name=m)
    import maua.flow.consistency as RC
    import maua.flow.lib as RL
    import maua.diffusion.video as RV
    out, meta = {}, {}
    g = torch.Generator().manual_seed(3801)

    # ---- flow_warp_map (it divides its argument in place: clones go in)
    for name, (h, w) in {"wm57": (5, 7), "wm129": (12, 9)}.items():
        flow = (torch.rand(2 if name == "wm57" else 1, h, w, 2, generator=g) - 0.5) * 3 * w
        RL.NEUTRAL = None
        out[f"{name}_flow"], out[f"{name}_map"] = flow.clone(), RL.flow_warp_map(flow.clone())

    # ---- mflo
    for name, (h, w) in {"mf_a": (6, 8), "mf_b": (7, 5)}.items():
        flow = ((torch.rand(h, w, 2, generator=g) - 0.5) * 40).numpy()
        enc = RL.encode_mflo(flow)
        out[f"{name}_flow"], out[f"{name}_enc"], out[f"{name}_dec"] = flow, enc, RL.decode_mflo(enc)

    # ---- check_consistency
    RC.gaussian_blur = lambda img, k: FR.gaussian_blur3(img)
    populated = dict(boundary=0, missed=0, overshoot=0)
    for name, (fwd, bwd) in consistency_pairs().items():
        out[f"cc_{name}_fwd"], out[f"cc_{name}_bwd"] = fwd, bwd
        out[f"cc_{name}_map"] = RC.check_consistency(fwd.clone(), bwd.clone())
        _, masks = FR.consistency_classes(fwd, bwd)
        for k in populated:
            populated[k] += int(masks[k].sum())
        _, frac = FR.near_threshold(fwd, bwd)
        assert frac <= 0.005, (name, frac)
    assert all(v > 0 for v in populated.values()), populated
    meta["cc_populated"] = populated

    # ---- the whole VideoFlowDiffusionProcessor.forward around recording stubs
    frames_data, flows, cons, first = FR.pipe_inputs(N_FRAMES, SIZE)      # seeded draws, regenerated by the tests (not stored)

    class Frames:
        def __init__(self, filename, height, width, device):
            pass

        def __len__(self):
            return N_FRAMES

        def __getitem__(self, idx):
            return frames_data[idx].clone()

    class Store:
        def __init__(self, name, log, items=None):
            self.name, self.log, self.items, self.length = name, log, dict(items or {}), len(items or {})

        def __len__(self):
            return self.length

        def __getitem__(self, idx):
            return self.items[int(idx)].clone()

        def insert(self, item, idx=None):
            idx = idx if idx is not None else len(self)
            self.items[int(idx)] = item.clone()
            self.log.append(["insert", self.name, int(idx)])
            self.length += 1

        def finalize(self):
            return self

    class Stub(torch.nn.Module):
        def __init__(self, log):
            super().__init__()
            self.log = log

        def forward(self, img, prompts, t_start, verbose=True):
            self.log.append(["forward", float(t_start), [type(p).__name__ for p in prompts]])
            return img * 0.75 + 0.125

    class Prompt:
        def __init__(self, *a, path=None, size=None, **k):
            self.img = first.clone()

    RV.trange = lambda *a, **k: range(*a)
    RV.VideoFrames = Frames
    RV.initialize_optical_flow = lambda *a, **k: None
    for cls in ("ContentPrompt", "StylePrompt", "ImagePrompt"):
        setattr(RV, cls, type(cls, (Prompt,), {}))
    RV.TextPrompt = type("TextPrompt", (), {"__init__": lambda self, text: None})

    cases = {"t1": dict(turbo=1, wrap_around=0), "t3": dict(turbo=3, wrap_around=0), "t1w2": dict(turbo=1, wrap_around=2),
             "t3w2": dict(turbo=3, wrap_around=2), "t3w2_first": dict(turbo=3, wrap_around=2, first_frame_init="first.png"),
             "t1_hist": dict(turbo=1, wrap_around=0, hist_persist=True), "t3w2_notrust": dict(turbo=3, wrap_around=2, consistency_trust=0.0)}
    for name, c in cases.items():
        log = []
        RV.match_histogram = lambda a, b, log=log: (log.append(["match_histogram"]), a * 0.9 + 0.1 * b.mean())[1]
        holder = {}

        def make_cache(names, out_name, device, log=log, holder=holder):
            holder["cache"] = type("C", (), dict(frame=Store("frame", log), flow=Store("flow", [], {i: flows[i] for i in range(N_FRAMES)}),
                                                 consistency=Store("consistency", [], {i: cons[i] for i in range(N_FRAMES)})))()
            return holder["cache"]
        RV.initialize_cache_files = make_cache
        # The reference's last step (f_n >= N + wrap_around: the one that only flushes the turbo in-betweens) indexes loop_fade past its
        # end (:268-269) and raises IndexError after the in-betweens are inserted and before the sampler is called.  Everything up to
        # there is recorded; the frames are read from the cache it filled.
        raised = False
        try:
            RV.VideoFlowDiffusionProcessor()(diffusion=Stub(log), init="clip.mp4", text="a prompt", style="style.png", size=(SIZE, SIZE),
                                             noise_injection=0.0, constant_seed=7, device="cpu", flow_exaggeration=1.5, **c)
        except IndexError:
            raised = True
        res = holder["cache"].frame
        video = torch.cat([res.items[i] for i in sorted(res.items)])
        # the result is as large as the clip: every fourth sample of both axes and a sum are kept
        out[f"pipe_{name}"] = video[:, :, 1::4, ::4].contiguous()
        meta[f"pipe_{name}"] = dict(log=log, shape=list(video.shape), sum=float(video.double().sum()), kwargs=c, raised=raised)

    # ---- the drop-in surface as data: argument names and default expressions, the command line's flags and help strings
    tree = ast.parse(Path(RV.__file__).read_text())
    sigs, flags = {}, []
    for node in ast.walk(tree):
        if isinstance(node, ast.FunctionDef) and node.name in ("forward", "video_sample", "initialize_optical_flow", "initialize_cache_files", "warp"):
            cls_init = node.name == "forward" and len(node.args.args) < 10        # WriteThread / Dataset methods are not captured
            if cls_init:
                continue
            a = node.args
            d = [None] * (len(a.args) - len(a.defaults)) + [ast.unparse(x) for x in a.defaults]
            sigs[node.name] = [[x.arg, dv] for x, dv in zip(a.args, d)]
        if isinstance(node, ast.Call) and getattr(node.func, "attr", "") == "add_argument":
            kw = {k.arg: ast.unparse(k.value) for k in node.keywords if k.arg in ("default", "action", "nargs")}
            hlp = [k.value.value for k in node.keywords if k.arg == "help"]
            flags.append([node.args[0].value, kw, hlp[0] if hlp else None])
    meta["signatures"], meta["cli"] = sigs, flags

    out["meta_json"] = np.array(json.dumps(meta))
    MG.save("g38_video_pipeline", **{k: (v.float() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v) for k, v in out.items()})


if __name__ == "__main__":
    main()
