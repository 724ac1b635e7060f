"""Augmented cutouts (maua/ops/cutouts.py:53-206 with skip_augs=False; csrc/cutout_augs.hip) inside text-prompt guidance: the time of
one CLIPGrads.forward with skip_augs True vs False - random-init ViT-B/16, `batch` 256^2 estimates, 8 cutout batches; "normal" with
cutn = 32 and "dango" with its default schedule at t = 300 and 700 - and the bytes the four augmentation kernels move per call (each
buffer read and written once: the nominal traffic, for an achieved-bandwidth figure from a rocprofv3 --kernel-trace --stats run of
this script).  `python scripts/bench_cutout_augs.py [--batch 4] [--reps 3]`; one JSON line per configuration."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def aug_bytes(mode, rects, B, H, W, cs):
    """Nominal bytes of the augmentation kernels of one call (f32): forward (1) source -> A, (2) A -> out; adjoint (1) out -> dA,
    (2) dA -> source gradient.  "normal": per cutout the crop's s^2 pixels x 3 planes x B images through all four, plus the gradient
    image written once per cutout batch; "dango": the N B resized cutouts through all four."""
    px = 0
    for batch in rects:
        if mode == "normal":
            px += sum(int(r[0]) ** 2 for r in batch) * B * 3 * 8   # 4 passes x (read + write)
            px += B * 3 * H * W                                      # the gradient image
        else:
            px += len(batch) * B * 3 * cs * cs * 8
    return px * 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from maua_amd.clip import load
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    model, _ = load("ViT-B/16", allow_random_init=True, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(1)
    prompts = [EmbeddingPrompt(torch.randn(512, generator=g)), EmbeddingPrompt(torch.randn(512, generator=g), 0.5)]
    img = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    # (make_cutouts takes cutn for every kind; DangoCutouts ignores it: its schedule decides)
    for mode, kw, t in (("normal", dict(cutn=32), 500), ("dango", dict(cutn=32), 300), ("dango", dict(cutn=32), 700)):
        res = {}
        for skip in (True, False):
            gm = CLIPGrads(scale=1000.0, cutouts=mode, clip_models=[model], cutout_kwargs=dict(kw, skip_augs=skip), cutout_batches=a.batches)
            gm.set_targets(prompts)
            tt = torch.full((a.batch,), float(t))
            torch.manual_seed(2)
            gm(img, tt)
            torch.cuda.synchronize()
            best = None
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = gm(img, tt)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                best = dt if best is None else min(best, dt)
            assert bool(torch.isfinite(out).all())
            res[skip] = best
            if not skip:
                rects = gm.last_aug_plan[0][0]
        nb = aug_bytes(mode, rects, a.batch, a.size, a.size, 224)
        print(json.dumps(dict(bench="cutout_augs", mode=mode, t=t, batch=a.batch, size=a.size, cutout_batches=a.batches,
                              cutouts_per_batch=int(rects.shape[1]), ms_skip_augs=round(res[True] * 1e3, 2),
                              ms_augs=round(res[False] * 1e3, 2), delta_ms=round((res[False] - res[True]) * 1e3, 2),
                              aug_kernel_bytes=int(nb), aug_kernel_mb=round(nb / 1e6, 1))), flush=True)


if __name__ == "__main__":
    main()
