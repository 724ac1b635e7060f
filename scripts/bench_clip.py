"""Text-prompt guidance (CLIPGrads, maua/grad.py:96-165) on one GPU: time of one grad-module call at configs[3]'s shape - `batch`
256^2 image estimates, `cutn` cutouts x `batches` cutout batches through a random-init image tower (`--model`: ViT-B/16 by default,
ViT-B/32, ViT-L/14, ViT-L/14@336px) forward AND backward - and the algorithmic FLOP rate, the images of the last pass through the
tower (the group the workspace budget led to, or its remainder) and the device memory in use.
`python scripts/bench_clip.py [--model ViT-L/14] [--batch 32] [--batches 8] [--reps 3]`; under rocprofv3 for the per-kernel split
(scripts/prof_clip.sh)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def vit_gflop(res=224, patch=16, width=768, layers=12, heads=12, out=512, backward=True):
    """Algorithmic GFLOP per image: patch embedding + per layer the four Linear layers and the two attention products (+ the head);
    the input gradient repeats every Linear against the transposed weight and costs four attention products (dV, dP, dQ, dK)."""
    G = res // patch
    T, kp = G * G + 1, 3 * patch * patch
    lin = T * (width * 3 * width + width * width + 2 * width * 4 * width)
    att = 2 * T * T * width
    fwd = G * G * kp * width + layers * (lin + att) + width * out
    bwd = G * G * kp * width + layers * (lin + 2 * att) + width * out if backward else 0
    return 2 * (fwd + bwd) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--cutn", type=int, default=32)
    ap.add_argument("--batches", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--dma", type=int, default=1)
    ap.add_argument("--model", default="ViT-B/16", choices=["ViT-B/32", "ViT-B/16", "ViT-L/14", "ViT-L/14@336px"])
    ap.add_argument("--workspace-limit", type=int, default=0, help="bytes one pass through the tower may take (0: from free memory)")
    a = ap.parse_args()
    import ctypes as C
    from maua_amd import _lib as L
    from maua_amd.clip import VISION_CONFIGS, load
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt
    cfg = VISION_CONFIGS[a.model]
    model, _ = load(a.model, allow_random_init=True, generator=torch.Generator().manual_seed(0), text_tower=False)
    if a.workspace_limit:
        model.visual.set_workspace_limit(a.workspace_limit)
    L.check(L.lib().maua_ctx_set_option(L.ctx(), b"gemm_dma", a.dma))
    gm = CLIPGrads(scale=1000.0, clip_models=[model], cutout_kwargs=dict(cutn=a.cutn), cutout_batches=a.batches)
    g = torch.Generator().manual_seed(1)
    gm.set_targets([EmbeddingPrompt(torch.randn(cfg[5], generator=g)), EmbeddingPrompt(torch.randn(cfg[5], generator=g), 0.5)])
    img = (torch.rand(a.batch, 3, a.size, a.size, generator=g) * 2 - 1).cuda()
    t = torch.full((a.batch,), 500.0)
    torch.manual_seed(2)
    out = gm(img, t)
    torch.cuda.synchronize()
    best = None
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = gm(img, t)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    n_img = a.batch * a.cutn * a.batches
    per_image = vit_gflop(*cfg)
    gf = per_image * n_img
    # images that actually went through the tower: a square image's identical whole-image cutouts go through once (merge_identical)
    torch.manual_seed(2)
    r, m = gm.merge_identical(gm.draw_rects(0, a.size, a.size, t)) if gm.merge_cutouts else (gm.draw_rects(0, a.size, a.size, t), None)
    n_exec = a.batch * r.shape[1] * a.batches
    lo, hi, probe = 0, a.batch * a.cutn, torch.empty(a.batch * a.cutn, device="cuda")   # images of the last pass (its kept forward)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if L.lib().maua_clip_last_image_losses(model.visual._handle(), mid, L.ptr(probe)) == 0 else (lo, mid - 1)
    print({"model": a.model, "images_executed_per_call": n_exec, "executed_tflops": per_image * n_exec / best / 1e3,
           "images_last_pass": lo, "cutouts_per_batch_executed": int(r.shape[1]), "batch": a.batch, "cutn": a.cutn, "cutout_batches": a.batches, "images_per_call": n_img, "seconds_per_call": best,
           "ms_per_cutout_batch": best / a.batches * 1e3, "gflop_per_image_fwd_bwd": per_image, "tflops": gf / best / 1e3,
           "frac_of_bf16_peak": gf / best / 1e3 / 2500.0, "finite": bool(torch.isfinite(out).all()), "gemm_dma": a.dma,
           "hbm_gb_allocated": torch.cuda.mem_get_info()[1] / 1e9 - torch.cuda.mem_get_info()[0] / 1e9})


if __name__ == "__main__":
    main()
