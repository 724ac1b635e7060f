"""Timing split of the optical-flow video pipeline on one device, with HIP events: one Farneback pair at 512 x 512 (both
directions), the consistency map, the composition launch, and a sampler call (random-init guided network) beside them.  Prints one
JSON line.  There is no parent to compare with: the numbers describe, they promise nothing.

    python scripts/bench_video_pipeline.py [--size 512] [--reps 10] [--timesteps 20] [--count-torch-kernels]

``--count-torch-kernels`` starts a ``rocprofv3 --kernel-trace --stats`` run of its own (a fresh child process, no counters in the same
run) over a short clip with turbo=1 and no hooks, and lists the kernels that are neither the library's nor the sampler's."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import torch  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def small_guided(timesteps):
    from maua_amd.diffusion import GuidedDiffusion, SpacedDiffusion, UNetModel, space_timesteps
    from oracle import diffusion as OD
    cfg = OD.unet_config(image_size=64, model_channels=32, num_res_blocks=1, attention_resolutions=(16, 8), channel_mult=(1, 2, 2), num_head_channels=32)
    net = UNetModel(image_size=cfg["image_size"], in_channels=3, model_channels=cfg["model_channels"], out_channels=cfg["out_channels"],
                    num_res_blocks=cfg["num_res_blocks"], attention_resolutions=cfg["attention_ds"], channel_mult=cfg["channel_mult"],
                    num_head_channels=cfg["num_head_channels"], use_scale_shift_norm=True, resblock_updown=True, dtype=torch.float32)
    net.load_state_dict(OD.init_unet_params(cfg, torch.Generator().manual_seed(0)))
    sd = SpacedDiffusion(space_timesteps(1000, str(timesteps)), OD.linear_betas(1000), rescale_timesteps=True)
    return GuidedDiffusion([], sampler="plms", timesteps=timesteps, model=net, diffusion=sd)


def clip(n, size):
    import flow_ref as FR
    return (torch.stack([FR.sinusoid_pair(size, size, shift=(1.5 * i, -0.75 * i), seed=40)[1] for i in range(n)]) * 255).round().byte()


def traced_child(size):
    import maua_amd.video_diffusion as VD
    VD.video_sample(small_guided(3), clip(4, size), size=(size, size), turbo=1, constant_seed=1)
    torch.cuda.synchronize()


def count_torch_kernels(size):
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "video", "--output-format", "csv", "--", sys.executable, __file__,
               "--traced-child", "--size", str(size)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
        if r.returncode != 0:
            return dict(error=r.stderr[-500:])
        names = {}
        for f in Path(d).rglob("*kernel_stats.csv"):
            for line in f.read_text().splitlines()[1:]:
                parts = line.split('","')
                if len(parts) > 1:
                    names[parts[0].strip('"')] = int(parts[1].strip('"'))
        foreign = {k: v for k, v in names.items() if "maua" not in k}
        return dict(kernels=len(names), not_the_librarys=foreign)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--timesteps", type=int, default=20)
    ap.add_argument("--count-torch-kernels", action="store_true")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.traced_child:
        return traced_child(min(args.size, 128))
    import flow_ref as FR
    import maua_amd.flow as F
    S = args.size
    a, b = (t.cuda() for t in FR.sinusoid_pair(S, S))
    model = F.get_flow_model()
    out = dict(size=S, levels=F.farneback_levels(S, S))
    out["farneback_pair_ms"] = timed(lambda: model.pair(a, b), args.reps)
    fwd, bwd = model.pair(a, b)
    buf = torch.empty((2, 1, S, S), device="cuda")
    out["consistency_ms"] = timed(lambda: F.check_consistency(fwd, bwd, out=(buf[0], buf[1])), args.reps)
    frame, prev = torch.rand(2, 1, 3, S, S, device="cuda") * 2 - 1
    res = torch.empty_like(frame)
    out["compose_ms"] = timed(lambda: F.compose(frame, prev, fwd, buf[1], None, noise_injection=0.02, seed=1, out=res), args.reps)
    gd = small_guided(args.timesteps)
    out["sampler_call_ms"] = timed(lambda: gd(frame, [], 0.7, verbose=False), max(1, args.reps // 5))
    out["sampler"] = f"random-init 3-level UNet, plms, {args.timesteps} timesteps, skip 0.7"
    if args.count_torch_kernels:
        out["trace"] = count_torch_kernels(S)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
