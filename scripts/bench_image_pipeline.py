"""Timing split of the multi-resolution image pipeline (maua_amd/image.py): 256² -> 512² with stitching at tile_size 256, a 50-step
plms sampler, random-init weights (there are no checkpoints).  The sampler calls and the operators between the scales (lanczos3
resize, destitch, restitch) are timed separately with HIP events; each operator's GB/s is its algorithmic bytes (image read once +
written once) over its time, against the 6.3 TB/s copy rate.  Prints one JSON line.

    python scripts/bench_image_pipeline.py [--repeats N] [--timesteps 50]
    python scripts/bench_image_pipeline.py --count-torch-kernels     # a rocprofv3 --kernel-trace --stats run of its own (child process)
                                                                     # of a tiled and an un-tiled two-scale run: the kernels between
                                                                     # consecutive sampler calls that are not the library's operators

No speed target is set; DESIGN §5d quotes the numbers this prints."""
import argparse
import csv
import json
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
LIB_KERNELS = ("image_resize_kernel", "destitch_kernel", "restitch_kernel", "sharpen_kernel", "moments_kernel", "match_apply_kernel",
               "perlin_octaves_kernel", "perlin_autocontrast_kernel")
COPY_RATE = 6.3e12
MARK_SEED = 77
MARKER = "philox_kernel"


class Timed:
    """a processor wrapper that brackets every sampler call with HIP events"""

    def __init__(self, gd, torch, mark=False):
        self.gd, self.torch, self.spans, self.mark = gd, torch, [], mark
        self.image_size, self.device, self.model = gd.image_size, gd.device, gd.model

    def __call__(self, img, prompts, t_start, verbose=True):
        a, b = self.torch.cuda.Event(enable_timing=True), self.torch.cuda.Event(enable_timing=True)
        a.record()
        if self.mark:      # a library kernel with a name of its own in the trace, before and after every sampler call
            from maua_amd.rng import philox_u32
            philox_u32(MARK_SEED, len(self.spans), 1)
        out = self.gd(img, prompts, t_start, verbose=False)
        if self.mark:
            philox_u32(MARK_SEED, len(self.spans), 1)
        b.record()
        self.spans.append((a, b, tuple(img.shape)))
        return out


def build(timesteps):
    import torch
    from maua_amd.diffusion import get_diffusion_model
    torch.manual_seed(0)
    return get_diffusion_model("guided", timesteps=timesteps, sampler="plms",
                               guided_kwargs=dict(allow_random_init=True, model_checkpoint="uncondImageNet256"))


def time_op(torch, fn, repeats=20):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(repeats):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / repeats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--timesteps", type=int, default=50)
    ap.add_argument("--count-torch-kernels", action="store_true")
    ap.add_argument("--traced-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.count_torch_kernels:
        return count_torch_kernels(args)
    import torch
    import maua_amd.image as I
    gd = build(args.timesteps)
    proc = I.MultiResolutionDiffusionProcessor()
    schedule = {(256, 256): 0.0, (512, 512): 0.6}
    if args.traced_child:      # under the tracer: the tiled run, then an un-tiled second scale with a sharpen hook
        from functools import partial
        t = Timed(gd, torch, mark=True)
        proc(t, "random", schedule=schedule, tile_size=256, stitch=True, max_batch=4, verbose=False)
        n1 = len(t.spans)
        proc(t, "random", schedule={(256, 256): 0.0, (256, 320): 0.6}, stitch=False, post_hook=partial(I.sharpen, strength=1.5), verbose=False)
        torch.cuda.synchronize()
        print("CALLS " + json.dumps([n1, len(t.spans) - n1]))
        return
    rows = []
    for r in range(args.repeats + 1):
        t = Timed(gd, torch)
        torch.manual_seed(1)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = proc(t, "random", schedule=schedule, tile_size=256, stitch=True, max_batch=4, verbose=False)
        b.record()
        torch.cuda.synchronize()
        total = a.elapsed_time(b)
        sampler = sum(x.elapsed_time(y) for x, y, _ in t.spans)
        # between the scales: from the end of scale 0's (single) sampler call to the start of scale 1's first one - resize + destitch;
        # the gaps between the tile batches of one scale are reported apart
        between = t.spans[0][1].elapsed_time(t.spans[1][0])
        gaps = sum(t.spans[i][1].elapsed_time(t.spans[i + 1][0]) for i in range(1, len(t.spans) - 1))
        if r:                   # the first pass warms up (graph capture, tables)
            rows.append((total, sampler, between, gaps, len(t.spans)))
    assert tuple(out.shape) == (1, 3, 512, 512) and bool(torch.isfinite(out).all())
    x256 = torch.randn(1, 3, 256, 256, device="cuda")
    x512 = I.resize(x256, (512, 512), interp_method="lanczos3")
    tiles = I.destitch(x512, 256)
    ops = {"resize_lanczos3_256_to_512": (lambda: I.resize(x256, (512, 512), interp_method="lanczos3"), x256.numel() * 4 + x512.numel() * 4),
           "destitch_512_t256": (lambda: I.destitch(x512, 256), 2 * tiles.numel() * 4),
           "restitch_512_t256": (lambda: I.restitch(tiles, 512, 512), tiles.numel() * 4 + x512.numel() * 4),
           "sharpen_512": (lambda: I.sharpen(x512, 1.5), 2 * x512.numel() * 4)}
    op_rows = {}
    for k, (fn, nbytes) in ops.items():
        ms = time_op(torch, fn)        # includes the host side of the call (allocation, ctypes): launch-latency sized operators
        op_rows[k] = dict(ms=round(ms, 4), gb_s=round(nbytes / (ms * 1e-3) / 1e9, 1), frac_of_copy_rate=round(nbytes / (ms * 1e-3) / COPY_RATE, 4))
    best = min(rows)
    print(json.dumps(dict(bench="image_pipeline", schedule="256x256 -> 512x512, tile 256, plms", timesteps=args.timesteps,
                          total_ms=round(best[0], 2), sampler_ms=round(best[1], 2), between_scales_ms=round(best[2], 3),
                          between_tile_batches_ms=round(best[3], 3), after_last_call_ms=round(best[0] - best[1] - best[2] - best[3], 3),
                          sampler_calls=best[4], sampler_share=round(best[1] / best[0], 4), operators=op_rows,
                          device=torch.cuda.get_device_name(0))))


def count_torch_kernels(args):
    """A traced run of the pipeline, tiled (256² -> 512², tile 256: one call, then 4 + 4 + 1 tiles) and un-tiled (256² -> 256 x 320 with
    a sharpen hook).  Every sampler call is bracketed by a marker kernel; the kernels between the closing marker of one call and the
    opening marker of the next one of the same run are listed: the library's operators are expected, nothing else."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, __file__, "--traced-child",
               "--timesteps", str(args.timesteps)]
        r = subprocess.run(cmd, cwd=str(ROOT), capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(r.stdout[-2000:], r.stderr[-2000:])
            raise SystemExit(r.returncode)
        calls = json.loads(next(l for l in r.stdout.splitlines() if l.startswith("CALLS "))[6:])
        rows = []
        for f in sorted(Path(d).rglob("*kernel_trace.csv")):
            with open(f) as fh:
                rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    names = [r["Kernel_Name"] for r in rows]
    marks = [i for i, n in enumerate(names) if MARKER in n]
    assert len(marks) == 2 * sum(calls), (len(marks), calls)
    run_of = [k for k, n in enumerate(calls) for _ in range(n)]          # which run a sampler call belongs to
    library, other = {}, {}
    for c in range(sum(calls) - 1):
        if run_of[c] != run_of[c + 1]:
            continue                                                      # (set-up of the second run: not between two scales)
        for n in names[marks[2 * c + 1] + 1:marks[2 * c + 2]]:
            hit = next((k for k in LIB_KERNELS if k in n), None)
            d = library if hit else other
            d[hit or n] = d.get(hit or n, 0) + 1
    print(json.dumps(dict(bench="image_pipeline_kernel_trace", kernels_total=len(names), sampler_calls=calls,
                          between_sampler_calls_library_kernels=library, between_sampler_calls_other_kernels=other)))


if __name__ == "__main__":
    main()
