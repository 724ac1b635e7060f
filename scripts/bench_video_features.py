"""Time the audio-reactivity instruments on one MI355X.

  * one VideoAnalyzer push of 128 uint8 HWC frames at 1024 x 1024 (what one bench.py step renders), on random frames and on frames of one
    constant colour (the worst case for the LDS bin counters: every pixel of a wave hits the same six counters);
  * one correlation call at T = 3600, Fx = Fy = 194, per metric.

HIP events around each call; warm-up first; every repetition reads another input buffer, and the buffers (402 MB each, more than the
256 MB Infinity Cache) rotate so that no repetition finds its frames cached by the one before; the median and the spread
(min .. max) over the repetitions.  Prints one JSON line.

The bar for the push is 2 % of bench.py's step at the same batch; measured 1.30 ms (random) / 1.20 ms (constant) beside a 27.76 ms step,
4.7 % / 4.3 %: missed, see DESIGN 5f for what binds it.

    python scripts/bench_video_features.py [--frames 128] [--size 1024] [--reps 9] [--step-ms <bench.py's ms per step>]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def time_calls(fn, inputs, warmup, reps):
    """fn(x) over rotating inputs -> sorted list of milliseconds, one per repetition."""
    for i in range(warmup):
        fn(inputs[i % len(inputs)])
    torch.cuda.synchronize()
    times = []
    for i in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x = inputs[(warmup + i) % len(inputs)]
        a.record()
        fn(x)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)


def summary(times, nbytes=None):
    med = statistics.median(times)
    out = {"ms_median": round(med, 4), "ms_min": round(times[0], 4), "ms_max": round(times[-1], 4), "reps": len(times)}
    if nbytes is not None:
        out["GB_per_s"] = round(nbytes / med / 1e6, 1)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--T", type=int, default=3600)
    ap.add_argument("--F", type=int, default=194)
    ap.add_argument("--step-ms", type=float, default=None, help="bench.py's ms per step in the same session: the push is quoted as a share of it")
    a = ap.parse_args(argv)
    from maua_amd import correlation as CR
    from maua_amd.video_features import VideoAnalyzer
    torch.cuda.set_device(0)
    B, S = a.frames, a.size
    nbytes = B * S * S * 3
    result = {"frames": B, "size": S, "bins": a.bins, "frame_bytes": nbytes}
    an = VideoAnalyzer(S, S, bins=a.bins, max_batch=B)
    hist = torch.empty((B, 6, a.bins), device="cuda")
    vd = torch.empty((2, B), device="cuda")

    def push(x):
        an.push_raw(x, hist, None, vd[0], vd[1], 0)

    g = torch.Generator(device="cuda").manual_seed(0)
    random_frames = [torch.randint(0, 256, (B, S, S, 3), dtype=torch.uint8, device="cuda", generator=g) for _ in range(3)]
    result["push_random"] = summary(time_calls(push, random_frames, a.warmup, a.reps), nbytes)
    del random_frames
    constant_frames = [torch.full((B, S, S, 3), 40 + 70 * i, dtype=torch.uint8, device="cuda") for i in range(3)]
    an.reset()
    result["push_constant"] = summary(time_calls(push, constant_frames, a.warmup, a.reps), nbytes)
    del constant_frames
    an.close()
    if a.step_ms:
        result["step_ms"] = a.step_ms
        result["push_random_share_of_step"] = round(result["push_random"]["ms_median"] / a.step_ms, 4)
        result["push_constant_share_of_step"] = round(result["push_constant"]["ms_median"] / a.step_ms, 4)
    T, F = a.T, a.F
    pairs = []
    for i in range(3):
        base = torch.randn(T, F, device="cuda", generator=g)
        pairs.append((base + 0.5 * torch.randn(T, F, device="cuda", generator=g), 0.5 * base + torch.randn(T, F, device="cuda", generator=g)))
    result["correlation"] = {"T": T, "Fx": F, "Fy": F}
    for m in CR.METRICS:
        result["correlation"][m] = summary(time_calls(lambda xy: CR.correlation(m, *xy), pairs, a.warmup, a.reps), 2 * T * F * 4)
    print(json.dumps(result))
    return result


if __name__ == "__main__":
    main()
