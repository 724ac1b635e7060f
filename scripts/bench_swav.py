"""Time the SwAV ResNet-50 feature extractor on one MI355X: batch 64 at 224 x 224, float32 (exact products) and bfloat16,
the reference's initialisation as weights.

  * images/s and TFLOP/s of the whole forward (2 x MACs of the convolutions, counted from the network's own shapes: about 8.2 GFLOP
    per image), ``--reps`` windows of ``--iters`` forwards between two HIP events after a warm-up, min and max per forward quoted;
  * the per-stage split (stem, max-pool, layer1 .. layer4, average pool) from HIP events between the stages of one forward
    (maua_resnet_forward_timed), the median over the repetitions;
  * for scale only, on the same device: torch.nn.functional.conv2d on the layer-4 3x3 (512 -> 512 at 7 x 7) and the layer-1 1x1
    (64 -> 256 at 56 x 56) next to the library's kernel on the same shape (maua_conv_strided_ex, which also prepares the weights
    on every call: its time includes that pass).

Prints one JSON line.

    python scripts/bench_swav.py [--reps 5] [--iters 40] [--batch 64] [--size 224]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
STAGES = ("stem", "maxpool", "layer1", "layer2", "layer3", "layer4", "avgpool")


def out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def forward_flops(shapes, layers, size):
    """2 x MACs per image of every convolution ([(Ci, Co, k, stride)] in the state dict's order), walking the network as the library does"""
    h = out_size(size, 7, 2, 3)
    total, i = 2 * h * h * 3 * shapes[0][1] * 49, 1
    h = out_size(h, 3, 2, 1)
    for blocks in layers:
        for b in range(blocks):
            c1, c2, c3 = shapes[i:i + 3]
            ho = out_size(h, 3, c2[3], 1)
            total += 2 * h * h * c1[0] * c1[1] + 2 * ho * ho * c2[0] * c2[1] * 9 + 2 * ho * ho * c3[0] * c3[1]
            i += 3
            if b == 0:
                total += 2 * ho * ho * shapes[i][0] * shapes[i][1]
                i += 1
            h = ho
    assert i == len(shapes)
    return total


def events_ms(fn, reps, iters):
    """milliseconds per call: ``reps`` windows of ``iters`` back-to-back calls between two HIP events, after a warm-up call"""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) / iters)
    return times


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=40, help="forwards per timed window")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=224)
    args = ap.parse_args(argv)
    from maua_amd import _lib as L
    from maua_amd import resnet as R
    layers = (3, 4, 6, 3)
    shapes = R.conv_shapes(layers)
    flops = forward_flops(shapes, layers, args.size)
    res = {"batch": args.batch, "size": args.size, "reps": args.reps, "iters": args.iters, "gflop_per_image": round(flops / 1e9, 3)}
    x = torch.rand((args.batch, 3, args.size, args.size), device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    sd = R.random_state_dict(layers, 64, torch.Generator().manual_seed(2))
    for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
        net = R.ResNetFeatures(layers, 64, dtype, sd)
        ms = events_ms(lambda: net(x), args.reps, args.iters)
        feats = torch.empty((args.batch, 2048), device="cuda")
        stage = (C.c_float * 7)()
        rows = []
        for _ in range(args.reps):
            L.check(L.lib().maua_resnet_forward_timed(net._net, L.ptr(x), args.batch, args.size, args.size, L.ptr(feats), stage))
            rows.append(list(stage))
        res[name] = {"ms": {"min": round(min(ms), 3), "max": round(max(ms), 3)},
                     "images_per_s": round(args.batch / (min(ms) / 1e3), 1),
                     "tflops": round(flops * args.batch / (min(ms) / 1e3) / 1e12, 2),
                     "stage_ms": {s: round(statistics.median(r[i] for r in rows), 3) for i, s in enumerate(STAGES)}}
        del net
    print(json.dumps(res), file=sys.stderr, flush=True)      # (the extractor's own numbers, should the comparison below not finish)
    # for scale: single layers, torch's convolution next to the library's kernel
    B = args.batch
    for tag, (ci, co, k, hw) in (("layer4_3x3", (512, 512, 3, 7)), ("layer1_1x1", (64, 256, 1, 56))):
        layer_flops = 2 * B * hw * hw * ci * co * k * k
        entry = {}
        for name, dtype in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            xt = torch.randn((B, ci, hw, hw), device="cuda").to(dtype)
            wt = torch.randn((co, ci, k, k), device="cuda").to(dtype)
            t = events_ms(lambda: torch.nn.functional.conv2d(xt, wt, None, 1, k // 2), args.reps, args.iters)
            xl = xt.permute(0, 2, 3, 1).contiguous()
            wl, yl = wt.float().contiguous(), torch.empty((B, hw, hw, co), dtype=dtype, device="cuda")
            d = L.SConvDesc(x=xl.data_ptr(), w=wl.data_ptr(), bias=0, res=0, y=yl.data_ptr(), B=B, H=hw, W=hw, Ci=ci, Co=co, k=k, stride=1,
                            pad=k // 2, relu=1)
            m = events_ms(lambda: L.check(L.lib().maua_conv_strided_ex(L.ctx(), C.byref(d), L.dtype_id(dtype))), args.reps, args.iters)
            entry[name] = {"torch_conv2d_ms": round(min(t), 4), "torch_tflops": round(layer_flops / (min(t) / 1e3) / 1e12, 2),
                           "maua_ms_with_weight_prep": round(min(m), 4), "maua_tflops": round(layer_flops / (min(m) / 1e3) / 1e12, 2)}
        res[tag] = entry
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
