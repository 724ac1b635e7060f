"""Time the synthesis network's gradient to its latents on one MI355X: SynthesisNetwork.vjp against the forward it
differentiates (the one with keep_features on) and against the render forward, at 1024^2, bfloat16, B = 8 by default; and the bytes
the gradient keeps alive (every layer's output, the walk's own workspaces).

A host clock around work that ends in a device synchronise, after a warm-up of the same calls; ``--reps`` repeats each, min and max
quoted (the discipline of every bench script here).  Prints one JSON line.

    python scripts/bench_synth_vjp.py [--res 1024] [--batch 8] [--reps 5] [--dtype bf16]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t, out


def spread(values, digits=2):
    return {"min": round(min(values), digits), "max": round(max(values), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    args = ap.parse_args(argv)
    from maua_amd.stylegan2 import SynthesisNetwork
    dt = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    net = SynthesisNetwork(512, args.res, 3, dtype=dt, generator=torch.Generator().manual_seed(0))
    B = args.batch
    g = torch.Generator(device="cuda").manual_seed(1)
    ws = torch.randn(B, net.num_ws, 512, device="cuda", generator=g)
    g_img = torch.randn(B, 3, args.res, args.res, device="cuda", generator=g)
    res = {"res": args.res, "batch": B, "dtype": args.dtype, "reps": args.reps}

    def run(name, fn):
        timed(fn)
        res[name + "_ms"] = spread([1e3 * timed(fn)[0] for _ in range(args.reps)])

    run("render_forward", lambda: net(ws))
    free0 = torch.cuda.mem_get_info()[0]
    net.keep_features(True)
    run("kept_forward", lambda: net(ws))
    free1 = torch.cuda.mem_get_info()[0]
    run("vjp", lambda: net.vjp(g_img))
    free2 = torch.cuda.mem_get_info()[0]
    es = 2 if dt == torch.bfloat16 else 4
    res["kept_feature_bytes"] = sum(B * co * r * r * es for _, _, co, r, _ in net.layer_shapes())
    res["kept_forward_workspace_growth_bytes"] = free0 - free1      # the features' own buffers, less what the render plan's scratch held
    res["vjp_workspace_bytes"] = free1 - free2                      # transposed weights, g_u / g_t / g_xm, gradients of two features
    res["backward_over_kept_forward"] = spread([res["vjp_ms"][k] / res["kept_forward_ms"][k] for k in ("min", "max")])
    res["backward_over_render_forward"] = spread([res["vjp_ms"][k] / res["render_forward_ms"][k] for k in ("min", "max")])
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
