"""Time the float64 Jacobi solver on one MI355X: ``cff`` on the stacked style-affine weight of the 1024^2 StyleGAN2 (its
shape computed from the network's channel table; Gaussian entries, as the random-init network has), and ``eigh`` at 512 and 2048.

Device events around each call, after a warm-up of the same call; ``--reps`` repeats, min and max quoted.  Beside each time: the sweeps
the call reported and, from the shapes alone, the launches and the bytes moved per sweep on the per-round path (every pair read and
written once per round: 2 columns of m + n doubles each way; a sweep that skips pairs moves less).  No target is set.  As a yardstick
only, ``torch.linalg.svd`` / ``eigh`` on the same device and matrix is timed beside it (``--no_yardstick`` leaves it out; where the
vendor solver is unavailable the field says so).  Prints one JSON line.

    python scripts/bench_decomposition.py [--reps 2] [--eigh 512 2048] [--no_yardstick]
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def device_ms(fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    out = fn()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop), out


def cff_shape(res=1024, w_dim=512):
    """rows of W: C_in of block 0's conv1, then of conv0 and conv1 of every later block"""
    from maua_amd.stylegan2 import block_resolutions, channels_dict
    ch = channels_dict(res)
    return sum(ch[r] if r == 4 else ch[r // 2] + ch[r] for r in block_resolutions(res)), w_dim


def traffic(m, n):
    """(launches, bytes) of one sweep of the per-round path"""
    N, mp, np_ = n + (n & 1), m + (m & 1), n + (n & 1)
    return N, (N - 1) * (n // 2) * 2 * (mp + np_) * 8 * 2


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--eigh", type=int, nargs="*", default=[512, 2048])
    ap.add_argument("--no_yardstick", action="store_true")
    args = ap.parse_args(argv)
    from maua_amd import decomposition as D
    g = torch.Generator(device="cuda").manual_seed(1)
    res = {"reps": args.reps}

    def run(name, ours, theirs, m, n):
        device_ms(ours)
        times, out = [], None
        for _ in range(args.reps):
            t, out = device_ms(ours)
            times.append(t)
        launches, nbytes = traffic(m, n)
        rec = {"shape": [m, n], "ms": {"min": round(min(times), 2), "max": round(max(times), 2)}, "sweeps": out["sweeps"],
               "launches_per_sweep": launches, "GB_per_sweep": round(nbytes / 1e9, 3),
               "GB_per_s": round(nbytes * out["sweeps"] / 1e9 / (min(times) / 1e3), 1)}
        if not args.no_yardstick:
            try:
                device_ms(theirs)
                rec["torch_linalg_ms"] = round(min(device_ms(theirs)[0] for _ in range(args.reps)), 2)
            except Exception as e:      # the yardstick is optional: the package never calls it
                rec["torch_linalg_ms"] = f"unavailable: {type(e).__name__}"
        res[name] = rec

    m, n = cff_shape()
    W = torch.randn(m, n, device="cuda", generator=g).double()
    run("cff_1024", lambda: D.svd_info(W, want_u=False), lambda: torch.linalg.svd(W, full_matrices=False), m, n)
    for d in args.eigh:
        x = torch.randn(2 * d, d, device="cuda", generator=g).double()
        S = x.T @ x / (2 * d)
        run(f"eigh_{d}", lambda: D.eigh_info(S), lambda: torch.linalg.eigh(S), d, d)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
