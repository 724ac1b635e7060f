"""Time the GAN evaluation metrics on one MI355X at the reference's defaults: N = 10 000 features of d = 2048 per set,
nearest_k = 5, 100 subsets of 1000 rows.

  * gemm: maua_gemm_f64 at 2048^3 (a Newton-Schulz product) and at 10 000 x 10 000 x 2048 (a distance matrix's product), TFLOP/s;
    also A^T B and A B^T at 2048^3, the two layouts the covariance and the distances use.
  * frechet: frechet_distance whole, and the Newton-Schulz square root alone with its iteration count.
  * kernel: kernel_distance whole.  prdc: prdc whole.
  * host: the numpy float64 restatement's sqrtm (tests/metrics_ref.py) at d = 2048 on this host's threads, with --host (minutes).

A host clock around work that ends in a device synchronise, after a warm-up of the same call; ``--reps`` repeats each, min and max
quoted (the discipline of every bench script here).  Prints one JSON line.

    python scripts/bench_metrics.py [--reps 3] [--n 10000] [--d 2048] [--host]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np
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
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--n", type=int, default=10_000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--skip", nargs="*", default=[], choices=["gemm", "frechet", "kernel", "prdc"])
    ap.add_argument("--host", action="store_true", help="also time the numpy float64 sqrtm at d on the host")
    args = ap.parse_args(argv)
    from maua_amd import metrics as M
    n, d = args.n, args.d
    g = torch.Generator(device="cuda").manual_seed(1)
    mix = torch.randn(d, d, device="cuda", generator=g) / d ** 0.5
    real = torch.randn(n, d, device="cuda", generator=g) @ (torch.eye(d, device="cuda") + 0.5 * mix)
    fake = torch.randn(n, d, device="cuda", generator=g) * 1.1 + 0.1
    res = {"n": n, "d": d, "reps": args.reps}

    def run(name, fn, flop=None, warm=1):
        for _ in range(warm):
            timed(fn)
        times, out = [], None
        for _ in range(args.reps):
            t, out = timed(fn)
            times.append(t)
        res[name + "_ms"] = spread([1e3 * t for t in times])
        if flop:
            res[name + "_tflops"] = spread([flop / t / 1e12 for t in times])
        return out

    if "gemm" not in args.skip:
        a = torch.randn(d, d, dtype=torch.float64, device="cuda", generator=g)
        b = torch.randn(d, d, dtype=torch.float64, device="cuda", generator=g)
        out = torch.empty(d, d, dtype=torch.float64, device="cuda")
        run("gemm_nn_d3", lambda: M.gemm_f64(a, b, out=out), 2.0 * d ** 3)
        run("gemm_tn_d3", lambda: M.gemm_f64(a, b, transa=True, out=out), 2.0 * d ** 3)
        run("gemm_nt_d3", lambda: M.gemm_f64(a, b, transb=True, out=out), 2.0 * d ** 3)
        x, y = real.double(), fake.double()
        big = torch.empty(n, n, dtype=torch.float64, device="cuda")
        run("gemm_nt_n2d", lambda: M.gemm_f64(x, y, transb=True, out=big), 2.0 * n * n * d)
        del x, y, big
    if "frechet" not in args.skip:
        info = run("frechet", lambda: M.frechet_info(real, fake))
        res["frechet_iterations"], res["frechet"] = info["iterations"], info["distance"]
        prod = M.gemm_f64(*(M.moments(f)[1] for f in (real, fake)))
        _, _, iters = run("sqrtm", lambda: M.sqrtm_info(prod))
        res["sqrtm_iterations"] = iters
        res["sqrtm_tflops_in_products"] = spread([(4 * iters) * 2.0 * d ** 3 / (ms / 1e3) / 1e12 for ms in res["sqrtm_ms"].values()])
        if args.host:
            sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "tests"))
            import metrics_ref as MR
            m = prod.cpu().numpy()
            t = time.perf_counter()
            _, _, host_iters = MR.sqrtm(m)
            res["host_sqrtm_s"], res["host_sqrtm_iterations"], res["host_threads"] = round(time.perf_counter() - t, 2), host_iters, torch.get_num_threads()
    if "kernel" not in args.skip:
        np.random.seed(0)
        res["kid"] = run("kernel", lambda: M.kernel_distance(real, fake))
    if "prdc" not in args.skip:
        res["prdc"] = run("prdc", lambda: M.prdc(real, fake))
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
