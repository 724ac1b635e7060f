"""Time one projection step (maua_amd/projection.py) stage by stage on one MI355X: the BASELINE 1024^2 random-init bfloat16
network at B = 1 and 8.  HIP events on the stream around each stage, a warm-up of the same calls, ``--reps`` repetitions, median and
min - max quoted.  The two arms of the noise-gradient extra - maua_synth_vjp_ex with and without g_noise, on the same build - alternate
inside one loop and must give the same g_ws bits.  Prints one JSON line.

    python scripts/bench_projection.py [--res 1024] [--batches 1 8] [--reps 5] [--warmup 2] [--no_lpips]
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def stats(ms):
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


class Stages:
    """stage name -> milliseconds per call, from a pair of events recorded on the current stream around it"""

    def __init__(self):
        self.pending, self.ms = [], {}

    def run(self, name, fn, record=True):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        if record:
            self.pending.append((name, a, b))
        return out

    def collect(self):
        torch.cuda.synchronize()
        for name, a, b in self.pending:
            self.ms.setdefault(name, []).append(a.elapsed_time(b))
        self.pending = []


def bench(res, B, reps, warmup, lpips):
    from maua_amd import _lib as L
    from maua_amd import projection as P
    from maua_amd.stylegan2 import SynthesisNetwork
    lib = L.lib()
    net = SynthesisNetwork(512, res, 3, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(0))
    net.keep_features(True)
    num_ws, w_dim = net.num_ws, net.w_dim
    sizes = [net.layer_size(l) for l in range(net.num_layers)]
    dev = "cuda"
    w = torch.randn(B, 1, w_dim, device=dev)
    eps, g_w, m_w, v_w = torch.empty_like(w), torch.empty_like(w), torch.zeros_like(w), torch.zeros_like(w)
    ws = torch.empty(B, num_ws, w_dim, device=dev)
    img = torch.empty(B, 3, res, res, device=dev)
    noise = [torch.randn(B, 1, h, wd, device=dev) for h, wd in sizes]
    g_noise = [torch.empty_like(n) for n in noise]
    m_n, v_n = [torch.zeros_like(n) for n in noise], [torch.zeros_like(n) for n in noise]
    reg_loss = torch.empty(len(noise), B, device=dev)
    nbytes = max([lib.maua_noise_reg_workspace_bytes(B, h) for h, _ in sizes] + [lib.maua_noise_renorm_workspace_bytes(B, h * wd) for h, wd in sizes])
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    module, module_error = None, None
    if lpips:
        try:
            from maua_amd.grad import ContentPrompt, LPIPSGrads
            module = LPIPSGrads(scale=1, allow_random_init=True)     # (no perceptor weights ship with the library: timing only)
            module.set_targets([ContentPrompt(img=torch.rand(B, 3, res, res))])
        except Exception as e:      # (no perceptor weights, ...): said in the result, the other stages are still timed
            module, module_error = None, f"{type(e).__name__}: {e}"
    g_fixed = torch.randn(B, 3, res, res, device=dev)
    t_mid = torch.tensor(500.0)
    st = Stages()
    step_size, inv = P.adam_scalars(0.1, 10)
    same_bits = True

    def adam_renorm():
        ctx = L.ctx()
        L.check(lib.maua_adam_step(ctx, L.ptr(w), L.ptr(g_w), L.ptr(m_w), L.ptr(v_w), w.numel(), 0.9, 0.999, 1e-8, step_size, inv))
        for l, (h, wd) in enumerate(sizes):
            L.check(lib.maua_adam_step(ctx, L.ptr(noise[l]), L.ptr(g_noise[l]), L.ptr(m_n[l]), L.ptr(v_n[l]), noise[l].numel(), 0.9, 0.999,
                                       1e-8, step_size, inv))
            L.check(lib.maua_noise_renorm(ctx, L.ptr(noise[l]), B, h * wd, L.ptr(scratch), scratch.numel()))

    def regulariser():
        ctx = L.ctx()
        for l, (h, _) in enumerate(sizes):
            L.check(lib.maua_noise_reg(ctx, L.ptr(noise[l]), B, h, 1e5, L.ptr(reg_loss[l]), L.ptr(g_noise[l]), 1, L.ptr(scratch), scratch.numel()))

    for it in range(warmup + reps):
        rec = it >= warmup
        ctx = L.ctx()
        st.run("expand", lambda: (L.check(lib.maua_philox_normal(ctx, 0, it, 0, L.ptr(eps), eps.numel(), 0.0, 1.0)),
                                  L.check(lib.maua_latent_expand(ctx, L.ptr(w), 1, L.ptr(eps), 0.01, L.ptr(ws), B, num_ws, w_dim))), rec)
        st.run("forward_kept", lambda: net(ws, noise=noise, out=img), rec)
        g_img = st.run("loss_module", lambda: module(img, t_mid), rec) if module is not None else g_fixed
        # the two arms, alternating order from repetition to repetition
        arms = [("vjp", lambda: net.vjp(g_img, noise=noise)), ("vjp_with_noise_grad", lambda: net.vjp(g_img, noise=noise, noise_grad=g_noise)[0])]
        got = {}
        for name, fn in (arms if it % 2 == 0 else arms[::-1]):
            got[name] = st.run(name, fn, rec)
        same_bits = same_bits and bool(torch.equal(got["vjp"], got["vjp_with_noise_grad"]))
        st.run("reduce", lambda: L.check(lib.maua_latent_reduce(ctx, L.ptr(got["vjp"]), L.ptr(g_w), B, num_ws, w_dim)), rec)
        st.run("regulariser", regulariser, rec)
        st.run("adam_renorm", adam_renorm, rec)
        st.collect()
    out = {k: stats(v) for k, v in st.ms.items()}
    out["noise_grad_extra_ms"] = round(out["vjp_with_noise_grad"]["median"] - out["vjp"]["median"], 3)
    out["g_ws_same_bits"] = same_bits
    out["noise_map_bytes"] = sum(B * h * wd * 4 for h, wd in sizes)
    out["step_ms_median"] = round(sum(out[k]["median"] for k in ("expand", "forward_kept", "vjp_with_noise_grad", "reduce", "regulariser",
                                                                  "adam_renorm")) + (out["loss_module"]["median"] if module is not None else 0), 3)
    if module_error:
        out["loss_module_error"] = module_error
    assert all(bool(torch.isfinite(n).all()) for n in noise)
    del net
    torch.cuda.empty_cache()
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no_lpips", action="store_true", help="time the other stages with a fixed image gradient")
    args = ap.parse_args(argv)
    res = {"res": args.res, "dtype": "bf16", "reps": args.reps, "warmup": args.warmup}
    for B in args.batches:
        res[f"B{B}"] = bench(args.res, B, args.reps, args.warmup, not args.no_lpips)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
