"""Time the cellular automaton's step on one MI355X against the reference's own formulation as torch ops on the same device.

  * render: the evolution video's steady state (generate.py:14-21 from frame 150 on): a 256 x 256 state, B = 1, 32 steps per frame, the frame
    packed to u8 on the device.  steps/s from calls of 32 steps; frames/s with the packing.  Both product modes ("f32": exact
    v_mfma_f32_32x32x2_f32, "split": hi / lo bf16).
  * training shape: 4 x 12 x 128 x 128, 64 steps (the mean of train.py:220's draw): steps/s, forward_keep steps/s, the automaton's half
    of a training iteration - forward_keep + the gradient back to the parameters (CA.backward) from a given dL/dx_64 - and the whole
    iteration (nca.train_step: the steps, the VGG-16 batch-mean Gram loss on five taps, the walk back, gradient normalisation, Adam)
    with the perceptor in bf16 and in f32, as iterations/s.  VGG-16 is randomly initialised: the time does not depend on the weights.
  * torch: F.pad(circular) + conv2d + two 1 x 1 convolutions + torch.rand mask (train.py:158-185) on the same shapes, without autograd
    for the steps; with autograd (64 steps, backward from the same dL/dx_64) for the automaton's half; and train.py:221-236 whole -
    the steps, calc_styles on a float32 vgg16.features[:26] of the same weights, style_loss, backward, normalisation, Adam.

A host clock around work that ends in a device synchronise, after a warm-up of the same calls; five repeats each, min and max quoted, the
library and torch alternating inside a repeat.  The render's steps/s are taken at 1, 2 and 4 steps per launch (temporal blocking,
CA(steps_per_launch=k): same bits) in both product modes; everything else runs one step per launch.
Prints one JSON line.

    python scripts/bench_nca.py [--reps 5] [--frames 200]
"""
import argparse
import json
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def torch_filters(dev):
    ident = torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 0.0]], device=dev)
    sobel = torch.tensor([[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]], device=dev)
    lap = torch.tensor([[1.0, 2.0, 1.0], [2.0, -12.0, 2.0], [1.0, 2.0, 1.0]], device=dev)
    return torch.stack([ident, sobel, sobel.T, lap])[:, None]


def torch_step(x, filters, w1, b1, w2, rate=0.5):
    b, c, h, w = x.shape
    y = F.pad(x.reshape(b * c, 1, h, w), [1, 1, 1, 1], "circular")
    y = F.conv2d(y, filters).reshape(b, -1, h, w)
    y = F.conv2d(torch.relu(F.conv2d(y, w1, b1)), w2)
    return x + y * (torch.rand(b, 1, h, w, device=x.device) + rate).floor()


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t


def spread(values, digits=1):
    return {"min": round(min(values), digits), "max": round(max(values), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=200, help="frames (of 32 steps) per timed window")
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), "bench_nca.py needs a HIP device"
    from maua_amd import nca
    dev = torch.device("cuda")
    torch.manual_seed(0)
    cas = {}
    for mode in ("f32", "split"):
        ca = nca.CA(products=mode).to(dev)
        with torch.no_grad():
            ca.w2.weight.normal_(0.0, 0.02)
        cas[mode] = ca
    cas["split"].load_state_dict(cas["f32"].state_dict())
    cas_k = {}
    for mode in cas:
        for k in (2, 4):
            cas_k[mode, k] = nca.CA(products=mode, steps_per_launch=k).to(dev)
            cas_k[mode, k].load_state_dict(cas["f32"].state_dict())
    w1, b1, w2 = (p.detach() for p in (cas["f32"].w1.weight, cas["f32"].w1.bias, cas["f32"].w2.weight))
    filters = torch_filters(dev)
    n = a.frames

    def lib_steps(ca, x):
        for _ in range(n):
            ca.step(x, 32)

    def lib_frames(ca, x):
        for _ in range(n):
            ca.step(x, 32)
            nca.frame_bytes(x)

    def lib_keep(ca, x):
        for _ in range(n // 2):
            ca.forward_keep(x, 64)

    def torch_steps(x):
        with torch.no_grad():
            for _ in range(n * 32):
                x = torch_step(x, filters, w1, b1, w2)

    g_last = torch.randn(4, 12, 128, 128, device=dev)
    tw = [p.detach().clone().requires_grad_(True) for p in (w1, b1, w2)]

    def lib_iter(ca, x):
        for _ in range(n // 10):
            ca.backward(ca.forward_keep(x, 64), g_last, step0=ca.steps_done - 64)

    def torch_iter(x):
        for _ in range(n // 10):
            y = x
            for _ in range(64):
                y = torch_step(y, filters, *tw)
            (y * g_last).sum().backward()
            for p in tw:
                p.grad = None

    # the whole iteration: the library's train_step and train.py:221-236 as torch ops, the same VGG-16 weights and style targets
    from maua_amd.perceptors import IMAGENET_MEAN, IMAGENET_STD, VGG16_CFG
    styles = {dt: nca.StyleLoss.vgg16(allow_random_init=True, dtype=t) for dt, t in (("bf16", torch.bfloat16), ("f32", torch.float32))}
    layers, cin, sd = [], 3, styles["f32"].net.state_dict()
    for v in VGG16_CFG:
        if len(layers) > 25:
            break
        if v == "M":
            layers.append(torch.nn.MaxPool2d(2))
        else:
            conv = torch.nn.Conv2d(cin, v, 3, padding=1)
            conv.load_state_dict({"weight": sd[f"{len(layers)}.weight"], "bias": sd[f"{len(layers)}.bias"]})
            layers += [conv, torch.nn.ReLU()]
            cin = v
    vgg = torch.nn.Sequential(*layers[:26]).to(dev).requires_grad_(False)
    mean, std = (torch.tensor(v, device=dev)[:, None, None] for v in (IMAGENET_MEAN, IMAGENET_STD))
    style_img = torch.rand(1, 3, 128, 128, device=dev)
    for st in styles.values():
        st.set_target(style_img)
    targets = styles["f32"].targets
    train_cas = {dt: nca.CA(products="f32").to(dev) for dt in styles}
    for c in train_cas.values():
        c.load_state_dict(cas["f32"].state_dict())
    opts = {dt: torch.optim.Adam(c.parameters(), 1e-3) for dt, c in train_cas.items()}
    tp = [p.detach().clone().requires_grad_(True) for p in (w1, b1, w2)]
    topt = torch.optim.Adam(tp, 1e-3)

    def lib_train(dt, x):
        for _ in range(n // 10):
            nca.train_step(train_cas[dt], x, 64, styles[dt], opts[dt])

    def torch_train(x):
        for _ in range(n // 10):
            y = x
            for _ in range(64):
                y = torch_step(y, filters, *tp)
            f, loss = (y[:, :3] - mean) / std, 0.0
            for i, layer in enumerate(vgg):
                f = layer(f)
                if i in nca.STYLE_LAYERS:
                    g = torch.einsum("bchw,bdhw->bcd", f, f) / (f.shape[-2] * f.shape[-1])
                    loss = loss + (g.mean(0) - targets[nca.STYLE_LAYERS.index(i)]).square().mean()
            loss.backward()
            with torch.no_grad():
                for p in tp:
                    p.grad /= p.grad.norm() + 1e-8
            topt.step()
            topt.zero_grad()

    out = {"reps": a.reps, "steps_per_window": n * 32, "steps_per_launch": "1 unless a key says k2 / k4"}
    for name, shape in (("render_256", (1, 12, 256, 256)), ("train_shape_4x128", (4, 12, 128, 128))):
        x0 = torch.zeros(shape, device=dev)
        runs = {f"lib_{m}_steps_per_s": (lambda m=m: lib_steps(cas[m], x0.clone())) for m in cas}
        runs["torch_steps_per_s"] = lambda: torch_steps(x0.clone())
        if name == "render_256":
            for (m, k), c in cas_k.items():
                runs[f"lib_{m}_k{k}_steps_per_s"] = (lambda c=c: lib_steps(c, x0.clone()))
            for m in cas:
                runs[f"lib_{m}_frames_per_s"] = (lambda m=m: lib_frames(cas[m], x0.clone()))
        else:
            for m in cas:
                runs[f"lib_{m}_forward_keep_steps_per_s"] = (lambda m=m: lib_keep(cas[m], x0.clone()))
            runs["lib_f32_keep_and_vjp_iters_per_s"] = lambda: lib_iter(cas["f32"], x0.clone())
            runs["torch_autograd_iters_per_s"] = lambda: torch_iter(x0.clone())
            for dt in styles:
                runs[f"lib_train_step_vgg_{dt}_iters_per_s"] = (lambda dt=dt: lib_train(dt, x0.clone()))
            runs["torch_train_iteration_iters_per_s"] = lambda: torch_train(x0.clone())
        for fn in runs.values():
            fn()                                              # warm-up: every shape and path of the timed window
        rates = {k: [] for k in runs}
        for _ in range(a.reps):
            for k, fn in runs.items():
                work = n // 10 if k.endswith("iters_per_s") else n if k.endswith("frames_per_s") else (n // 2) * 64 if "keep" in k else n * 32
                rates[k].append(work / timed(fn))
        out[name] = {k: spread(v) for k, v in rates.items()}
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
