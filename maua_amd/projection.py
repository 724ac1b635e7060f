"""Projection of images (or prompts) into the latent space of a StyleGAN2 generator: find w / w+ and the per-layer noise maps whose
image the given losses like best, and hand them to the renderer as a palette.

The algorithm is the published one (Karras et al. 2020, "Analyzing and Improving the Image Quality of StyleGAN", appendix D, and the
projector.py that ships with StyleGAN2-ADA), restated from the publication: that code is not among the reference's files
(maua/parameterizations/stylegan.py is empty), so parity with it is unpinned.  Differences that are stated, not hidden:
  - the distance is this library's LPIPS (``LPIPSGrads``), not NVIDIA's own VGG16 feature file; any list of ``GradModule``s may stand
    in its place (``CLIPGrads`` with a ``TextPrompt`` gives text-driven latents);
  - the w-noise is drawn by the library's Philox generator (seed, stream = step), not torch's;
  - the noise maps are per sample, [B, 1, h, w], and the batch is optimised in one loop.

One step is library calls only (csrc/project.hip and the generator's own entries); torch runs no elementwise kernel inside the loop:
    maua_philox_normal -> maua_latent_expand -> forward (features kept) -> grad modules -> maua_synth_vjp_ex -> maua_latent_reduce (space w)
    -> maua_noise_reg (into the noise gradients) -> maua_adam_step (w, every map) -> maua_noise_renorm
"""
import argparse
import inspect
from math import cos, pi, sqrt
from pathlib import Path

import numpy as np
import torch

from . import _lib as L

ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8
NOISE_STREAM0 = 1 << 32     # Philox stream of layer l's initial noise maps: NOISE_STREAM0 + l (the steps' w-noise uses stream = step)


def schedule(step, num_steps, w_std, initial_learning_rate=0.1, initial_noise_factor=0.05, lr_rampdown_length=0.25,
             lr_rampup_length=0.05, noise_ramp_length=0.75):
    """(learning rate, w-noise scale) of a step, as published: the noise fades quadratically over the first ``noise_ramp_length`` of
    the run; the rate ramps up linearly over the first ``lr_rampup_length`` and down on a cosine over the last ``lr_rampdown_length``."""
    t = step / num_steps
    w_noise_scale = w_std * initial_noise_factor * max(0.0, 1.0 - t / noise_ramp_length) ** 2
    lr_ramp = min(1.0, (1.0 - t) / lr_rampdown_length)
    lr_ramp = 0.5 - 0.5 * cos(lr_ramp * pi)
    lr_ramp = lr_ramp * min(1.0, t / lr_rampup_length)
    return initial_learning_rate * lr_ramp, w_noise_scale


def adam_scalars(lr, t, betas=ADAM_BETAS):
    """(lr / (1 - beta1^t), 1 / sqrt(1 - beta2^t)) in double: maua_adam_step's two host-side factors (t = 1 for the first update)"""
    return lr / (1.0 - betas[0] ** t), 1.0 / sqrt(1.0 - betas[1] ** t)


class Projection:
    """``ws`` [B, num_ws, w_dim] (no w-noise added), ``noise`` (list of [B, 1, h, w] in layer order: the optimised maps, or with
    ``optimize_noise=False`` the maps the run drew and used), ``losses`` {name: [steps, B]} where the modules report them."""

    def __init__(self, ws, noise, losses=None):
        self.ws, self.noise, self.losses = ws, list(noise), dict(losses or {})

    def noise_kwargs(self):
        """the maps as the synthesizer wrapper takes them: G.synthesizer(latents=p.ws, **p.noise_kwargs())"""
        return {f"noise{l}": n for l, n in enumerate(self.noise)}

    def save(self, path):
        arrays = {"ws": self.ws.detach().float().cpu().numpy()}
        for l, n in enumerate(self.noise):
            arrays[f"noise{l}"] = n.detach().float().cpu().numpy()
        for k, v in self.losses.items():
            arrays[f"loss_{k}"] = torch.as_tensor(v).detach().float().cpu().numpy()
        np.savez(path, **arrays)
        return path


def load(path):
    """a Projection from ``Projection.save``'s .npz (host tensors)"""
    with np.load(path) as f:
        noise, l = [], 0
        while f"noise{l}" in f.files:
            noise.append(torch.from_numpy(f[f"noise{l}"]))
            l += 1
        losses = {k[5:]: torch.from_numpy(f[k]) for k in f.files if k.startswith("loss_")}
        return Projection(torch.from_numpy(f["ws"]), noise, losses)


def check_generator(G_synth):
    """the refusals, by name and before any work"""
    if getattr(G_synth, "architecture", "skip") != "skip":
        raise NotImplementedError(f"project: architecture {G_synth.architecture!r} has no gradient walk (only 'skip' networks are differentiated)")
    if getattr(G_synth, "_resize", None) is not None:
        raise NotImplementedError("project: the synthesizer's output_size installs a resize hook, which is not differentiated "
                                  "(maua_synth_vjp: a resize or warp hook is installed); build it at its native size")
    if G_synth.dtype == torch.float16:
        raise NotImplementedError("project: an MAUA_F16 network is not differentiated (maua_synth_vjp); use float32 or bfloat16")


def _target_tensor(targets):
    """[B, 3, H, W] in [-1, 1] from a tensor of that kind, or a list of images / paths (ImagePrompt's inputs, [0, 1] or bytes)"""
    if isinstance(targets, torch.Tensor):
        return targets.float() if targets.dim() == 4 else targets.float()[None]
    from .grad import ImagePrompt
    imgs = [ImagePrompt(path=t) if isinstance(t, (str, Path)) else ImagePrompt(img=t) for t in targets]
    return torch.cat([p()[0] for p in imgs])


def w_statistics(G_map, w_avg_samples, device="cuda"):
    """(w_avg [w_dim], w_std scalar) from ``w_avg_samples`` draws of np.random.RandomState(123) through the mapper (set-up, once)"""
    z = torch.from_numpy(np.random.RandomState(123).randn(w_avg_samples, G_map.z_dim)).float()
    w = torch.cat([G_map.forward(z[i:i + 1000].to(device), None)[:, 0].float() for i in range(0, w_avg_samples, 1000)])
    w_avg = w.mean(0)
    w_std = float(((w - w_avg) ** 2).sum().div(w_avg_samples).sqrt())
    return w_avg, w_std


def project(G, targets=None, grad_modules=None, space="w", num_steps=1000, w_avg_samples=10000, initial_learning_rate=0.1,
            initial_noise_factor=0.05, lr_rampdown_length=0.25, lr_rampup_length=0.05, noise_ramp_length=0.75,
            regularize_noise_weight=1e5, optimize_noise=True, w_init=None, seed=0, on_step=None):
    """Optimise w (``space="w"``: one row for all layers) or w+ (``"w+"``: a row per layer) and, with ``optimize_noise``, the noise
    maps of ``G`` (a StyleGAN2 generator: ``G.mapper.G_map``, ``G.synthesizer.G_synth``) under the sum of the ``grad_modules``' image
    gradients plus ``regularize_noise_weight`` times the noise regulariser.  ``targets`` ([B, 3, H, W] in [-1, 1], or a list of images
    or paths) become one ``LPIPSGrads(scale=1)`` unless ``grad_modules`` is given (then they only set the batch size, as does
    ``w_init`` [B, 1 | num_ws, w_dim]; else B = 1).  ``on_step(i, state)`` sees, BEFORE step i's update, the tensors the update reads -
    w, noise, eps, g_w, g_noise, the Adam moments m_w, v_w, m_noise, v_noise - and ws, img, lr, w_noise_scale, w_std, reg_loss (a list of [B]),
    losses: live device tensors, valid during the call (clone what you keep).  Returns a ``Projection``."""
    if space not in ("w", "w+"):
        raise ValueError(f"space must be 'w' or 'w+', got {space!r}")
    G_map, G_synth = G.mapper.G_map, G.synthesizer.G_synth
    check_generator(G_synth)
    if targets is None and grad_modules is None:
        raise ValueError("project: give targets or grad_modules")
    L.require_device()
    lib, dev = L.lib(), "cuda"
    tg = None if targets is None else L.dev_tensor(_target_tensor(targets), torch.float32)
    if grad_modules is None:
        from .grad import ContentPrompt, LPIPSGrads
        m = LPIPSGrads(scale=1)
        m.set_targets([ContentPrompt(img=tg.add(1).div(2))])
        grad_modules = [m]
    elif isinstance(grad_modules, torch.nn.Module):
        grad_modules = [grad_modules]
    num_ws, w_dim, n_layers = G_synth.num_ws, G_synth.w_dim, G_synth.num_layers
    rows = 1 if space == "w" else num_ws
    B = tg.shape[0] if tg is not None else (w_init.shape[0] if w_init is not None and torch.as_tensor(w_init).dim() == 3 else 1)
    # ---- start (set-up: torch device ops are fine here)
    w_avg, w_std = w_statistics(G_map, w_avg_samples, dev)
    start = w_avg if w_init is None else L.dev_tensor(torch.as_tensor(w_init), torch.float32)
    if start.dim() == 1:
        start = start[None, None]
    elif start.dim() == 2:
        start = start[:, None]
    if start.shape[1] not in (1, rows):
        raise ValueError(f"w_init has {start.shape[1]} rows; space {space!r} takes 1 or {rows}")
    w = start.expand(B, rows, w_dim).contiguous().clone()
    sizes = [G_synth.layer_size(l) for l in range(n_layers)]
    noise = []
    for l, (h, wd) in enumerate(sizes):
        n = torch.empty((B, 1, h, wd), device=dev)
        L.check(lib.maua_philox_normal(L.ctx(), seed, NOISE_STREAM0 + l, 0, L.ptr(n), n.numel(), 0.0, 1.0))
        noise.append(n)
    zeros = lambda t: torch.zeros_like(t)
    eps, g_w = torch.empty_like(w), torch.empty_like(w)
    m_w, v_w = zeros(w), zeros(w)
    m_n, v_n = [zeros(n) for n in noise], [zeros(n) for n in noise]
    g_noise = [torch.empty_like(n) for n in noise] if optimize_noise else []
    # (every step's regulariser values land in their own row: nothing is copied or summed inside the loop)
    reg_hist = torch.zeros((num_steps, n_layers, B), device=dev) if optimize_noise else None
    reg_loss = list(reg_hist[0]) if optimize_noise and num_steps > 0 else []
    ws = torch.empty((B, num_ws, w_dim), device=dev)
    img = torch.empty((B, 3, *G_synth.output_hw), device=dev)
    reg_bytes = max([lib.maua_noise_reg_workspace_bytes(B, h) for h, _ in sizes] + [0]) if optimize_noise else 0
    ren_bytes = max([lib.maua_noise_renorm_workspace_bytes(B, h * wd) for h, wd in sizes] + [0]) if optimize_noise else 0
    scratch = torch.empty(max(reg_bytes, ren_bytes, 256), dtype=torch.uint8, device=dev)
    if optimize_noise:
        for l, (h, wd) in enumerate(sizes):   # the regulariser's refusals (a non-square or odd-sized map), before the first step
            if h != wd:
                raise NotImplementedError(f"project: layer {l}'s noise map is {h} x {wd}; the regulariser takes square maps")
            L.check(lib.maua_noise_reg_check(L.ptr(noise[l]), B, h, None, L.ptr(g_noise[l]), L.ptr(scratch), scratch.numel()))
    reports = [("return_loss" in inspect.signature(m.forward).parameters) for m in grad_modules]
    losses = {f"{type(m).__name__}{k}": [] for k, m in enumerate(grad_modules) if reports[k]}
    t_mid = torch.tensor(500.0)
    was = G_synth._keep_features
    G_synth.keep_features(True)
    try:
        for step in range(num_steps):
            lr, w_noise_scale = schedule(step, num_steps, w_std, initial_learning_rate, initial_noise_factor, lr_rampdown_length,
                                         lr_rampup_length, noise_ramp_length)
            ctx = L.ctx()
            if optimize_noise:
                reg_loss = list(reg_hist[step])
            L.check(lib.maua_philox_normal(ctx, seed, step, 0, L.ptr(eps), eps.numel(), 0.0, 1.0))
            L.check(lib.maua_latent_expand(ctx, L.ptr(w), rows, L.ptr(eps), w_noise_scale, L.ptr(ws), B, num_ws, w_dim))
            G_synth.forward(ws, noise=noise, out=img)
            g_img, step_losses = None, {}
            for k, m in enumerate(grad_modules):
                if reports[k]:
                    g, loss = m(img, t_mid, return_loss=True)
                    step_losses[f"{type(m).__name__}{k}"] = loss
                else:
                    g = m(img, t_mid)
                if g_img is None:
                    g_img = g
                else:
                    from .ops import add
                    g_img = add(g_img, g, out=g_img)
            if optimize_noise:
                g_ws, _ = G_synth.vjp(g_img, noise=noise, noise_grad=g_noise)
            else:
                g_ws = G_synth.vjp(g_img, noise=noise)
            if space == "w":
                L.check(lib.maua_latent_reduce(ctx, L.ptr(g_ws), L.ptr(g_w), B, num_ws, w_dim))
            else:
                g_w = g_ws
            if optimize_noise:
                for l, (h, _) in enumerate(sizes):
                    L.check(lib.maua_noise_reg(ctx, L.ptr(noise[l]), B, h, regularize_noise_weight, L.ptr(reg_loss[l]), L.ptr(g_noise[l]), 1,
                                               L.ptr(scratch), scratch.numel()))
            for k, v in step_losses.items():
                losses[k].append(v)
            if on_step is not None:
                on_step(step, dict(step=step, w=w, noise=noise, eps=eps, ws=ws, img=img, g_img=g_img, g_w=g_w, g_noise=g_noise, m_w=m_w,
                                   v_w=v_w, m_noise=m_n, v_noise=v_n, lr=lr, w_noise_scale=w_noise_scale, w_std=w_std, reg_loss=reg_loss,
                                   losses=step_losses))
            step_size, inv_sqrt_bc2 = adam_scalars(lr, step + 1)
            adam = lambda p, g, m_, v_: L.check(lib.maua_adam_step(ctx, L.ptr(p), L.ptr(g), L.ptr(m_), L.ptr(v_), p.numel(), ADAM_BETAS[0],
                                                                   ADAM_BETAS[1], ADAM_EPS, step_size, inv_sqrt_bc2))
            adam(w, g_w, m_w, v_w)
            if optimize_noise:
                for l, (h, wd) in enumerate(sizes):
                    adam(noise[l], g_noise[l], m_n[l], v_n[l])
                    L.check(lib.maua_noise_renorm(ctx, L.ptr(noise[l]), B, h * wd, L.ptr(scratch), scratch.numel()))
    finally:
        G_synth.keep_features(was)
    L.check(lib.maua_latent_expand(L.ctx(), L.ptr(w), rows, None, 0.0, L.ptr(ws), B, num_ws, w_dim))
    losses = {k: torch.stack(v) for k, v in losses.items() if v}
    if optimize_noise:
        losses["noise_reg"] = reg_hist.sum(1)
    return Projection(ws, noise, losses)


# ---------------------------------------------------------------------------------------------------------------- command line
def parser():
    p = argparse.ArgumentParser(prog="python -m maua_amd.projection", description="project images or a text prompt into StyleGAN2 latent space")
    p.add_argument("--model_file", required=True)
    what = p.add_mutually_exclusive_group(required=True)
    what.add_argument("--target", nargs="+", help="image files, one projection each (a batch)")
    what.add_argument("--text", help="a CLIP text prompt instead of target images")
    p.add_argument("--space", choices=["w", "w+"], default="w")
    p.add_argument("--num_steps", type=int, default=1000)
    p.add_argument("--no_noise", action="store_true", help="leave the noise maps as drawn")
    p.add_argument("--out_dir", default="output")
    p.add_argument("--allow_random_init", action="store_true", help="run on a randomly initialised generator when model_file is 'None'")
    p.add_argument("--bpe_path", default=None, help="CLIP's BPE vocabulary file (for --text)")
    p.add_argument("--seed", type=int, default=0)
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    if args.model_file in (None, "None") and not args.allow_random_init:
        raise SystemExit("--model_file None needs --allow_random_init (a random generator has nothing to project onto)")
    from .stylegan2 import StyleGAN2
    G = StyleGAN2(None if args.model_file == "None" else args.model_file, inference=False)
    if args.text is not None:
        from .grad import CLIPGrads, TextPrompt
        kw = {} if args.bpe_path is None else dict(bpe_path=args.bpe_path)
        m = CLIPGrads(scale=1, **kw)
        m.set_targets([TextPrompt(args.text)])
        out = project(G, grad_modules=[m], space=args.space, num_steps=args.num_steps, optimize_noise=not args.no_noise, seed=args.seed)
        names = ["text"]
    else:
        side = G.synthesizer.G_synth.img_resolution
        from .grad import ImagePrompt
        tg = torch.cat([ImagePrompt(path=t, size=(side, side))()[0] for t in args.target])
        out = project(G, targets=tg, space=args.space, num_steps=args.num_steps, optimize_noise=not args.no_noise, seed=args.seed)
        names = [Path(t).stem for t in args.target]
    out_dir = Path(args.out_dir)
    out_dir.mkdir(parents=True, exist_ok=True)
    out.save(out_dir / f"projection_{'_'.join(names)[:80]}.npz")
    imgs = G.synthesizer(latents=out.ws, **out.noise_kwargs())
    from PIL import Image
    u8 = imgs.add(1).mul(127.5).clamp(0, 255).round().byte().permute(0, 2, 3, 1).cpu().numpy()
    for k in range(u8.shape[0]):
        Image.fromarray(u8[k]).save(out_dir / f"projection_{names[min(k, len(names) - 1)]}_{k}.png")
    return out


if __name__ == "__main__":
    main()
