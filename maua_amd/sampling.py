"""Latent sampling strategies of maua/GAN/sampling/ (langevin.py, jacnorm.py, __init__.py sample_latents) and the still-image path of
maua/GAN/generate_images.py, on the device: the generator's gradient to its latents is StyleGAN2.latent_grad (the hand-written
synthesis-network gradient, csrc/synth_vjp.hip), the critics are the image losses of maua_amd.grad."""
import hashlib
from math import ceil, sqrt
from pathlib import Path

import numpy as np
import torch

from . import _lib as L
from .grad import CLIPGrads, GradModule, TextPrompt


def prepare_critic(critic, allow_random_init=False, bpe_path=None):
    """A GradModule, a list of them, or a text prompt (langevin.py:26-60: CLIP ViT-B/32 against the prompt) -> [GradModule, ...]."""
    if isinstance(critic, GradModule):
        return [critic]
    if isinstance(critic, (list, tuple)) and all(isinstance(c, GradModule) for c in critic):
        return list(critic)
    if critic == "discriminator":
        raise NotImplementedError("the 'discriminator' critic needs the official StyleGAN3 repository's discriminator (langevin.py:29-32), "
                                  "which is not part of the reference tree: use a text prompt or a GradModule")
    if isinstance(critic, str):
        # (a random-init tower - plumbing tests, benchmarks - has to be told to build its text half)
        clip = CLIPGrads(scale=1, perceptors=["ViT-B/32"], allow_random_init=allow_random_init, text_tower=True if allow_random_init else None,
                         bpe_path=bpe_path)
        clip.set_targets([TextPrompt(critic)])
        return [clip]
    raise TypeError(f"critic must be a GradModule, a list of them or a text prompt, got {type(critic).__name__}")


def pad_latents(zs, bs, generator=None):
    """langevin.py:91-94: the latents padded with fresh normal draws to a multiple of the batch size"""
    l = len(zs)
    new_zs = torch.randn((bs * ceil(l / bs), zs.shape[1]), generator=generator)
    new_zs[:l] = zs.detach().float().cpu()
    return new_zs


def langevin_with_critic(G, zs, critic, bs=8, rate=0.1, noise_std=1, decay=0.25, decay_steps=200, steps=1000, log_intermediate=False,
                         generator=None, allow_random_init=False, bpe_path=None, on_step=None):
    """Discriminator Driven Latent Sampling ("Your GAN is Secretly an Energy-based Model", Che et al., arXiv:2003.06060) as
    maua/GAN/sampling/langevin.py:63-144 runs it, with an image loss as the critic:

        z <- z - 1/2 rate grad E(z) + sqrt(rate) scaler eps,   E(z) = 1/2 |z|^2 + sum_critics loss(G(z)),   eps ~ N(0, noise_std I)

    rate and scaler are multiplied by ``decay`` after every ``decay_steps`` steps (:129-131); zs are padded to a multiple of ``bs``
    with normal draws (:91-94) and the first len(zs) rows come back.  ``critic``: a maua_amd.grad.GradModule, a list of them (their
    gradients are summed), or a text prompt, which becomes CLIPGrads on ViT-B/32 with that prompt; "discriminator" raises
    NotImplementedError (the nv discriminator loader is not in the reference tree).  Every draw comes from ``generator`` (a CPU
    torch.Generator), so a seed reproduces the result bit for bit.

    The reference computes its critic's logits under torch.no_grad() (:109-115) and then differentiates
    ``-prior.log_prob(zs) - fake_logits``: the logits are constants there, so the gradient it applies is the prior's alone (z).
    This function implements the published update, in which the critic's gradient reaches z through the generator.

    ``allow_random_init`` / ``bpe_path``: maua_amd.clip.load's, for a text critic (a synthetic tower; the tokenizer's vocabulary).
    ``on_step(i, zs, grad, eps)``: optional observer (tests, logging), called with the step's latents BEFORE the update, the energy
    gradient and the noise draw.  ``log_intermediate``: save a grid of the current images per step under output/langevin_<critic>/."""
    critics = prepare_critic(critic, allow_random_init, bpe_path)
    l = len(zs)
    zs = L.dev_tensor(pad_latents(zs, bs, generator), torch.float32)
    Gs = G.synthesizer.G_synth
    was = Gs._keep_features
    Gs.keep_features(True)   # (once for the whole run: switching it frees the network's workspace)

    def loss_grad(z):
        return G.latent_grad(z, critics, space="z")[0]

    def log(i, zs):
        name = critic if isinstance(critic, str) else "critic"
        save_grid([G.forward(zs[j:j + bs]).cpu() for j in range(0, len(zs), bs)], f"output/langevin_{name}/{i:04}.png")
    try:
        zs = langevin_loop(zs, loss_grad, bs, rate, noise_std, decay, decay_steps, steps, generator, on_step, log if log_intermediate else None)
    finally:
        Gs.keep_features(was)
    return zs[:l]


def langevin_loop(zs, loss_grad, bs, rate, noise_std, decay, decay_steps, steps, generator=None, on_step=None, log=None):
    """The update of langevin_with_critic on latents already padded to a multiple of ``bs``; loss_grad(z [bs, D]) -> d loss / d z.
    Works on whatever device zs is on (the noise is drawn on the host from ``generator``)."""
    scaler = 1.0
    apply_decay = decay > 0 and decay_steps > 0
    for i in range(steps):
        grad = torch.empty_like(zs)
        for b in range(0, zs.shape[0], bs):
            grad[b:b + bs] = zs[b:b + bs] + loss_grad(zs[b:b + bs])       # d/dz (1/2 |z|^2 + loss)
        eps = (torch.randn(zs.shape, generator=generator) * sqrt(noise_std)).to(zs)   # covariance noise_std I (:87-89)
        if on_step is not None:
            on_step(i, zs, grad, eps)
        zs = zs - 0.5 * rate * grad + rate ** 0.5 * eps * scaler
        if apply_decay and (i + 1) % decay_steps == 0:
            rate *= decay
            scaler *= decay
        if log is not None:
            log(i, zs)
    return zs


def latents_seed(zs):
    """a 32-bit seed from the latents' bytes (jacnorm.py:35 seeds its extra draws from a hash of zs)"""
    return int.from_bytes(hashlib.sha256(np.ascontiguousarray(zs.detach().float().cpu().numpy()).tobytes()).digest()[:4], "little")


@torch.no_grad()
def jacobian_norm_rejection(G, zs, ratio=0.7, N=10, sigma=1e-3):
    """Jacobian-based truncation ("Learning Disconnected Manifolds: a no GAN's land", Tanielian et al., arXiv:2006.04596), jacnorm.py:14-47:
    ceil(len / ratio) candidates (zs plus draws seeded from the latents themselves - the reference hands RandomState the None that
    random.seed() returns, i.e. an unseeded stream), each scored by mean |G(z + eps) - G(z)|^2 / sigma^2 over N perturbations
    eps ~ N(0, sigma^4) (torch.normal(0, sigma ** 2), :43); the ceil(ratio * candidates) lowest scores are kept.  Forward only."""
    d = G.z_dim
    n_extra = ceil(len(zs) / ratio) - len(zs) + 1
    extra = torch.from_numpy(np.random.RandomState(latents_seed(zs)).randn(n_extra, d)[1:]).float()
    zs = L.dev_tensor(torch.cat((zs.detach().float().cpu(), extra)), torch.float32)
    g = torch.Generator().manual_seed(latents_seed(zs))
    jacnorms = []
    for z in zs[:, None]:
        eps = (torch.randn((N, d), generator=g) * sigma ** 2).to(zs.device)
        jacnorms.append(float(torch.mean(torch.norm(G.forward(z + eps) - G.forward(z)) ** 2 / sigma ** 2)))
    idxs = torch.argsort(torch.tensor(jacnorms))
    return zs[idxs[:ceil(ratio * len(zs))].to(zs.device)]


def sample_latents(G, seeds, batch_size, truncation, how, langevin_critic, **langevin_kwargs):
    """maua/GAN/sampling/__init__.py:9-26"""
    base_zs = torch.cat([torch.from_numpy(np.random.RandomState(seed).randn(1, G.z_dim)) for seed in seeds]).float()
    if how.startswith("langevin"):
        return langevin_with_critic(G, base_zs, langevin_critic, bs=batch_size, **langevin_kwargs)
    if how == "jacobian":
        return jacobian_norm_rejection(G, base_zs, ratio=truncation)
    if how == "polarity":
        raise NotImplementedError()
    return base_zs


def generate_images(G, seeds, class_idx=None, truncation=1.0, latent_sampling="standard", langevin_critic="discriminator", translation=None,
                    rotation=None, batch_size=8, **langevin_kwargs):
    """maua/GAN/generate_images.py:19-49 for StyleGAN2 generators: yields one [1, 3, H, W] image in [0, 1] (CPU) per latent."""
    if class_idx is not None:
        raise NotImplementedError("class conditioning is not on the render path")
    if translation is not None or rotation is not None:
        raise NotImplementedError("translation / rotation are StyleGAN3's input transform")
    latents = sample_latents(G, seeds, batch_size, truncation, latent_sampling, langevin_critic, **langevin_kwargs)
    for i in range(0, len(latents), batch_size):
        z = L.dev_tensor(latents[i:i + batch_size], torch.float32)
        ws = G.mapper(z, truncation=truncation if latent_sampling == "standard" else 1)
        for img in G.synthesizer(ws)[:, None]:
            yield img.add(1).div(2).cpu()


def tile_grid(imgs, nrow):
    """[N, 3, H, W] -> [1, 3, rows H, nrow W], row-major, the missing cells black"""
    n, c, h, w = imgs.shape
    rows = ceil(n / nrow)
    out = torch.zeros((1, c, rows * h, nrow * w), dtype=imgs.dtype)
    for k in range(n):
        r, q = divmod(k, nrow)
        out[0, :, r * h:(r + 1) * h, q * w:(q + 1) * w] = imgs[k]
    return out


def save_grid(img_batches, path, nrow=None):
    """images in [-1, 1] -> one tiled PNG"""
    from .image import save_image
    imgs = torch.cat([b.float().cpu() for b in img_batches])
    save_image(tile_grid(imgs, nrow or max(1, round(sqrt(len(imgs)) * 4 / 3))), path)


def parse_seed_list(text):
    """generate_images.py:72: '1,3,5,6-10' (a range excludes its end)"""
    return sum([([int(s)] if "-" not in s else list(range(int(s.split("-")[0]), int(s.split("-")[1])))) for s in text.split(",")], [])


def output_name(args, res):
    """generate_images.py:98-106"""
    out_size = tuple(int(s) for s in args.out_size.split(","))
    name = Path(str(args.model_file).replace("/network-snapshot", "")).stem
    if out_size[0] != res or out_size[1] != res:
        name += f"_{args.resize_strategy}@{args.resize_layer}_{out_size[0]}x{out_size[1]}"
    if args.latent_sampling != "standard":
        name += f"_{args.latent_sampling}"
        if args.latent_sampling == "langevin":
            name += f":{args.langevin_critic}"
    if args.truncation != 1.0:
        name += f"_trunc{args.truncation}"
    return name


def build_parser():
    # fmt: off
    import argparse
    parser = argparse.ArgumentParser()
    parser.add_argument("--model_file", required=True, type=str, help="Path to .pkl/.pt file containing the model to use ('None': a random-init network)")
    parser.add_argument("--architecture", default="stylegan2", type=str, choices=["stylegan2"], help="The architecture of the model")
    parser.add_argument("--seeds", default="42", type=str, help="Comma separated list of seeds to generate images for. Use a dash to specify a range: e.g. '1,3,5,6-10'")
    parser.add_argument("--class_idx", default=None, type=int, help="Index of class to generate (only applicable to conditional models)")
    parser.add_argument("--truncation", default=1.0, type=float, help="Latent truncation value. Lower values give higher quality with less diversity; higer values vice versa")
    parser.add_argument("--latent_sampling", default="standard", choices=["standard", "langevin", "polarity", "jacobian"], type=str, help="Strategy used to sample latents")
    parser.add_argument("--langevin_critic", default="discriminator", type=str, help="Critic to use for langevin latent sampling: a text prompt for CLIP-guided langevin sampling")
    parser.add_argument("--langevin_steps", default=1000, type=int, help="Steps of langevin sampling")
    parser.add_argument("--bpe_path", default=None, type=str, help="CLIP's BPE vocabulary file for a text critic (default: ~/.cache/clip/)")
    parser.add_argument("--allow_random_init", action="store_true", help="Let the CLIP critic run without a checkpoint (random weights: plumbing tests)")
    parser.add_argument("--batch_size", default=8, type=int, help="Batch size")
    parser.add_argument("--out_size", default="1024,1024", type=str, help="Desired width,height of output image: e.g. 1920,1080 or 720,1280")
    parser.add_argument("--resize_strategy", default="stretch", type=str, help="Strategy used to resize (in feature space) to achieve desired output resolution")
    parser.add_argument("--resize_layer", default=0, choices=list(range(18)), type=int, help="Which layer in the network to perform resizing at")
    parser.add_argument("--grid", action="store_true", help="Whether to output images together as a grid, rather than image by image")
    parser.add_argument("--out_dir", default="./output/", type=str, help="Directory to output images in")
    # fmt: on
    return parser


def main(argv=None):
    """the command line of maua/GAN/generate_images.py:52-117 (StyleGAN2; images are written as PNG)"""
    from .image import save_image
    from .stylegan2 import get_generator_class
    args = build_parser().parse_args(argv)
    seeds = parse_seed_list(args.seeds)
    out_size = tuple(int(s) for s in args.out_size.split(","))
    G = get_generator_class(args.architecture)(model_file=args.model_file, output_size=out_size, strategy=args.resize_strategy,
                                               layer=args.resize_layer)
    kw = dict(steps=args.langevin_steps, allow_random_init=args.allow_random_init, bpe_path=args.bpe_path) if args.latent_sampling == "langevin" else {}
    imgs = generate_images(G, seeds, args.class_idx, args.truncation, args.latent_sampling, args.langevin_critic,
                           batch_size=args.batch_size, **kw)
    name = output_name(args, G.res)
    written = []
    if args.grid:
        imgs = torch.cat(list(imgs))
        path = Path(args.out_dir) / f"seeds{args.seeds}_{name}.png"
        save_image(tile_grid(imgs, max(1, round(sqrt(len(seeds)) * 4 / 3))) * 2 - 1, path)
        written.append(path)
    else:
        for seed, img in zip(seeds, imgs):
            path = Path(args.out_dir) / f"seed{seed}_{name}.png"
            save_image(img * 2 - 1, path)
            written.append(path)
    return written


if __name__ == "__main__":
    main()
