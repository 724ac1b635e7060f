"""The reference's image parameterisation protocol (maua/parameterizations/__init__.py:5-46: a tensor that ``decode``s to an image,
``encode`` that fits it to one, and an optional debiased running average of it) for StyleGAN2 latents.  The reference leaves its own
stylegan.py empty; here ``encode`` is latent-space projection (maua_amd.projection) and the tensor is ws [B, num_ws, w_dim].

The "rgb" and "vqgan" parameterisations of the reference are not part of this library: ``load_parameterization`` names them when it
refuses them."""
import torch


class Parameterization(torch.nn.Module):
    """height, width: the decoded image's size; tensor: what is optimised.  With ``ema`` a running average of the tensor is kept the way
    the reference keeps it: accum <- accum decay (from 1); biased <- biased decay + (1 - decay) tensor (from 0); average = biased / (1 -
    accum) - the debiased mean, equal to the tensor itself after the first update."""

    def __init__(self, height, width, tensor, ema=False, decay=0.99):
        super().__init__()
        self.h, self.w = height, width
        self.tensor = torch.nn.Parameter(tensor)
        self.ema = ema
        if ema:
            self.decay = decay
            self.register_buffer("biased", torch.zeros_like(tensor))
            self.register_buffer("average", torch.zeros_like(tensor))
            self.register_buffer("accum", torch.tensor(1.0))
            self.update_ema()

    def encode(self, tensor):
        raise NotImplementedError()

    def decode(self, tensor=None):
        raise NotImplementedError()

    @torch.no_grad()
    def update_ema(self):
        if not self.ema:
            return
        self.accum.mul_(self.decay)
        self.biased.mul_(self.decay).add_((1 - self.decay) * self.tensor)
        self.average.copy_(self.biased).div_(1 - self.accum)

    @torch.no_grad()
    def reset_ema(self):
        if not self.ema:
            return
        self.biased.zero_()
        self.average.zero_()
        self.accum.fill_(1.0)
        self.update_ema()

    def decode_average(self):
        return self.decode(self.average) if self.ema else self.decode()


class StyleGANParameterization(Parameterization):
    """ws of a StyleGAN2 generator ``G`` (maua_amd.stylegan2.StyleGAN2).  ``encode(image)`` projects [B, 3, H, W] in [-1, 1] into the
    generator's latent space (``project_kwargs`` reach maua_amd.projection.project) and keeps the noise maps it found; ``decode`` renders
    the tensor (or the one given) with them."""

    def __init__(self, G, height=None, width=None, tensor=None, ema=False, decay=0.99, **project_kwargs):
        G_synth = G.synthesizer.G_synth
        if tensor is None:
            tensor = torch.zeros(1, G_synth.num_ws, G_synth.w_dim)
        side = G_synth.img_resolution
        super().__init__(side if height is None else height, side if width is None else width, tensor, ema, decay)
        self.__dict__["G"] = G       # (not a sub-module: the generator's parameters are not this module's)
        self.project_kwargs = project_kwargs
        self.noise = None

    @torch.no_grad()
    def encode(self, tensor):
        from .projection import project
        out = project(self.G, targets=tensor, **self.project_kwargs)
        self.tensor.data = out.ws.detach().to(self.tensor.device if self.tensor.is_cuda else out.ws.device)
        self.noise = out.noise
        if self.ema:
            self.biased.data, self.average.data = torch.zeros_like(self.tensor.data), torch.zeros_like(self.tensor.data)
            self.accum.data = self.accum.data.to(self.tensor.device)
            self.reset_ema()
        return out

    def decode(self, tensor=None):
        ws = self.tensor if tensor is None else tensor
        noise = {} if self.noise is None else {f"noise{l}": n for l, n in enumerate(self.noise)}
        return self.G.synthesizer(latents=ws.detach(), **noise)


def load_parameterization(which):
    """maua/parameterizations/__init__.py:53-59, with the name the reference left empty"""
    if which == "stylegan":
        return StyleGANParameterization
    if which in ("rgb", "vqgan"):
        raise NotImplementedError(f"parameterization {which!r} is the reference's (maua/parameterizations/{which}.py) and is not part of this "
                                  "library; 'stylegan' is")
    raise Exception(f"Parameterization {which} not recognized!")
