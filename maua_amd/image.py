"""The multi-resolution image pipeline around guided diffusion (maua/diffusion/image.py:30-74, 132-323) and the image operators it
runs between two scales (maua/ops/image.py:15-71, 105-173; maua/ops/noise.py:90-132), each a library call (csrc/image_ops.hip).

Same names, keyword arguments, defaults and order of operations as the reference.  What differs, on purpose:
  * images stay on the device between scales (the reference's ``.cpu()`` after the resize, :180, and the ``.to(dev)`` per batch are not
    reproduced).  With ``super_res=None`` and hooks that are library calls (``match_histogram``, ``sharpen``), no torch kernel
    runs between two sampler calls: every prompt (content, style per scale, text, image) is built before the first scale, and the
    ``max_batch`` pieces are joined by device-to-device copies, not ``torch.cat``.  The RealESRGAN route and user hooks run what
    they run;
  * ``diffusion``: "guided" or a processor instance; the latent / stable / glide / glid3xl processors are other networks and raise;
  * ``super_res``: None / "None" or a RealESRGAN name of ``maua_amd.super`` - anything else (the reference's default
    "SwinIR-M-DFO-GAN" included) raises when the schedule is set up, not at the second scale; the reference's swallowing of
    out-of-memory errors around the up-scaler (:170-177) is not reproduced;
  * a size the sampler's network cannot take is refused before any sampling.
"""
import ctypes as C
import math
from functools import partial
from pathlib import Path
from typing import Callable, Dict, List, Optional, Tuple, Union
from uuid import uuid4

import numpy as np
import torch

from . import _lib as L
from .diffusion import GuidedDiffusion, get_diffusion_model
from .grad import ContentPrompt, ImagePrompt, StylePrompt, TextPrompt

SUPPORTED_DIFFUSION = ("guided",)
OTHER_PROCESSORS = ("latent", "stable", "glide", "glid3xl")


# ======================================================================================================== operators
def _cubic(x):
    """resize_right interp_methods.cubic (support 4)."""
    a = x.abs()
    a2, a3 = a ** 2, a ** 3
    return ((1.5 * a3 - 2.5 * a2 + 1.0) * (a <= 1.0).to(x.dtype)
            + (-0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0) * ((1.0 < a) & (a <= 2.0)).to(x.dtype))


def _lanczos3(x):
    """resize_right interp_methods.lanczos3 (support 6)."""
    eps = torch.finfo(torch.float32).eps
    return ((torch.sin(math.pi * x) * torch.sin(math.pi * x / 3) + eps) / ((math.pi ** 2 * x ** 2 / 3) + eps)) * (x.abs() < 3).to(x.dtype)


INTERP_METHODS = {"cubic": (_cubic, 4.0), "lanczos3": (_lanczos3, 6.0)}
cubic, lanczos3 = "cubic", "lanczos3"   # what the reference imports from resize_right.interp_methods, as names of the kernels here


def resize_tables(in_sz, out_sz, interp_method="cubic"):
    """One dimension of ``resize_right.resize(..., out_shape=...)`` (antialiasing, not by_convs): -> (left int32 [out_sz], the first
    input index of each output sample's field of view - may be negative or run past in_sz: zero padding; weights float32
    [out_sz, taps], normalised per output sample).  Host arithmetic in the published order, float32 tensors."""
    fn, support = INTERP_METHODS[interp_method]
    eps = torch.finfo(torch.float32).eps
    scale = out_sz / in_sz
    projected = torch.arange(out_sz) / float(scale) + (in_sz - 1) / 2 - (out_sz - 1) / (2 * float(scale))
    method = fn
    if scale < 1.0:
        method = lambda a: scale * fn(scale * a)
        support = support / scale
    left = torch.ceil(projected - support / 2 - eps).long()
    fov = left[:, None] + torch.arange(math.ceil(support - eps))
    w = method(projected[:, None] - fov)
    s = w.sum(1, keepdim=True)
    s[s == 0] = 1
    return left.int().contiguous(), (w / s).float().contiguous()


_table_cache = {}


def _device_tables(in_sz, out_sz, interp_method, device):
    key = (in_sz, out_sz, interp_method, str(device))
    t = _table_cache.get(key)
    if t is None:
        with L.host_threads(1):
            left, w = resize_tables(in_sz, out_sz, interp_method)
        if len(_table_cache) > 64:
            _table_cache.clear()
        t = _table_cache[key] = (left.to(device), w.to(device), w.shape[1])
    return t


def _image(x, name):
    x = L.dev_tensor(x, torch.float32)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"{name}: expected a [B, 3, H, W] image, got {tuple(x.shape)}")
    return x


def resize(img, out_shape, interp_method="cubic", out=None, accumulate=False, add=0.0):
    """``resize_right.resize(img, out_shape=out_shape, interp_method=...)`` on the last two dimensions of a float32 device tensor
    ([..., H, W]).  ``out`` / ``accumulate`` / ``add``: write ``resized + add`` into ``out``, or ``(out + resized) + add``."""
    if callable(interp_method):
        interp_method = getattr(interp_method, "__name__", interp_method)
    if interp_method not in INTERP_METHODS:
        raise ValueError(f"resize: interp_method must be one of {sorted(INTERP_METHODS)}, got {interp_method!r}")
    x = L.dev_tensor(img, torch.float32)
    if x.dim() < 2:
        raise ValueError("resize: needs at least two dimensions")
    H, W = int(x.shape[-2]), int(x.shape[-1])
    Ho, Wo = int(out_shape[-2]), int(out_shape[-1])
    planes = x.numel() // (H * W)
    if out is None:
        if accumulate:
            raise ValueError("resize: accumulate needs out=")
        out = torch.empty((*x.shape[:-2], Ho, Wo), dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != (*x.shape[:-2], Ho, Wo) or out.dtype != torch.float32 or not out.is_contiguous() or not out.is_cuda:
        raise ValueError("resize: out must be a contiguous float32 device tensor of the result's shape")
    ly, wy, ty = _device_tables(H, Ho, interp_method, x.device) if H != Ho else (None, None, 0)
    lx, wx, tx = _device_tables(W, Wo, interp_method, x.device) if W != Wo else (None, None, 0)
    L.check(L.lib().maua_image_resize(L.ctx(x.device), L.ptr(x), planes, H, W, L.ptr(out), Ho, Wo, L.ptr(ly), L.ptr(wy), ty, L.ptr(lx),
                                      L.ptr(wx), tx, int(bool(accumulate)), add))
    return out


def tile_origins(size, tile_size, overtile=1):
    """ops/image.py:17-21: ``torch.linspace(0, size - tile_size, n).round().long()`` with n = round(floor(size / tile_size) + overtile)."""
    n = round(np.floor(size / tile_size) + overtile)
    return [int(v) for v in torch.linspace(0, size - tile_size, n).round().long()]


def _ints(v):
    return (C.c_int * len(v))(*v)


def destitch(img, tile_size, overtile=1):
    """ops/image.py:15-23 -> [n_tiles * B, 3, tile_size, tile_size], one gather launch."""
    x = _image(img, "destitch")
    B, _, H, W = x.shape
    if tile_size > min(H, W):
        raise ValueError(f"destitch: tile_size {tile_size} exceeds the image ({H} x {W})")
    ys, xs = tile_origins(H, tile_size, overtile), tile_origins(W, tile_size, overtile)
    out = torch.empty((len(ys) * len(xs) * B, 3, tile_size, tile_size), dtype=torch.float32, device=x.device)
    L.check(L.lib().maua_image_destitch(L.ctx(x.device), L.ptr(x), B, H, W, tile_size, _ints(ys), len(ys), _ints(xs), len(xs), L.ptr(out)))
    return out


def smoothstep(x, N=2):
    """ops/image.py:26-31."""
    result = torch.zeros_like(x)
    for n in range(0, N + 1):
        result += float(math.comb(N + n, n) * math.comb(2 * N + 1, N - n)) * (-x) ** n
    result *= x ** (N + 1)
    return result


def blend_weight1d(total_size, fade_in, fade_out):
    """ops/image.py:34-41."""
    return torch.cat((smoothstep(torch.linspace(0, 1, fade_in)), torch.ones(total_size - fade_in - fade_out),
                      smoothstep(torch.linspace(1, 0, fade_out))))


def blend_tables(H, W, tile_size, overtile=1):
    """The tile origins and 1-D weights of restitch (ops/image.py:46-57) -> (ys, xs, wy [n_rows, T], wx [n_cols, T]) on the host.  As
    there, both axes fade over ``tile_size - ys[1]`` samples, and there is no fade at the image's edges."""
    ys, xs = tile_origins(H, tile_size, overtile), tile_origins(W, tile_size, overtile)
    if len(ys) < 2:
        raise ValueError("restitch: needs at least two tile rows (the reference reads ys[1])")
    fade = tile_size - ys[1]
    with L.host_threads(1):
        wy = torch.stack([blend_weight1d(tile_size, 0 if y == 0 else fade, 0 if y == ys[-1] else fade) for y in ys])
        wx = torch.stack([blend_weight1d(tile_size, 0 if x == 0 else fade, 0 if x == xs[-1] else fade) for x in xs])
    return ys, xs, wy.float().contiguous(), wx.float().contiguous()


_blend_cache = {}


def restitch(tiled, H, W, overtile=1):
    """ops/image.py:44-62 -> [1, 3, H, W], one launch (each pixel sums its covering tiles in the reference's order)."""
    t = _image(tiled, "restitch")
    n, _, T2, T = t.shape
    if T2 != T:
        raise ValueError("restitch: square tiles")
    key = (H, W, T, overtile, str(t.device))
    tab = _blend_cache.get(key)
    if tab is None:
        ys, xs, wy, wx = blend_tables(H, W, T, overtile)
        if len(_blend_cache) > 16:
            _blend_cache.clear()
        tab = _blend_cache[key] = (ys, xs, wy.to(t.device), wx.to(t.device))
    ys, xs, wy, wx = tab
    if n != len(ys) * len(xs):
        raise ValueError(f"restitch: {n} tiles for a {len(ys)} x {len(xs)} grid")
    out = torch.empty((1, 3, H, W), dtype=torch.float32, device=t.device)
    L.check(L.lib().maua_image_restitch(L.ctx(t.device), L.ptr(t), T, _ints(ys), len(ys), _ints(xs), len(xs), L.ptr(wy), L.ptr(wx),
                                        L.ptr(out), H, W))
    return out


def sharpen(img, strength):
    """ops/image.py:70-71 (torchvision ``adjust_sharpness`` around the [-1, 1] <-> [0, 1] maps), one pass."""
    x = _image(img, "sharpen")
    B, _, H, W = x.shape
    out = torch.empty_like(x)
    L.check(L.lib().maua_image_sharpen(L.ctx(x.device), L.ptr(x), B, H, W, strength, L.ptr(out)))
    return out


def _moments(x, navg, noise, noise_scale):
    """-> per frame (mean [3], second moment [3, 3], min, max) in float64 from the kernel's float32 slice sums."""
    frames = x.shape[0] // navg
    HW = x.shape[2] * x.shape[3]
    slices = L.lib().maua_image_moments_slices(HW)
    part = torch.empty((frames, slices, 11), dtype=torch.float32, device=x.device)
    L.check(L.lib().maua_image_moments(L.ctx(x.device), L.ptr(x), frames, navg, HW, L.ptr(noise), noise_scale, L.ptr(part)))
    p = part.cpu().numpy().astype(np.float64)     # (the one device -> host copy of the operator: 44 bytes per 4096 pixels)
    s = p[:, :, :9].sum(1) / HW
    out = []
    for f in range(frames):
        m2 = np.array([[s[f, 3], s[f, 4], s[f, 5]], [s[f, 4], s[f, 6], s[f, 7]], [s[f, 5], s[f, 7], s[f, 8]]])
        out.append((s[f, :3].copy(), m2, float(p[f, :, 9].min()), float(p[f, :, 10].max())))
    return out


def _sqrtm_sym(cov):
    """ops/image.py:147-150: eigh, sqrt of the eigenvalues with NaN -> 0, recomposed - in float64."""
    if not np.isfinite(cov).all():
        raise RuntimeError("match_histogram: non-finite covariance")     # (torch.linalg.eigh raises a RuntimeError there)
    eva, eve = np.linalg.eigh(cov)
    with np.errstate(invalid="ignore"):
        e = np.sqrt(eva)
    e[e != e] = 0
    return eve @ np.diag(e) @ eve.T


MATCH_NOISE_SEED = 0x6d617561   # default Philox key of match_histogram's own perturbation (stream 2 k: target of source k, 2 k + 1: source k)


def match_histogram(target_tensor, source_tensor, mode="avg", noise=None, seed=None):
    """ops/image.py:113-173, mode "avg": every target frame's colour mean / covariance moved onto the (batch-averaged) source's,
    ``Qs Qt^-1 (x - mu_t) + mu_s``, clamped to the sources' min / max.  One reduction pass per tensor (fixed-order float32 partial sums
    on the device), the 3x3 square roots and the inverse in float64 on the HOST, one apply pass.  The reference's ``1e-3 * randn``
    perturbations (:141-144) come from the library's Philox streams; ``noise = (noise_target [B, 3, H, W], noise_source [B, 3, Hs, Ws])``
    - frame b's pair, in image layout - overrides them.  ``seed``: the Philox key of the perturbation; None draws one from torch's host
    generator (``torch.randint``), so ``torch.manual_seed`` fixes the result as it does in the reference and successive calls differ;
    an int fixes it outright.  A RuntimeError in the matrix step leaves the input unmodified, as there (:167-170).
    Mode "False": identity; other modes raise."""
    if mode == "False":
        return target_tensor
    if mode != "avg":
        raise NotImplementedError(f'match_histogram(mode="{mode}"): only "avg" and "False" are built')
    x = _image(target_tensor, "match_histogram")
    sources = source_tensor if isinstance(source_tensor, list) else [source_tensor]
    sources = [_image(s, "match_histogram") for s in sources]
    if noise is not None and len(sources) != 1:
        raise ValueError("match_histogram: explicit noise goes with a single source")
    B, _, H, W = x.shape
    HW = H * W
    out = torch.empty_like(x)
    lib, ctx = L.lib(), L.ctx(x.device)
    f3 = lambda v: (C.c_float * len(v))(*[float(u) for u in v])
    stats = [_moments(s, s.shape[0], None, 0.0)[0] for s in sources]
    lo, hi = min(st[2] for st in stats), max(st[3] for st in stats)
    eps = float(torch.finfo(torch.float32).eps)
    if noise is None and seed is None:
        seed = int(torch.randint(0, 2 ** 62, ()))
    try:
        plan = []
        for k, s in enumerate(sources):
            if noise is not None:
                nt, ns = (_image(n, "match_histogram noise") for n in noise)
                if nt.shape != x.shape or tuple(ns.shape) != (B, 3, s.shape[2], s.shape[3]):
                    raise ValueError("match_histogram: noise = (like the target, [B, 3, Hs, Ws])")
            else:
                from .rng import philox_normal
                nt = philox_normal(x.shape, seed, 2 * k, device=x.device)
                ns = philox_normal((B, 3, s.shape[2], s.shape[3]), seed, 2 * k + 1, device=x.device)
            mt = _moments(x, 1, nt, 1e-3)
            # the source's perturbation is drawn anew per target frame (:142-144): frame b's statistics use noise_source[b]
            ms = [_moments(s, s.shape[0], ns[b:b + 1], 1e-3)[0] for b in range(B)]
            frames = []
            for b in range(B):
                mu_t, m2t = mt[b][0], mt[b][1]
                mu_s, m2s = ms[b][0], ms[b][1]
                Ct = m2t - np.outer(mu_t, mu_t) + eps * np.eye(3)
                Cs = m2s - np.outer(mu_s, mu_s) + eps * np.eye(3)
                try:
                    M = _sqrtm_sym(Cs) @ np.linalg.inv(_sqrtm_sym(Ct))
                except np.linalg.LinAlgError as e:
                    raise RuntimeError(str(e))
                frames.append((M, mu_t, mu_s))
            plan.append((nt, frames))
        for k, (nt, frames) in enumerate(plan):
            for b, (M, mu_t, mu_s) in enumerate(frames):
                L.check(lib.maua_image_match_apply(ctx, L.ptr(x[b]), L.ptr(nt[b]), 1e-3, HW, f3(M.ravel()), f3(mu_t),
                                                   f3(mu_s), 1.0 / len(plan), int(k > 0), int(k == len(plan) - 1),
                                                   lo, hi, L.ptr(out[b])))
    except RuntimeError as e:
        if isinstance(e, L.MauaHipError):
            raise
        import traceback
        traceback.print_exc()
        print("Skipping histogram matching...")
        ident, zero = f3(np.eye(3).ravel()), f3([0, 0, 0])
        for b in range(B):
            L.check(lib.maua_image_match_apply(ctx, L.ptr(x[b]), None, 0.0, HW, ident, zero, zero, 1.0, 0, 1,
                                               lo, hi, L.ptr(out[b])))
    return out


def perlin_gradients(octaves, width, height, grayscale, generator=None):
    """The draws of perlin_ms (ops/noise.py:109-121, :96): per channel, per octave one ``torch.randn(2, w + 1, h + 1, 1, 1)`` with w / h
    doubling - the reference's call shapes and order, from torch's host generator -> list (channel-major) of [2, w + 1, h + 1] tensors."""
    out = []
    for _ in range(1 if grayscale else 3):
        w, h = width, height
        for _o in octaves:
            out.append(torch.randn(2, w + 1, h + 1, 1, 1, generator=generator).reshape(2, w + 1, h + 1))
            w, h = w * 2, h * 2
    return out


def create_perlin_noise(octaves=[1, 1, 1, 1], width=2, height=2, grayscale=True, gradients=None, generator=None, return_raw=False):
    """ops/noise.py:124-132 -> [3, width * 2^n, height * 2^n] in [0, 1] on the device: the octave sum, clamp, 8-bit quantisation
    (``to_pil_image``), per-channel ``ImageOps.autocontrast`` and ``to_tensor`` in the library.  ``gradients``: perlin_gradients'
    list (else drawn here).  ``return_raw``: also perlin_ms's sum [channels, ...] before the clamp."""
    L.require_device()
    n = len(octaves)
    ch = 1 if grayscale else 3
    if gradients is None:
        with L.host_threads(1):
            gradients = perlin_gradients(octaves, width, height, grayscale, generator)
    if len(gradients) != ch * n:
        raise ValueError(f"create_perlin_noise: {ch * n} gradient tensors expected, got {len(gradients)}")
    offs, pos = [], 0
    for k, g in enumerate(gradients):
        w, h = width << (k % n), height << (k % n)
        if tuple(g.shape) != (2, w + 1, h + 1):
            raise ValueError(f"create_perlin_noise: gradient {k} must be [2, {w + 1}, {h + 1}], got {tuple(g.shape)}")
        offs.append(pos)
        pos += g.numel()
    flat = torch.cat([g.reshape(-1).float() for g in gradients]).to("cuda")
    S_r, S_c = width << n, height << n
    out = torch.empty((3, S_r, S_c), dtype=torch.float32, device=flat.device)
    raw = torch.empty((ch, S_r, S_c), dtype=torch.float32, device=flat.device) if return_raw else None
    octs = (C.c_float * n)(*[float(o) for o in octaves])
    L.check(L.lib().maua_image_perlin(L.ctx(flat.device), L.ptr(flat), (C.c_long * len(offs))(*offs), octs, n, width, height, int(grayscale),
                                      L.ptr(raw), L.ptr(out)))
    return (out, raw) if return_raw else out


# ======================================================================================================== pipeline
def round64(x):
    return round(x / 64) * 64


def width_height(arg: str):
    w, h = arg.split(",")
    return int(h), int(w)


def build_output_name(init=None, style=None, text=None, image=None, unique=True):
    out_name = str(uuid4())[:6] if unique else "video"
    if text is not None:
        out_name = f"{text.replace(' ', '_')}_{out_name}"
    if image is not None:
        out_name = f"{Path(image).stem}_{out_name}"
    if style is not None:
        out_name = f"{Path(style).stem}_{out_name}"
    if init is not None:
        out_name = f"{Path(init).stem}_{out_name}"
    return out_name


def get_start_steps(skips, diffusion):
    start_steps = np.argmax(
        diffusion.original_num_steps * (1 - np.array(skips)[:, None])
        <= np.array(list(diffusion.timestep_map[1:]) + [diffusion.original_num_steps])[None, :],
        axis=1,
    )
    return start_steps


def load_image(path):
    """``to_tensor(Image.open(path).convert("RGB"))`` -> HWC uint8 array (ImagePrompt and initialize_image scale it)."""
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def initialize_image(init, shape):
    """diffusion/image.py:61-74 -> [1, 3, H, W] on the device ("random": torch's host generator, as there; "perlin": the gradient draws
    from it, everything else in the library)."""
    if init == "random":
        img = torch.randn((1, 3, *shape)).to("cuda")
    elif init == "perlin":
        a = create_perlin_noise([1.5 ** -i * 0.5 for i in range(12)], 1, 1, False)
        img = resize(a, out_shape=shape)
        del a
        b = create_perlin_noise([1.5 ** -i * 0.5 for i in range(8)], 4, 4, True)
        img = resize(b, out_shape=shape, out=img, accumulate=True, add=-1.0).unsqueeze(0)
    elif init is not None:
        img = resize(ImagePrompt(img=load_image(init)).img, out_shape=shape)
    else:
        raise Exception("init strategy not recognized!")
    return img


def check_super_res(name, load=False, allow_random_init=False):
    """-> None or a RealESRGAN name ``maua_amd.super.load_model`` serves; everything else raises (the SwinIR / latent-diffusion
    up-scalers of maua.super.image are not part of this build).  ``load``: build the up-scaler now, so that a missing checkpoint
    raises here and not at the second scale (``allow_random_init``: seeded random weights instead)."""
    if name is None or name == "None" or name is False:
        return None
    if not isinstance(name, str):
        return name          # a ready up-scaler (maua_amd.super.RealESRGANer)
    from .super import BLOCKS
    known = sorted(BLOCKS) + ["xsx4-animevideo"]
    if name not in known:
        raise NotImplementedError(f'super_res="{name}" is not built (the RealESRGAN models are: {known}); pass super_res=None for plain '
                                  f'lanczos3 resizing between scales')
    if load:
        load_upscaler(name, allow_random_init)
    return name


_upscalers = {}


def load_upscaler(model_name, allow_random_init=False):
    from . import super as SR
    m = _upscalers.get(model_name)
    if m is None:
        m = _upscalers[model_name] = SR.load_model(model_name, allow_random_init=allow_random_init)
    return m


def upscale_image(img, model_name, allow_random_init=False):
    """maua/super/image/single.py ``upscale_image`` for the RealESRGAN models: [1, 3, H, W] in [0, 1] -> x 4.  ``model_name``: a name
    of ``maua_amd.super.load_model`` or a ready ``RealESRGANer``.  (Through ``RealESRGANer.enhance``'s host arrays, as
    ``maua_amd.super.upscale`` goes.)"""
    from . import super as SR
    m = load_upscaler(model_name, allow_random_init) if isinstance(model_name, str) else model_name
    return torch.cat(list(SR.upscale([im.unsqueeze(0) for im in img], m))).to(img.device)


def check_sizes(diffusion, shapes, tile_size, stitch):
    """What runs un-tiled must be a size the sampler's network takes: maua_unet_forward accepts any H x W that are multiples of
    2^(levels - 1) (its image_size is the training size, not a limit), so round64's multiples of 64 pass for up to 7 levels; a tile
    must be such a size as well."""
    model = getattr(diffusion, "model", None)
    down = 2 ** (len(model.channel_mult) - 1) if hasattr(model, "channel_mult") else 1
    for h, w in shapes:
        if h <= 0 or w <= 0:
            raise ValueError(f"size {w}x{h} rounds to nothing: sizes are rounded to multiples of 64")
        tiled = stitch and min(h, w) > tile_size
        sizes = (tile_size, tile_size) if tiled else (h, w)
        if any(s % down for s in sizes):
            what = f"tile size {tile_size}" if tiled else f"size {w}x{h}"
            raise ValueError(f"{what}: the diffusion network takes multiples of {down} only")


def join_batches(parts):
    """``torch.cat(parts)`` along dimension 0 as device-to-device copies: contiguous pieces of one dtype go into slices of one
    buffer with ``copy_`` (a memory copy, no kernel); anything else falls back to ``torch.cat``."""
    first = parts[0]
    if not all(p.is_cuda and p.is_contiguous() and p.dtype == first.dtype and p.shape[1:] == first.shape[1:] for p in parts):
        return torch.cat(parts)
    out = torch.empty((sum(p.shape[0] for p in parts), *first.shape[1:]), dtype=first.dtype, device=first.device)
    at = 0
    for p in parts:
        out[at:at + p.shape[0]].copy_(p)
        at += p.shape[0]
    return out


class MultiResolutionDiffusionProcessor(torch.nn.Module):
    def forward(
        self,
        diffusion,
        init: str,
        text: Optional[str] = None,
        image: Optional[str] = None,
        content: Optional[str] = None,
        style: Optional[str] = None,
        schedule: Dict[Tuple[int, int], float] = {(512, 512): 0.5},
        pre_hook: Optional[Callable] = None,
        post_hook: Optional[Callable] = None,
        super_res_model: Optional[str] = None,
        tile_size: Optional[int] = None,
        stitch: bool = True,
        max_batch: int = 4,
        verbose: bool = True,
        allow_random_init: bool = False,
    ):
        shapes = [(round64(h), round64(w)) for h, w in list(schedule.keys())]
        t_starts = list(schedule.values())

        if tile_size is None:
            tile_size = diffusion.image_size
        super_res_model = check_super_res(super_res_model, load=len(shapes) > 1, allow_random_init=allow_random_init)
        check_sizes(diffusion, shapes, tile_size, stitch)

        # initialize image
        img = initialize_image(init, shapes[0])
        if content is None:
            content = dict(img=img.clone())
        else:
            content = dict(path=content)

        # every prompt is built here, before the first scale: the reference builds them inside the loop from the same arguments
        # (image.py:190-197); here that would put torch's elementwise kernels between two sampler calls
        content_prompt = ContentPrompt(**content)
        style_prompts = [StylePrompt(path=style, size=shape) for shape in shapes] if style is not None else None
        text_prompt = TextPrompt(text) if text is not None else None
        image_prompt = ImagePrompt(path=image) if image is not None else None

        for scale, t_start in enumerate(t_starts):
            if verbose:
                print(f"Current size: {shapes[scale][1]}x{shapes[scale][0]}")

            if scale != 0:
                # maybe upsample image with super-resolution model
                if super_res_model:
                    img = upscale_image(img.add(1).div(2), model_name=super_res_model).mul(2).sub(1)

                # resize image for next scale (stays on the device)
                img = resize(img, out_shape=shapes[scale], interp_method=lanczos3)

            if pre_hook:  # user-supplied pre-processing function
                img = pre_hook(img)

            # if the image is larger than specified size, chop it into tiles
            needs_stitching = stitch and min(shapes[scale]) > tile_size
            if needs_stitching:
                img = destitch(img, tile_size=tile_size)

            # initialize prompts for diffusion (we don't support stitched content yet)
            prompts = [content_prompt] if not needs_stitching else []
            if style is not None:
                prompts.append(style_prompts[scale])
            if text is not None:
                prompts.append(text_prompt)
            if image is not None:
                prompts.append(image_prompt)

            # run diffusion sampling (in multiple batches if necessary)
            if img.shape[0] > max_batch:
                tiles = img.split(max_batch)
                if verbose:
                    from tqdm import tqdm
                    tiles = tqdm(tiles)
                img = join_batches([diffusion(ims, prompts, t_start, verbose=False) for ims in tiles])
            else:
                img = diffusion(img, prompts, t_start, verbose=verbose)

            # reassemble image tiles to final image
            if needs_stitching:
                img = restitch(img, *shapes[scale])

            if post_hook:  # user-supplied post-processing function
                img = post_hook(img)

        return img


@torch.no_grad()
def image_sample(
    init: str = "random",
    text: Optional[str] = None,
    image: Optional[str] = None,
    content: Optional[str] = None,
    style: Optional[str] = None,
    sizes: List[Tuple[int, int]] = [(512, 512)],
    skips: List[float] = [0.0],
    timesteps: int = 50,
    super_res: str = "SwinIR-M-DFO-GAN",
    stitch: bool = False,
    tile_size: Optional[int] = None,
    max_batch: int = 4,
    diffusion="guided",
    sampler: str = "plms",
    guidance_speed: str = "fast",
    clip_scale: float = 0.0,
    lpips_scale: float = 0.0,
    style_scale: float = 0.0,
    color_match_scale: float = 0.0,
    cfg_scale: float = 5.0,
    match_hist: bool = False,
    sharpness: float = 0.0,
    device: str = "cuda",
    number: int = 1,
    guided_kwargs=None,
    text_encoder=None,
    clip_models=None,
):
    """diffusion/image.py:217-282.  ``guided_kwargs`` / ``text_encoder`` / ``clip_models`` reach ``get_diffusion_model`` (ready networks,
    ``allow_random_init``: there are no checkpoints in the image)."""
    rnd = bool((guided_kwargs or {}).get("allow_random_init"))
    super_res = check_super_res(super_res, load=len(sizes) > 1, allow_random_init=rnd)      # before any other network is built
    if isinstance(diffusion, str) and diffusion in OTHER_PROCESSORS:
        raise NotImplementedError(f'diffusion="{diffusion}": the latent / stable / glide / glid3xl processors are not built; "guided" or a '
                                  f'processor instance')
    assert len(sizes) == len(skips), "`sizes` and `skips` must have equal length!"
    if isinstance(diffusion, str):
        diffusion = get_diffusion_model(
            diffusion=diffusion,
            timesteps=timesteps,
            sampler=sampler,
            guidance_speed=guidance_speed,
            clip_scale=clip_scale,
            lpips_scale=lpips_scale,
            style_scale=style_scale,
            color_match_scale=color_match_scale,
            cfg_scale=cfg_scale,
            image=image,
            guided_kwargs=guided_kwargs,
            text_encoder=text_encoder,
            clip_models=clip_models,
            text=text,
        )

    pre_hook = partial(match_histogram, source_tensor=StylePrompt(path=style).img) if match_hist else None
    post_hook = partial(sharpen, strength=sharpness) if sharpness > 0 else None

    schedule = {shape: skip for shape, skip in zip(sizes, skips)}

    processor = MultiResolutionDiffusionProcessor()
    imgs = [
        processor(
            diffusion=diffusion.to(device) if hasattr(diffusion, "to") else diffusion,
            init=init,
            text=text,
            image=image,
            content=content,
            style=style,
            schedule=schedule,
            pre_hook=pre_hook,
            post_hook=post_hook,
            super_res_model=super_res,
            tile_size=tile_size,
            stitch=stitch,
            max_batch=max_batch,
            allow_random_init=rnd,
        )
        for _ in range(number)
    ]
    return imgs[0] if len(imgs) == 1 else imgs


def save_image(img, path):
    """[1, 3, H, W] in [-1, 1] -> PNG (maua/ops/io.py save_image's role for one image), through PIL."""
    from PIL import Image
    u8 = img.detach().float().squeeze(0).add(1).div(2).clamp(0, 1).mul(255).round().byte().permute(1, 2, 0).cpu().numpy()
    Path(path).parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(u8).save(path)


def build_parser():
    # fmt:off
    import argparse
    parser = argparse.ArgumentParser(formatter_class=argparse.ArgumentDefaultsHelpFormatter, allow_abbrev=True)
    parser.add_argument("--init", type=str, default="random", help='How to initialize the image "random", "perlin", or a path to an image file.')
    parser.add_argument("--text", type=str, default=None, help='A text prompt to visualize.')
    parser.add_argument("--image", type=str, default=None, help='An image prompt to use (overrides --text and uses Justin Pinkney\'s image conditioned Stable Diffusion model).')
    parser.add_argument("--content", type=str, default=None, help='A content image whose structure to adapt in the output image (only works with "guided" diffusion at the moment, see --lpips-scale).')
    parser.add_argument("--style", type=str, default=None, help='An image whose style should be optimized for in the output image (only works with "guided" diffusion at the moment, see --style-scale).')
    parser.add_argument("--sizes", type=width_height, nargs="+", default=[(512, 512)], help='Sequence of sizes to synthesize the image at.')
    parser.add_argument("--skips", type=float, nargs="+", default=[0], help='Sequence of skip fractions for each size. Lower fractions will stray further from the original image, while higher fractions will hallucinate less detail.')
    parser.add_argument("--timesteps", type=int, default=50, help='Number of timesteps to sample the diffusion process at. Higher values will take longer but are generally of higher quality.')
    parser.add_argument("--super-res", type=str, default="SwinIR-M-DFO-GAN", help='Super resolution model to upscale intermediate results with before applying next diffusion resolution (see maua.super.image --model-help for full list of possibilities, None to perform simple resizing).')
    parser.add_argument("--stitch", action="store_true", help='Enable tiled synthesis of images which are larger than the specified --tile-size.')
    parser.add_argument("--tile-size", type=int, default=None, help='The maximum size of tiles the image is cut into.')
    parser.add_argument("--max-batch", type=int, default=4, help='Maximum batch of tiles to synthesize at one time (lower values use less memory, but will be slower).')
    parser.add_argument("--diffusion", type=str, default="stable", help='Which diffusion model to use. Options: "guided", "latent", "glide", "glid3xl", "stable" or a /path/to/stable-diffusion.ckpt')
    parser.add_argument("--sampler", type=str, default="lms", choices=["p", "ddim", "plms", "euler", "euler_ancestral", "heun", "dpm_fast", "dpm_adaptive", "dpm_2", "dpm_2_ancestral", "lms"], help='Which sampling method to use. "p", "ddim", and "plms" work for all diffusion models, the rest are currently only supported with "stable" diffusion.')
    parser.add_argument("--guidance-speed", type=str, default="fast", choices=["regular", "fast"], help='How to perform "guided" diffusion. "regular" is slower but can be higher quality, "fast" corresponds to the secondary model method (a.k.a. Disco Diffusion).')
    parser.add_argument("--clip-scale", type=float, default=0.0, help='Controls strength of CLIP guidance when using "guided" diffusion.')
    parser.add_argument("--lpips-scale", type=float, default=0.0, help='Controls the apparent influence of the content image when using "guided" diffusion and a --content image.')
    parser.add_argument("--style-scale", type=float, default=0.0, help='When using "guided" diffusion and a --style image, a higher --style-scale enforces textural similarity to the style, while a lower value will be conceptually similar to the style.')
    parser.add_argument("--color-match-scale", type=float, default=0.0, help='When using "guided" diffusion, the --color-match-scale guides the output\'s colors to match the --style image.')
    parser.add_argument("--cfg-scale", type=float, default=7.5, help='Classifier-free guidance strength. Higher values will match the text prompt more closely at the cost of output variability.')
    parser.add_argument("--match-hist", action="store_true", help='Match the histogram of the initialization image to the --style image before starting diffusion.')
    parser.add_argument("--sharpness", type=float, default=0.0, help='Sharpen the image by this amount after each diffusion scale (a value of 1.0 will leave the image unchanged, higher values will be sharper).')
    parser.add_argument("--device", type=str, default="cuda", help='Which device to use (e.g. "cpu" or "cuda:1")')
    parser.add_argument("--number", type=int, default=1, help='How many images to render.')
    parser.add_argument("--out-dir", type=str, default="output/", help='Directory to save output images to.')
    # fmt:on
    return parser


def main(argv=None):
    """``python -m maua.diffusion.image``: the reference's flags (:285-322).  Not in the reference: when the guided-diffusion
    checkpoints are missing, MAUA_ALLOW_RANDOM_INIT=1 in the environment runs with randomly initialised networks (smoke runs)."""
    import os
    args = build_parser().parse_args(argv)
    if args.sampler == "lms" and args.diffusion == "guided":
        args.sampler = "plms"      # the CLI's default sampler is a "stable"-only one; image_sample's own default for "guided"
    out_name = build_output_name(args.init, args.style, args.text, args.image)[:222]
    out_dir = args.out_dir
    del args.out_dir
    kw = vars(args)
    if os.environ.get("MAUA_ALLOW_RANDOM_INIT") == "1":
        kw["guided_kwargs"] = dict(allow_random_init=True)
    imgs = image_sample(**kw)
    imgs = imgs if isinstance(imgs, list) else [imgs]
    for i, img in enumerate(imgs):
        path = f"{out_dir}/{Path(args.diffusion).stem}_{out_name}{i}.png"
        save_image(img, path)
        print(path)


if __name__ == "__main__":
    main()
