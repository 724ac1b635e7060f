"""CPU restatements of the third-party pieces the reference's image pipeline calls and that are absent from the reference tree and the
image (parity unpinned): torchvision's ``adjust_sharpness`` / ``to_pil_image`` / ``to_tensor`` and ``resize_right.resize`` with
the cubic and lanczos3 kernels.  Used by tests/golden/make_golden_image_pipeline.py (standing in for the absent packages while the
reference's own functions run) and by the tests (as the reference of the HIP operators).  PIL itself is present and is used as it is."""
import math

import numpy as np
import torch


# ---------------------------------------------------------------------------------------------- resize_right (published algorithm)
def cubic(x):
    a = x.abs()
    a2, a3 = a ** 2, a ** 3
    return ((1.5 * a3 - 2.5 * a2 + 1.0) * (a <= 1.0).to(x.dtype)
            + (-0.5 * a3 + 2.5 * a2 - 4.0 * a + 2.0) * ((1.0 < a) & (a <= 2.0)).to(x.dtype))


cubic.support_sz = 4.0


def lanczos3(x):
    eps = torch.finfo(torch.float32).eps
    return ((torch.sin(math.pi * x) * torch.sin(math.pi * x / 3) + eps) / ((math.pi ** 2 * x ** 2 / 3) + eps)) * (x.abs() < 3).to(x.dtype)


lanczos3.support_sz = 6.0


def resize_tables(in_sz, out_sz, interp_method=cubic):
    """field of view and weights of one dimension (resize_right.py: get_projected_grid, get_field_of_view, get_weights)."""
    eps = torch.finfo(torch.float32).eps
    scale = out_sz / in_sz
    projected = torch.arange(out_sz) / float(scale) + (in_sz - 1) / 2 - (out_sz - 1) / (2 * float(scale))
    support = interp_method.support_sz
    method = interp_method
    if scale < 1.0:                                    # antialiasing
        method = lambda a: scale * interp_method(scale * a)
        support = support / scale
    left = torch.ceil(projected - support / 2 - eps).long()
    fov = left[:, None] + torch.arange(math.ceil(support - eps))
    w = method(projected[:, None] - fov)
    s = w.sum(1, keepdim=True)
    s[s == 0] = 1
    return left, w / s


def resize(x, out_shape=None, interp_method=cubic, **_kw):
    """``resize_right.resize(x, out_shape=..., interp_method=...)``: a short out_shape applies to the last dimensions; dimensions are
    processed in order of ascending scale factor (ties keep their order); zero padding; unchanged dimensions are skipped."""
    out_shape = list(x.shape[:x.dim() - len(out_shape)]) + list(out_shape)
    dims = [(d, out_shape[d] / x.shape[d]) for d in range(x.dim()) if out_shape[d] != x.shape[d]]
    for dim, _s in sorted(dims, key=lambda ds: ds[1]):
        in_sz, out_sz = x.shape[dim], out_shape[dim]
        left, w = resize_tables(in_sz, out_sz, interp_method)
        idx = left[:, None] + torch.arange(w.shape[1])
        ok = ((idx >= 0) & (idx < in_sz)).to(x.dtype)
        nb = x.movedim(dim, -1)[..., idx.clamp(0, in_sz - 1)]
        x = (nb * (w.to(x.dtype) * ok)).sum(-1).movedim(-1, dim)
    return x


# ---------------------------------------------------------------------------------------------- torchvision.transforms.functional
def to_tensor(pic):
    """PIL image / ndarray [H, W, C] -> float CHW; bytes / 255."""
    arr = np.asarray(pic)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))
    return t.float().div(255) if arr.dtype == np.uint8 else t.float()


def to_pil_image(pic):
    """float tensor [C, H, W] / [H, W] -> PIL image: ``pic.mul(255).byte()``, mode L or RGB."""
    from PIL import Image
    if pic.dim() == 2:
        pic = pic.unsqueeze(0)
    u8 = pic.mul(255).byte().permute(1, 2, 0).numpy()
    return Image.fromarray(u8[:, :, 0], mode="L") if u8.shape[2] == 1 else Image.fromarray(u8, mode="RGB")


def adjust_sharpness(img, sharpness_factor):
    """tensor path: 3x3 blur [[1,1,1],[1,5,1],[1,1,1]] / 13 on the interior, border kept; ratio * img + (1 - ratio) * blurred, clamp 0..1."""
    if img.shape[-1] <= 2 or img.shape[-2] <= 2:
        return img
    k = torch.ones((3, 3), dtype=img.dtype)
    k[1, 1] = 5.0
    k /= k.sum()
    c = img.shape[-3]
    flat = img.reshape(-1, c, img.shape[-2], img.shape[-1])
    blur = torch.nn.functional.conv2d(flat, k.expand(c, 1, 3, 3), groups=c)
    deg = flat.clone()
    deg[..., 1:-1, 1:-1] = blur
    return (sharpness_factor * flat + (1.0 - sharpness_factor) * deg).clamp(0, 1).reshape(img.shape)


def sharpen(img, strength):
    """maua/ops/image.py:70-71 on the restated adjust_sharpness."""
    return adjust_sharpness(img.add(1).div(2), strength).mul(2).sub(1)


def perlin_image(raw, grayscale):
    """maua/ops/noise.py:126-132 after perlin_ms: clamp, to_pil_image, (convert RGB), PIL's autocontrast, to_tensor -> [3, H, W]."""
    from PIL import ImageOps
    if grayscale:
        out = to_pil_image(raw.clamp(0, 1)).convert("RGB")
    else:
        out = raw.reshape(-1, 3, raw.shape[0] // 3, raw.shape[1])
        out = to_pil_image(out.clamp(0, 1).squeeze())
    return to_tensor(ImageOps.autocontrast(out))
