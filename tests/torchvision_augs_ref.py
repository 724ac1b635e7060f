"""torchvision's augmentation transforms as the "normal" / "dango" cutouts use them (maua/ops/cutouts.py:59-71, 133-146), restated on
the CPU from torchvision's published tensor path (>= 0.12) - TEST INFRASTRUCTURE.  torchvision is absent from the reference tree and
from the image, so this module stands in for ``T`` / ``TF`` when tests/golden/make_golden_augs.py runs the reference's own
``Cutouts`` / ``DangoCutouts``, and it is the CPU semantics the device kernels (csrc/cutout_augs.hip) are checked against.

Parity with torchvision itself is unpinned: what is restated is ``get_params`` of RandomHorizontalFlip / RandomAffine /
RandomPerspective / RandomGrayscale (the same torch calls with the same arguments, so the same draws from torch's global generator),
``_get_inverse_affine_matrix``, ``_get_perspective_coeffs``, ``_gen_affine_grid``, ``_perspective_grid``, ``_apply_grid_transform``
(grid_sample with the appended ones channel as the fill mask) and ``rgb_to_grayscale``.

A record (what ``maua_amd.grad.draw_augs`` returns and the library takes) is float32 [17]:
    flip, affine[6] (the inverse affine matrix, float32), persp_on, persp[8] (float32 coefficients; zero when off), grey
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

AUG_REC = 17
LOG = []   # every transform appends what it drew: ("flip", bool) / ("affine", angle, tx, ty, matrix) / ("persp", on, coeffs) / ("grey", bool)


class InterpolationMode:
    NEAREST = "nearest"
    BILINEAR = "bilinear"


# ------------------------------------------------------------------------------------------------ functional pieces
def get_inverse_affine_matrix(center, angle, translate, scale, shear):
    """torchvision.transforms.functional._get_inverse_affine_matrix (Python doubles)."""
    rot = math.radians(angle)
    sx, sy = math.radians(shear[0]), math.radians(shear[1])
    cx, cy = center
    tx, ty = translate
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    matrix = [d, -b, 0.0, -c, a, 0.0]
    matrix = [x / scale for x in matrix]
    matrix[2] += matrix[0] * (-cx - tx) + matrix[1] * (-cy - ty)
    matrix[5] += matrix[3] * (-cx - tx) + matrix[4] * (-cy - ty)
    matrix[2] += cx
    matrix[5] += cy
    return matrix


def get_perspective_coeffs(startpoints, endpoints):
    """torchvision.transforms.functional._get_perspective_coeffs: float64 least squares (gels), rounded to float32."""
    a = torch.zeros(2 * len(startpoints), 8, dtype=torch.float64)
    for i, (p1, p2) in enumerate(zip(endpoints, startpoints)):
        a[2 * i, :] = torch.tensor([p1[0], p1[1], 1, 0, 0, 0, -p2[0] * p1[0], -p2[0] * p1[1]])
        a[2 * i + 1, :] = torch.tensor([0, 0, 0, p1[0], p1[1], 1, -p2[1] * p1[0], -p2[1] * p1[1]])
    b = torch.tensor(startpoints, dtype=torch.float64).view(8)
    res = torch.linalg.lstsq(a, b, driver="gels").solution.to(torch.float32)
    return res.tolist()


def affine_grid(matrix, w, h):
    """_gen_affine_grid for the tensor path's theta = tensor(matrix, float32): pixel centres linspace(-w/2 + 0.5, w/2 - 0.5)."""
    theta = torch.tensor(matrix, dtype=torch.float32).reshape(1, 2, 3)
    d = 0.5
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(-w * 0.5 + d, w * 0.5 + d - 1, steps=w))
    base[..., 1].copy_(torch.linspace(-h * 0.5 + d, h * 0.5 + d - 1, steps=h).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled = theta.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32)
    return base.view(1, h * w, 3).bmm(rescaled).view(1, h, w, 2)


def perspective_grid(coeffs, w, h):
    """_perspective_grid: (theta1 [x, y, 1]) / (0.5 w, 0.5 h) / (theta2 [x, y, 1]) - 1, pixel centres linspace(0.5, w - 0.5)."""
    theta1 = torch.tensor([[[coeffs[0], coeffs[1], coeffs[2]], [coeffs[3], coeffs[4], coeffs[5]]]], dtype=torch.float32)
    theta2 = torch.tensor([[[coeffs[6], coeffs[7], 1.0], [coeffs[6], coeffs[7], 1.0]]], dtype=torch.float32)
    d = 0.5
    base = torch.empty(1, h, w, 3, dtype=torch.float32)
    base[..., 0].copy_(torch.linspace(d, w * 1.0 + d - 1.0, steps=w))
    base[..., 1].copy_(torch.linspace(d, h * 1.0 + d - 1.0, steps=h).unsqueeze_(-1))
    base[..., 2].fill_(1)
    rescaled1 = theta1.transpose(1, 2) / torch.tensor([0.5 * w, 0.5 * h], dtype=torch.float32)
    g1 = base.view(1, h * w, 3).bmm(rescaled1)
    g2 = base.view(1, h * w, 3).bmm(theta2.transpose(1, 2))
    return (g1 / g2 - 1.0).view(1, h, w, 2)


def apply_grid(img, grid, mode):
    """_apply_grid_transform with fill 0: a ones channel appended as the mask; nearest: mask < 0.5 -> 0; bilinear: img * m + (1 - m) * 0."""
    grid = grid.expand(img.shape[0], *grid.shape[1:])
    mask = torch.ones((img.shape[0], 1, img.shape[2], img.shape[3]), dtype=img.dtype)
    out = F.grid_sample(torch.cat((img, mask), 1), grid, mode=mode, padding_mode="zeros", align_corners=False)
    m = out[:, -1:].expand_as(out[:, :-1])
    out = out[:, :-1]
    fill = torch.zeros_like(out)
    if mode == "nearest":
        return torch.where(m < 0.5, fill, out)
    return out * m + (1.0 - m) * fill


def affine(img, matrix):
    return apply_grid(img, affine_grid(matrix, img.shape[-1], img.shape[-2]), "nearest")


def perspective(img, coeffs):
    return apply_grid(img, perspective_grid(coeffs, img.shape[-1], img.shape[-2]), "bilinear")


def hflip(img):
    return img.flip(-1)


def rgb_to_grayscale(img):
    r, g, b = img.unbind(dim=-3)
    return (0.2989 * r + 0.587 * g + 0.114 * b).unsqueeze(dim=-3).expand(img.shape)


def perspective_params(width, height, distortion_scale):
    """RandomPerspective.get_params: 8 randint draws (TL, TR, BR, BL; x before y)."""
    hh, hw = height // 2, width // 2
    ri = lambda lo, hi: int(torch.randint(lo, hi, size=(1,)).item())
    tl = [ri(0, int(distortion_scale * hw) + 1), ri(0, int(distortion_scale * hh) + 1)]
    tr = [ri(width - int(distortion_scale * hw) - 1, width), ri(0, int(distortion_scale * hh) + 1)]
    br = [ri(width - int(distortion_scale * hw) - 1, width), ri(height - int(distortion_scale * hh) - 1, height)]
    bl = [ri(0, int(distortion_scale * hw) + 1), ri(height - int(distortion_scale * hh) - 1, height)]
    start = [[0, 0], [width - 1, 0], [width - 1, height - 1], [0, height - 1]]
    return start, [tl, tr, br, bl]


# ------------------------------------------------------------------------------------------------ the transforms (T.*)
class Compose:
    def __init__(self, transforms):
        self.transforms = transforms

    def __call__(self, x):
        for t in self.transforms:
            x = t(x)
        return x


class Lambda:
    def __init__(self, fn):
        self.fn = fn

    def __call__(self, x):
        return self.fn(x)


class RandomHorizontalFlip:
    def __init__(self, p=0.5):
        self.p = p

    def __call__(self, x):
        on = bool(torch.rand(1) < self.p)
        LOG.append(("flip", on))
        return hflip(x) if on else x


class RandomAffine:
    """degrees / translate only (scale 1, shear 0): what the cutouts use; fill 0, NEAREST."""

    def __init__(self, degrees, translate=None, interpolation=InterpolationMode.NEAREST, fill=0):
        if interpolation != InterpolationMode.NEAREST:
            raise NotImplementedError("RandomAffine: only NEAREST is restated (the 'Video Input' pipeline)")
        self.degrees = [-float(degrees), float(degrees)] if isinstance(degrees, (int, float)) else [float(d) for d in degrees]
        self.translate = translate

    def __call__(self, x):
        w, h = x.shape[-1], x.shape[-2]
        angle = float(torch.empty(1).uniform_(float(self.degrees[0]), float(self.degrees[1])).item())
        max_dx, max_dy = float(self.translate[0] * w), float(self.translate[1] * h)
        tx = int(round(torch.empty(1).uniform_(-max_dx, max_dx).item()))
        ty = int(round(torch.empty(1).uniform_(-max_dy, max_dy).item()))
        matrix = get_inverse_affine_matrix([0.0, 0.0], angle, [float(tx), float(ty)], 1.0, [0.0, 0.0])
        LOG.append(("affine", angle, tx, ty, matrix))
        return affine(x, matrix)


class RandomPerspective:
    def __init__(self, distortion_scale=0.5, p=0.5, interpolation=InterpolationMode.BILINEAR, fill=0):
        self.distortion_scale, self.p = distortion_scale, p

    def __call__(self, x):
        if torch.rand(1) < self.p:
            start, end = perspective_params(x.shape[-1], x.shape[-2], self.distortion_scale)
            coeffs = get_perspective_coeffs(start, end)
            LOG.append(("persp", True, coeffs))
            return perspective(x, coeffs)
        LOG.append(("persp", False, None))
        return x


class RandomGrayscale:
    def __init__(self, p=0.1):
        self.p = p

    def __call__(self, x):
        on = bool(torch.rand(1) < self.p)
        LOG.append(("grey", on))
        return rgb_to_grayscale(x) if on else x


class Grayscale:
    def __init__(self, num_output_channels=1):
        assert num_output_channels == 3

    def __call__(self, x):
        return rgb_to_grayscale(x)


class Pad:
    def __init__(self, padding, fill=0):
        self.padding, self.fill = padding, fill

    def __call__(self, x):
        return F.pad(x, (self.padding,) * 4, value=float(self.fill))


class ColorJitter:
    def __init__(self, *a, **k):
        raise NotImplementedError("ColorJitter is not restated")


# ------------------------------------------------------------------------------------------------ records
def records_from_log(log):
    """LOG entries (flip, affine, persp, grey per pipeline run) -> float32 [n, 17] records."""
    recs = []
    for i in range(0, len(log), 4):
        (kf, flip), (ka, _, _, _, matrix), (kp, on, coeffs), (kg, grey) = log[i:i + 4]
        assert (kf, ka, kp, kg) == ("flip", "affine", "persp", "grey")
        r = np.zeros(AUG_REC, dtype=np.float32)
        r[0] = flip
        r[1:7] = np.asarray(matrix, dtype=np.float32)
        r[7] = on
        if on:
            r[8:16] = np.asarray(coeffs, dtype=np.float32)
        r[16] = grey
        recs.append(r)
    return np.stack(recs) if recs else np.zeros((0, AUG_REC), np.float32)


def augment(x, rec, noises=None):
    """The 'Video Input' pipeline on x [N, 3, s, s] with the draws of one record (float32 [17]) and the four noise tensors (each like
    x, already scaled by 0.01; None: no noise).  Differentiable (torch.autograd): the CPU adjoint the device's is checked against."""
    rec = np.asarray(rec, dtype=np.float32)
    nz = noises if noises is not None else [None] * 4
    add = lambda v, k: v if nz[k] is None else v + nz[k]
    if rec[0]:
        x = hflip(x)
    x = add(x, 0)
    x = affine(x, [float(v) for v in rec[1:7]])
    x = add(x, 1)
    if rec[7]:
        x = perspective(x, [float(v) for v in rec[8:16]])
    x = add(x, 2)
    if rec[16]:
        x = rgb_to_grayscale(x)
    return add(x, 3)


def philox_noise(key, j, shape):
    """The library's noise of pipeline run j (streams 4 j + stage, offset = row-major element index), already x 0.01: four tensors."""
    from oracle import rng as OR
    n = int(np.prod(shape))
    return [torch.from_numpy(OR.normal(key, 4 * j + s, n).reshape(shape)) * 0.01 for s in range(4)]
