"""Generate tests/golden/g39_video_features.npz by IMPORTING the reference (authoring container only; the tests consume the committed .npz).
This script holds no reference code: it runs the reference's own

  * ``redogram`` / ``greenogram`` / ``blueogram`` (bins = 32) and ``rgb_hist`` (bins = 96), ``visual_variance`` and ``absdiff``
    (maua/audiovisual/audioreactive/selfsupervised/features/video.py:12-31, 61-75) on a 7-frame 37 x 53 clip;
  * ``pearson``, ``concordance``, ``autocorrcorr``, ``rv``, ``rv2`` and ``r1`` (.../features/correlation.py:353-382) on X, Y [50, 7] (all six)
    and on X, Z [50, 5] (the three that take unequal widths).

cv2, kornia, anatome, torchmetrics and torchsort are absent from the image: their modules are stubbed, and so are the package's
``processing`` / ``efficient_quantile`` siblings (torchaudio, a native extension); none of the captured functions calls into them.  The HSV
functions are NOT recorded: their rgb_to_hsv would be this script's own stub.

The clip is stored as bytes, uint8 HWC; the reference functions see ``clip.permute(0, 3, 1, 2).float().div(255)`` on the CPU (video.py:208).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_video_features.py
"""
import importlib
import sys
import types
from pathlib import Path
from unittest.mock import MagicMock

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
FEATURES = Path("/root/reference/maua/audiovisual/audioreactive/selfsupervised/features")
OUT = HERE / "g39_video_features.npz"
T, H, W = 7, 37, 53


def reference_modules():
    for name in ("cv2", "kornia", "kornia.color", "kornia.color.hsv", "anatome", "anatome.distance", "torchmetrics", "torchmetrics.functional",
                 "torchsort"):
        sys.modules.setdefault(name, MagicMock(name=name))
    pkg = types.ModuleType("_ref_features")
    pkg.__path__ = [str(FEATURES)]
    sys.modules["_ref_features"] = pkg
    for sibling in ("processing", "efficient_quantile"):
        sys.modules[f"_ref_features.{sibling}"] = MagicMock(name=sibling)
    return importlib.import_module("_ref_features.video"), importlib.import_module("_ref_features.correlation")


def make_clip(rng):
    """Smooth gradients plus noise (no bin empty, none equal), frame 3 constant."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    clip = np.empty((T, H, W, 3), dtype=np.uint8)
    for t in range(T):
        for c in range(3):
            phase = 0.7 * t + 1.3 * c
            ramp = 0.5 + 0.35 * np.sin(x / W * (2.0 + c) + phase) * np.cos(y / H * (1.5 + 0.5 * t) - phase)
            clip[t, :, :, c] = np.clip((ramp + 0.12 * rng.standard_normal((H, W))) * 255, 0, 255).round().astype(np.uint8)
    clip[3] = np.array([90, 160, 40], dtype=np.uint8)
    return clip


def make_matrices(rng):
    """Correlated feature matrices whose column standard deviations are well above 1e-2 of the column means."""
    base = rng.standard_normal((50, 7))
    X = (base + 0.5 + 0.1 * rng.standard_normal((50, 7))).astype(np.float32)
    Y = (0.6 * base[:, ::-1] + 0.4 * base + 1.0 + 0.5 * rng.standard_normal((50, 7))).astype(np.float32)
    Z = (0.7 * base[:, :5] - 0.3 + 0.7 * rng.standard_normal((50, 5))).astype(np.float32)
    return X, Y, Z


def main():
    torch.set_num_threads(1)
    V, CR = reference_modules()
    rng = np.random.default_rng(39)
    clip = make_clip(rng)
    video = torch.from_numpy(clip).permute(0, 3, 1, 2).float().div(255)
    out = {"clip": clip}
    with torch.inference_mode():
        for name in ("redogram", "greenogram", "blueogram"):
            out[name] = getattr(V, name)(video, 32).numpy()
        out["rgb_hist"] = V.rgb_hist(video, 96).numpy()
        out["visual_variance"] = V.visual_variance(video).numpy()
        out["absdiff"] = V.absdiff(video).numpy()
        X, Y, Z = make_matrices(rng)
        out.update(X=X, Y=Y, Z=Z)
        tx, ty, tz = torch.from_numpy(X), torch.from_numpy(Y), torch.from_numpy(Z)
        for name in ("pearson", "concordance", "autocorrcorr", "rv", "rv2", "r1"):
            out[f"{name}_XY"] = np.float32(getattr(CR, name)(tx, ty).item())
        for name in ("autocorrcorr", "rv", "rv2"):
            out[f"{name}_XZ"] = np.float32(getattr(CR, name)(tx, tz).item())
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    for k, v in out.items():
        print(f"  {k}: {np.asarray(v).shape} {np.asarray(v).dtype}")


if __name__ == "__main__":
    main()
