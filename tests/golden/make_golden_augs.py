"""Generate tests/golden/g36_cutout_augs.npz by running the REFERENCE's own ``Cutouts.forward`` and ``DangoCutouts.forward``
(maua/ops/cutouts.py:53-206) with ``skip_augs=False`` - their default - on seeded inputs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_augs.py

Runs only in the authoring container (needs the reference tree, imported through make_golden.import_reference(); the GPU box only
consumes the .npz).  torchvision and resize_right are absent from the reference tree and from the image, so three stand-ins are set:
  * ``RC.T`` / ``RC.TF`` -> tests/torchvision_augs_ref.py (torchvision's transforms restated; they log every draw they make);
  * ``RC.resize``        -> oracle.clip.resize (resize_right restated, as g33 / g34 do);
  * the ``torch.randn_like`` the pipeline's noise Lambdas call -> a counter that returns the library's Philox noise in the documented
    layout (call j of the key's streams: stream = j, offset = row-major element index; j = 4 cutout + stage for "normal", the stage
    for "dango"), via oracle/rng.py.
What this pins is the reference's control flow around torchvision: the draw order (crop, then its augmentations; all crops, then
the batch's augmentations), which resolution each pipeline sees, which stages run, and the concatenation.  torchvision's internals
stay restated (parity unpinned).  Stored per config: inputs, the recorded draws as records, the crops, the outputs, the
noise key, and one torch.rand(4) taken after the forward (the global generator's end state)."""
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
sys.path.insert(0, str(HERE.parent))
sys.dont_write_bytecode = True

import make_golden as MG  # noqa: E402
import torchvision_augs_ref as TA  # noqa: E402


class _NoiseTorch(types.ModuleType):
    """``torch`` as the reference's cutouts module sees it: everything is torch's except randn_like, which hands out the Philox noise."""

    def __init__(self, key):
        super().__init__("torch")
        self.key, self.calls = key, 0

    def __getattr__(self, name):
        return getattr(torch, name)

    def randn_like(self, x):
        from oracle import rng as OR
        n = OR.normal(self.key, self.calls, x.numel()).reshape(tuple(x.shape))
        self.calls += 1
        return torch.from_numpy(n).to(x.dtype)


def main():
    MG.import_reference()
    import maua.ops.cutouts as RC
    from oracle import clip as OC
    out = {}
    crops = []

    class _SpyCompose(TA.Compose):
        def __call__(self, x):
            base = x._base if x._base is not None else x
            off = x.storage_offset() - base.storage_offset()
            crops.append((x.shape[-1], (off // base.shape[-1]) % base.shape[-2], off % base.shape[-1]))
            return super().__call__(x)

    seen = []

    def spy_resize(cutout, out_shape):
        base = cutout._base if cutout._base is not None else cutout
        off = cutout.storage_offset() - base.storage_offset()
        seen.append((cutout.shape[-1], (off // base.shape[-1]) % base.shape[-2], off % base.shape[-1]))
        return OC.resize(cutout, tuple(out_shape[-2:]))

    T = types.SimpleNamespace(**{k: getattr(TA, k) for k in ("Lambda", "RandomHorizontalFlip", "RandomAffine", "RandomPerspective",
                                                               "RandomGrayscale", "Grayscale", "Pad", "ColorJitter", "InterpolationMode")})
    T.Compose = _SpyCompose
    RC.T, RC.TF, RC.resize = T, types.SimpleNamespace(hflip=TA.hflip), spy_resize
    real_torch = RC.torch
    # "normal": B = 2 images share each cutout's draws; crops at their own size, the last cutn // 4 - 1 the whole padded image
    for k, (S, cs, cutn, seed, key) in enumerate(((32, 24, 8, 61, 0x0123456789ABCDEF), (40, 32, 12, 62, 0xFEDCBA9876543210))):
        img = torch.rand(2, 3, S, S, generator=torch.Generator().manual_seed(360 + k))
        RC.torch = _NoiseTorch(key)
        TA.LOG.clear()
        crops.clear()
        torch.manual_seed(seed)
        cuts = RC.Cutouts(cs, cutn)(img, None)
        end = torch.rand(4)
        assert RC.torch.calls == 4 * cutn
        out[f"normal{k}_cfg"] = np.array([S, cs, cutn, seed], dtype=np.int64)
        out[f"normal{k}_key"] = np.array(key, dtype=np.uint64)
        out[f"normal{k}_img"] = img
        out[f"normal{k}_rects"] = np.array(crops, dtype=np.int64)
        out[f"normal{k}_augs"] = TA.records_from_log(TA.LOG)
        out[f"normal{k}_out"] = cuts
        out[f"normal{k}_rand_after"] = end
    # "dango": one pipeline run on the concatenated [N, 3, cs, cs] batch, after all crops; both halves of the default schedule
    for k, (S, cs, t, seed, key) in enumerate(((40, 32, 300, 63, 0x0F1E2D3C4B5A6978), (48, 32, 700, 64, 0x8796A5B4C3D2E1F0))):
        img = torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(370 + k))
        dc = RC.DangoCutouts(cs)
        RC.torch = _NoiseTorch(key)
        TA.LOG.clear()
        seen.clear()
        torch.manual_seed(seed)
        cuts = dc(img, t)
        end = torch.rand(4)
        assert RC.torch.calls == 4
        out[f"dango{k}_cfg"] = np.array([S, cs, t, seed, dc.cut_overview[999 - t], dc.cut_innercut[999 - t]], dtype=np.int64)
        out[f"dango{k}_key"] = np.array(key, dtype=np.uint64)
        out[f"dango{k}_img"] = img
        out[f"dango{k}_sizes"] = np.array(seen, dtype=np.int64)
        out[f"dango{k}_augs"] = TA.records_from_log(TA.LOG)
        out[f"dango{k}_out"] = cuts
        out[f"dango{k}_rand_after"] = end
    RC.torch = real_torch
    MG.save("g36_cutout_augs", **out)


if __name__ == "__main__":
    with torch.no_grad():
        main()
