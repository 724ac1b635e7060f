"""Generate tests/golden/g42_swav.npz by IMPORTING the reference's maua/GAN/metrics/extractors/swav.py by file path (authoring container
only; the tests consume the committed .npz).  This script holds no reference code: it builds the reference's own
``ResNet(Bottleneck, [1, 2, 1, 1])`` on the CPU - one block with a downsample branch and one identity block - loads
tests/swav_ref.py's ``make_state_dict(7, ...)`` into it and records what ``forward_backbone`` / ``forward_head`` return for a
2 x 3 x 40 x 56 input (stages 20x28, 10x14, 10x14, 5x7, 3x4, 2x2: odd sizes meet both stride-2 forms).  The reference's ``forward``
calls ``.cuda()`` and is not used.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_swav.py <reference checkout>

Recorded:
  x                    the input, float32 [2, 3, 40, 56] in [0, 1]
  feat_f64, feat_f32   the features of the ``.double()`` network on x.double(), and of the float32 network
  tap_max, tap_err     per tap (stem, pool, layer1 .. layer4; forward hooks on relu / maxpool / layerN) the largest absolute value of the
                       float64 tap, and the largest |float32 tap - float64 tap|: the reference's own float32 error
  feat_err             the same for the features
  sum_keys, sums       a float64 checksum (swav_ref.checksums) of every generated weight tensor; the weights themselves are not stored
  layers, seed
"""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import swav_ref as SR  # noqa: E402

OUT = HERE / "g42_swav.npz"
LAYERS, SEED, X_SEED, SHAPE = (1, 2, 1, 1), 7, 11, (2, 3, 40, 56)


def load(root):
    spec = importlib.util.spec_from_file_location("_ref_swav", root / "maua" / "GAN" / "metrics" / "extractors" / "swav.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(net, x):
    taps = []
    hooks = [net.maxpool.register_forward_pre_hook(lambda m, a: taps.append(a[0].detach().clone())),      # the stem after its ReLU
             net.maxpool.register_forward_hook(lambda m, a, o: taps.append(o.detach().clone()))]
    hooks += [getattr(net, f"layer{i}").register_forward_hook(lambda m, a, o: taps.append(o.detach().clone())) for i in (1, 2, 3, 4)]
    with torch.no_grad():
        feats = net.forward_head(net.forward_backbone(x))
    for h in hooks:
        h.remove()
    return taps, feats


def main():
    ref = load(Path(sys.argv[1]))
    torch.set_num_threads(1)
    sd = SR.make_state_dict(SEED, LAYERS)
    x = SR.make_input(X_SEED, SHAPE)
    net = ref.ResNet(ref.Bottleneck, list(LAYERS)).eval()
    missing = net.load_state_dict(sd, strict=False)
    assert not missing.unexpected_keys and all(k.endswith("num_batches_tracked") for k in missing.missing_keys), missing
    t32, f32 = run(net, x)
    t64, f64 = run(net.double(), x.double())
    assert [tuple(t.shape[2:]) for t in t64] == [(20, 28), (10, 14), (10, 14), (5, 7), (3, 4), (2, 2)], [t.shape for t in t64]
    twin_taps, twin_feats = SR.forward(sd, x, LAYERS)
    assert (twin_feats - f64).abs().max() <= 1e-12 * f64.abs().max()
    sums = SR.checksums(sd)
    rec = {"x": x.numpy(), "feat_f64": f64.numpy(), "feat_f32": f32.numpy(),
           "tap_max": np.array([float(t.abs().max()) for t in t64]),
           "tap_err": np.array([float((a.double() - b).abs().max()) for a, b in zip(t32, t64)]),
           "feat_err": np.float64((f32.double() - f64).abs().max()),
           "sum_keys": np.array(sorted(sums)), "sums": np.array([sums[k] for k in sorted(sums)], dtype=np.float64),
           "layers": np.array(LAYERS, dtype=np.int64), "seed": np.int64(SEED)}
    for name, m, e in zip(("stem", "pool", "layer1", "layer2", "layer3", "layer4"), rec["tap_max"], rec["tap_err"]):
        print(f"{name}: max {m:.4g}, float32 error {e:.3g} ({e / m:.3g} of max)")
    print("features: max", float(f64.abs().max()), "float32 error", float(rec["feat_err"]))
    np.savez_compressed(OUT, **rec)
    print(OUT, OUT.stat().st_size, "bytes")


if __name__ == "__main__":
    main()
