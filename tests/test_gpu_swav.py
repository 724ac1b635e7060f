"""The SwAV ResNet extractor on the device (maua_amd/resnet.py, csrc/resnet.hip) against the float64 restatement (tests/swav_ref.py).

Bounds, set before anything ran on a device:
  * float32: the error of a tap, divided by the tap's largest value, is at most 4 x the error of the reference network's OWN float32
    forward against its float64 forward (recorded per tap in tests/golden/g42_swav.npz; for the ResNet-50 case, where there is no
    fixture, the restatement's float32 evaluation of the same operations, computed here).  The device evaluates the same float32
    arithmetic in another order and with BatchNorm folded; a dropped tap, a shifted border or a missing ReLU miss by orders of magnitude.
  * bfloat16: within 2 x the error of the bf16-emulating restatement (folded weights and every stored activation rounded to bfloat16,
    sums in float64) against the float64 one, computed here: two valid bf16 evaluations may each be that far from the truth.
Measured ratios (error / bound, one MI355X) are printed by the tests and recorded in DESIGN.md section 5k.
"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import swav_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden" / "g42_swav.npz"
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
STAGES = ("stem", "pool", "layer1", "layer2", "layer3", "layer4")
R50 = (3, 4, 6, 3)


@pytest.fixture(scope="module")
def R():
    from maua_amd import resnet
    return resnet


@pytest.fixture(scope="module")
def small():
    """the fixture network and input; the float64 taps and the bf16 emulation's error per tap and for the features"""
    z = np.load(GOLDEN)
    layers = tuple(int(n) for n in z["layers"])
    sd, x = SR.make_state_dict(int(z["seed"]), layers), torch.from_numpy(z["x"])
    taps, feats = SR.forward(sd, x, layers)
    btaps, bfeats = SR.forward(sd, x, layers, bf16=True)
    assert float((feats - torch.from_numpy(z["feat_f64"])).abs().max()) <= 1e-12 * float(feats.abs().max())
    return {"layers": layers, "sd": sd, "x": x, "taps": taps, "feats": feats, "tap_max": z["tap_max"], "tap_err": z["tap_err"],
            "feat_err": float(z["feat_err"]), "bf16_tap_err": [float((a - b).abs().max()) for a, b in zip(taps, btaps)],
            "bf16_feat_err": float((feats - bfeats).abs().max())}


@pytest.fixture(scope="module")
def r50():
    """ResNet-50 at 2 x 3 x 64 x 64 and 1 x 3 x 40 x 56: float64 features, and the float32 / bf16 evaluations' errors"""
    sd = SR.make_state_dict(9, R50)
    out = {"sd": sd, "cases": []}
    for seed, shape in ((3, (2, 3, 64, 64)), (4, (1, 3, 40, 56))):
        x = SR.make_input(seed, shape)
        f64 = SR.forward(sd, x, R50)[1]
        f32 = SR.forward(sd, x, R50, dtype=torch.float32)[1]
        b16 = SR.forward(sd, x, R50, bf16=True)[1]
        out["cases"].append({"x": x, "f64": f64, "f32_err": float((f32.double() - f64).abs().max()), "bf16_err": float((b16 - f64).abs().max())})
    return out


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_every_tap_of_the_fixture_network(R, small, dt):
    net = R.ResNetFeatures(small["layers"], 64, DTYPES[dt], small["sd"])
    feats = net(small["x"])
    assert feats.dtype == torch.float32 and feats.is_cuda and tuple(feats.shape) == (2, 2048)
    for stage, name in enumerate(STAGES):
        got, want = net.tap(stage).cpu().double(), small["taps"][stage]
        assert got.shape == want.shape, name
        err = float((got - want).abs().max())
        bound = 4 * small["tap_err"][stage] if dt == "f32" else 2 * small["bf16_tap_err"][stage]
        print(f"{dt} {name}: error {err:.3g} ({err / small['tap_max'][stage]:.3g} of max), bound {bound:.3g}, ratio {err / bound:.3f}")
        assert err / small["tap_max"][stage] <= bound / small["tap_max"][stage], (dt, name, err, bound)
    err = float((feats.cpu().double() - small["feats"]).abs().max())
    bound = 4 * small["feat_err"] if dt == "f32" else 2 * small["bf16_feat_err"]
    print(f"{dt} features: error {err:.3g}, bound {bound:.3g}, ratio {err / bound:.3f}")
    assert err <= bound


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_resnet50_features_repeat_and_recarve(R, r50, dt):
    net = R.ResNetFeatures(R50, 64, DTYPES[dt], r50["sd"])
    first = None
    for case in (r50["cases"][0], r50["cases"][1], r50["cases"][0]):      # (B, H, W) changes between calls: the workspace is laid out again
        got = net(case["x"])
        again = net(case["x"])
        assert torch.equal(got, again)
        err = float((got.cpu().double() - case["f64"]).abs().max())
        bound = 4 * case["f32_err"] if dt == "f32" else 2 * case["bf16_err"]
        print(f"{dt} resnet50 {tuple(case['x'].shape)}: error {err:.3g} of max {float(case['f64'].abs().max()):.3g}, bound {bound:.3g}, "
              f"ratio {err / bound:.3f}")
        assert err <= bound, (dt, tuple(case["x"].shape), err, bound)
        if first is None:
            first = got.clone()
    assert torch.equal(first, got)      # the first shape again, after the other one: the same bits
    assert tuple(net.tap(5).shape) == (2, 2048, 2, 2)
    crops = [case["x"] for case in (r50["cases"][0], r50["cases"][0], r50["cases"][1])]      # a list: grouped by consecutive equal width
    both = net(crops)
    assert tuple(both.shape) == (5, 2048) and torch.equal(both[:2], first) and torch.equal(both[2:4], first)


def test_compute_with_the_swav_extractor():
    from maua_amd import metrics as M
    g = torch.Generator().manual_seed(12)
    real = [torch.rand((8, 3, 32, 32), generator=g) for _ in range(2)]
    fakes = [torch.rand((8, 3, 32, 32), generator=g) * 2 - 1 for _ in range(2)]
    todo = list(fakes)
    torch.manual_seed(21)
    np.random.seed(5)
    res, rf, ff = M.compute(real, lambda: todo.pop(0), n_samples=16, extractor="SwAV:random", batch_size=8, verbose=False,
                            return_features=True, allow_random_init=True)
    assert sorted(res) == sorted(["Frechet SwAV Distance", "Kernel SwAV Distance", "Precision (SwAV)", "Recall (SwAV)", "Density (SwAV)",
                                  "Coverage (SwAV)"])
    assert all(np.isfinite(v) for v in res.values()) and tuple(rf.shape) == tuple(ff.shape) == (16, 2048)
    # the same features by hand: the extractor on each batch in [0, 1], resized as compute resizes them
    torch.manual_seed(21)
    ex, size, name = M.get_extractor("SwAV:random", allow_random_init=True)
    assert (size, name) == (224, "SwAV")
    from maua_amd.image import resize
    hand_r, hand_f = [], []
    for rb, fb in zip(real, fakes):
        fb = resize(fb.float().add(1).div(2), out_shape=(224, 224)).to("cuda")      # GeneratorImages, then compute's .to(device)
        rb = resize(rb.to("cuda").float(), out_shape=(224, 224))
        feats = ex(torch.cat((rb, fb)))
        hand_r.append(feats[:8])
        hand_f.append(feats[8:])
    hand_r, hand_f = torch.cat(hand_r), torch.cat(hand_f)
    assert torch.equal(hand_r, rf) and torch.equal(hand_f, ff)
    assert res["Frechet SwAV Distance"] == M.frechet_distance(hand_r, hand_f)
    assert (res["Precision (SwAV)"], res["Recall (SwAV)"], res["Density (SwAV)"], res["Coverage (SwAV)"]) == M.prdc(hand_r, hand_f)
    np.random.seed(5)      # kernel_distance draws its subsets with np.random.choice, and nothing else in compute draws from it
    assert res["Kernel SwAV Distance"] == M.kernel_distance(hand_r, hand_f)
