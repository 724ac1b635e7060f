"""The NCA training loss and loop on the device: maua_vgg_gram_mean_grad (csrc/perceptor.hip) and maua_amd.nca.train_step / train, against
the float64 restatement tests/nca_ref.py and the reference's recorded calc_styles / style_loss / autograd run (tests/golden/g40_nca.npz).

The network is the fixture's 64-64-pool-128 stand-in with two taps (nca_ref.style_net; weights representable in bf16, so one set serves
both network modes).  As in tests/test_gpu_perceptor.py every stage is compared on the device's own stored inputs (ReLU's mask and the
pool's argmax are functions of the stored activations, so no tie allowance is needed), inside element-wise bounds read from the kernels:
perceptor_ref's per-layer bounds and nca_ref.gram_mean_bounds for the head.

Against the fixture the comparison is in the f32 network mode: the reference's float32 image differs from the device's by the steps'
rounding, which the restatement evaluated on float32 steps measures.  In the bf16 mode the stored activations are rounded to bf16; how
that moves the end result through ReLU masks is not something perceptor_ref bounds, so bf16 is pinned stage by stage only."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import nca_ref as R  # noqa: E402
import perceptor_ref as P  # noqa: E402
from test_gpu_nca import make_ca  # noqa: E402
from test_gpu_perceptor import Buf, Net, _sync, ratio  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "g40_nca.npz"
TORCH_DT = {"f32": torch.float32, "bf16": torch.bfloat16}


@pytest.fixture(scope="module")
def g40():
    return R.load_g40(GOLDEN)


@pytest.fixture(scope="module")
def case(g40):
    """the fixture's image in float64 and as float32 steps would give it, the targets, the restatement's results on both"""
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    net, targets = R.style_net(), [t.astype(np.float64) for t in R.style_targets()]
    img = R.steps(g40["v_x0"], *prm, g40["v_u"])[:, :3].astype(np.float32).astype(np.float64)
    img32 = R.steps(g40["v_x0"], *prm, g40["v_u"], dtype=np.float32)[:, :3].astype(np.float64)
    return dict(prm=prm, net=net, targets=targets, img=img, at=R.gram_mean_grad(net, img, targets), at32=R.gram_mean_grad(net, img32, targets))


def device_gram_mean(net, img, taps, targets):
    net.B, _, net.H, net.W = img.shape
    net.img = Buf(img)
    tb = [Buf(t) for t in targets]
    grad, loss = Buf(n=img.size), Buf(n=1)
    n = len(taps)
    L.check(L.lib().maua_vgg_gram_mean_grad(net.h, net.img.ptr, net.B, net.H, net.W, (C.c_int * n)(*taps), n,
                                            (C.c_void_p * n)(*[t.ptr.value for t in tb]), grad.ptr, loss.ptr))
    _sync()
    return grad.get("grad").reshape(img.shape), float(loss.get("loss")[0])


def check_head(ref_net, img, targets, dt):
    net = Net(ref_net, dt)
    grad, loss = device_gram_mean(net, img, list(R.STYLE_TAPS), targets)
    acts = net.acts()
    net.close()
    want_loss, eloss, want, bound = R.gram_mean_grad_bound(ref_net, acts, targets, dt)
    r_loss, r = abs(loss - want_loss) / eloss, ratio(grad, want, bound)
    print(f"gram_mean_grad {dt} {img.shape}: loss error / bound {r_loss:.3g}, gradient error / bound {r:.3g}")
    assert r_loss <= 1, (loss, want_loss, eloss)
    assert r <= 1
    assert np.abs(want).max() > 0
    return grad, loss, want, want_loss, bound, eloss


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("shape", [(16, 16), (32, 16)])
def test_gram_mean_grad_against_restatement_and_recorded(shape, dt, g40, case):
    if shape == (16, 16):
        img = case["img"]
    else:
        img = R.style_image(9, 2, *shape)
    grad, loss, want, want_loss, bound, eloss = check_head(case["net"], img, case["targets"], dt)
    if shape == (16, 16) and dt == "f32":
        (l64, g64), (l32, g32) = case["at"], case["at32"]
        moved_l, moved_g = 2 * abs(l32 - l64), 2 * np.abs(g32 - g64)
        r_loss = abs(loss - float(g40["v_loss"])) / (2 * eloss + moved_l + 2.0 ** -24 * l64)
        r = ratio(grad, g40["v_g_last"][:, :3].astype(np.float64), 2 * bound + moved_g)
        print(f"against the recorded run: loss {r_loss:.3g}, gradient {r:.3g}")
        assert r_loss <= 1 and r <= 1


def test_gram_mean_grad_twice_identical_bits_and_one_image(case):
    net = Net(case["net"], "f32")
    a = device_gram_mean(net, case["img"], list(R.STYLE_TAPS), case["targets"])
    b = device_gram_mean(net, case["img"], list(R.STYLE_TAPS), case["targets"])
    assert np.array_equal(a[0], b[0]) and a[1] == b[1]
    one = device_gram_mean(net, case["img"][:1], list(R.STYLE_TAPS), case["targets"])       # B = 1: the mean is the image's own Gram
    acts = net.acts()
    want_loss, eloss, want, bound = R.gram_mean_grad_bound(case["net"], acts, case["targets"], "f32")
    assert abs(one[1] - want_loss) <= eloss and ratio(one[0], want, bound) <= 1
    rc = L.lib().maua_vgg_gram_mean_grad(net.h, net.img.ptr, 0, 16, 16, (C.c_int * 1)(0), 1, (C.c_void_p * 1)(net.img.ptr.value), net.img.ptr, None)
    assert rc != 0 and "at least 1" in L.lib().maua_last_error().decode()
    net.close()


def stand_in_style(dt="f32"):
    """maua_amd.nca.StyleLoss on the stand-in network: torchvision-style keys of a [conv, ReLU, conv, ReLU, pool, conv, ReLU] features"""
    from maua_amd import nca, perceptors
    net = perceptors.VGGFeatures((64, 64, "M", 128), 6, (1.0, 0.0, perceptors.IMAGENET_MEAN, perceptors.IMAGENET_STD), dtype=TORCH_DT[dt])
    assert net.plan == list(R.STYLE_PLAN)
    sd = {}
    for key, (w, b) in zip(("0", "2", "5"), R.style_net()[1]):
        sd[f"{key}.weight"], sd[f"{key}.bias"] = torch.from_numpy(w).float(), torch.from_numpy(b).float()
    net.load_state_dict(sd)
    return nca.StyleLoss(net, layers=(1, 6))


def test_one_training_iteration_against_restatement(g40, case):
    """pool-free core of an iteration (train_step) at batch 2, 16 x 16, 4 steps, Philox masks of seed 11: every stage on the device's stored
    inputs - the states, the loss and dL/d image on the stored activations, the parameter gradients through the stored states with the
    image gradient's bound carried in, then float64 normalisation and Adam's first step with the gradients' bound carried through."""
    from maua_amd import nca
    prm = case["prm"]
    ca = make_ca(*prm, "f32", seed=11)
    style = stand_in_style()
    opt = torch.optim.Adam(ca.parameters(), 1e-3)
    x0 = g40["v_x0"]
    trace = {}
    xn, loss = nca.train_step(ca, torch.from_numpy(x0).cuda(), 4, style, opt, targets=[torch.from_numpy(t).cuda() for t in R.style_targets()],
                              trace=trace)
    assert ca.steps_done == 4 and trace["step0"] == 0
    u = np.stack([R.philox_u(11, 0, t, 2, 16, 16) for t in range(4)])
    states = trace["states"].cpu().numpy()
    assert np.array_equal(states[0], x0) and torch.equal(xn, trace["states"][-1])
    want_x, bx = R.steps_bound(x0, *prm, u)
    assert ratio(states[-1], want_x, bx) <= 1
    acts = [style.net.features(i).cpu().double().numpy() for i in style.net.index]
    want_loss, eloss, dimg, bimg = R.gram_mean_grad_bound(case["net"], acts, case["targets"], "f32")
    assert abs(float(loss) - want_loss) <= eloss
    g_last = trace["g_last"].cpu().numpy()
    assert not g_last[:, 3:].any() and ratio(g_last[:, :3], dimg, bimg) <= 1
    gl, ge = np.zeros_like(want_x), np.zeros_like(want_x)
    gl[:, :3], ge[:, :3] = dimg, bimg
    want, bound = R.vjp(states, *prm, u, gl, bound=True, g_err=ge)
    p0 = dict(zip(("dw1", "db1", "dw2"), prm))
    new = {"dw1": ca.w1.weight, "db1": ca.w1.bias, "dw2": ca.w2.weight}
    for name, w, b in zip(("g_first", "dw1", "db1", "dw2"), want, bound):
        r = ratio(trace[name].cpu().numpy().reshape(w.shape), w, b)
        print(f"train_step {name}: error / bound {r:.3g}")
        assert r <= 1, name
        if name == "g_first":
            continue
        ghat, eg = R.normalise(w), R.normalise_bound(w, b)
        p = p0[name].astype(np.float64)
        ref = R.adam_first_step(p, ghat)
        r = ratio(new[name].detach().cpu().numpy().reshape(p.shape), ref, R.adam_first_step_bound(p, ghat, eg))
        print(f"updated {name}: error / bound {r:.3g}, moved by {np.abs(ref - p).max():.3g}")
        assert r <= 1 and np.abs(ref - p).max() > 5e-4, name


def test_train_lowers_the_loss_and_writes_its_files(tmp_path):
    """train() end to end on the stand-in network: pool 8, batch 2, 16 x 16, 20 iterations of 8 steps; a sanity check, not a number.
    The learning rate is 1e-4: with normalised gradients Adam moves every weight by about lr per iteration whatever the loss, and on this
    random stand-in network a step's gain passes 1 once |w2| reaches about 0.01 - at the reference's 1e-3 the float64 restatement of this
    very run (same pool draws and masks) reaches a loss of 1e16 by iteration 19 as well, and 5.2 from 7.8 at 1e-4."""
    import PIL.Image
    from maua_amd import nca
    rng = np.random.default_rng(6)
    PIL.Image.fromarray(rng.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(tmp_path / "tex.png")
    ca, losses = nca.train(tmp_path / "tex.png", tmp_path / "out", steps=20, pool_size=8, batch=2, size=16, step_range=(8, 9), save_every=10,
                           seed=3, style=stand_in_style(), lr=1e-4)
    assert len(losses) == 20 and all(np.isfinite(losses))
    print(f"loss: first {losses[0]:.6g}, after 20 iterations {losses[-1]:.6g}")
    assert losses[-1] < losses[0]
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["tex_10.png", "tex_10.pt", "tex_20.png", "tex_20.pt"]
    assert PIL.Image.open(tmp_path / "out" / "tex_20.png").size == (32, 16)
    back = nca.load_ca(tmp_path / "out" / "tex_20.pt")
    assert torch.equal(back.w2.weight, ca.w2.weight.cpu()) and bool(ca.w2.weight.any())
    assert ca.steps_done == 20 * 8
