"""Generate tests/golden/g40_nca.npz by IMPORTING the reference's maua/nca/train.py (authoring container only; the tests consume the
committed .npz).  This script holds no reference code: it runs the reference's own ``CA.forward`` (train.py:172-185, with ``perception`` /
``perchannel_conv``, :158-169) on the CPU and records what it returns.

train.py is a script: it reads ``sys.argv[1:3]``, selects the CUDA default tensor type and downloads VGG-16 at import.  So torchvision, tqdm,
maua_utils and moviepy's writer are stubbed (matplotlib too where it is absent), ``torch.set_default_tensor_type`` is a no-op for the duration
of the import and ``sys.argv`` carries two dummy arguments.  ``torch.rand`` is replaced, while a trajectory runs, by a function that hands
out this script's recorded uniforms in call order, so that the update masks are data of the fixture.

Recorded (all float32):
  a_*   [2,12,5,7]:   x0, uniforms [5,2,5,7], the states after steps 1 .. 5 at update_rate 0.5
  b_*   [1,12,20,36]: the same, keeping the states after steps 1 and 5
  m_*   one step of a_x0 under a per-pixel rate map [5,7] (the reference's ``ca(x, p)``, generate.py:57)
  g_*   one round of generate.py:31-34's checkpoint grid at a small size: two models on two 5-column strips of a [1,12,6,12] grid, each on a
        view 2 columns wider than its strip whose interior it replaces; the second sees the first one's fresh column.
  v_*   train.py:221-229 through three steps of the a_ rule on [2,12,16,16] (nca_ref.style_case): the reference's calc_styles / style_loss on
        the RGB slice, with the module global vgg16 replaced by nca_ref.style_net's 64-64-pool-128 stand-in (a seed, not values), against
        nca_ref.style_targets; the loss, rows of the two batch-mean Grams, torch.autograd's dL/dx_3 (its three RGB channels, v_g_img; the rest is zero), dL/dx_0 and parameter gradients
The reference's zero-initialised w2 makes every step the identity, so the parameters are tests/nca_ref.py params_from_seed's (w2 drawn
N(0, 0.1^2)); the fixture stores their seeds (a_seed, b_seed).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_nca.py
"""
import importlib.util
import sys
from pathlib import Path
from unittest.mock import MagicMock, patch

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = Path(__file__).resolve().parent
TRAIN = Path("/root/reference/maua/nca/train.py")
OUT = HERE / "g40_nca.npz"


def reference_module():
    for name in ("torchvision", "torchvision.models", "tqdm", "maua_utils", "moviepy", "moviepy.video", "moviepy.video.io",
                 "moviepy.video.io.ffmpeg_writer"):
        sys.modules[name] = MagicMock(name=name)
    try:
        import matplotlib.pylab  # noqa: F401
    except Exception:
        sys.modules["matplotlib"] = MagicMock(name="matplotlib")
        sys.modules["matplotlib.pylab"] = MagicMock(name="matplotlib.pylab")
    spec = importlib.util.spec_from_file_location("_ref_nca_train", TRAIN)
    mod = importlib.util.module_from_spec(spec)
    with patch.object(torch, "set_default_tensor_type", lambda *a, **k: None), patch.object(sys, "argv", ["train.py", "style.png", "out"]):
        spec.loader.exec_module(mod)
    return mod


class Uniforms:
    """torch.rand's stand-in: the next recorded plane, checked against the shape the reference asks for."""

    def __init__(self, planes):
        self.planes, self.i = planes, 0

    def __call__(self, *shape):
        u = self.planes[self.i]
        self.i += 1
        assert tuple(shape) == (u.shape[0], 1, u.shape[1], u.shape[2]), (shape, u.shape)
        return torch.from_numpy(u)[:, None]


def make_ca(R, seed):
    """the reference's CA holding tests/nca_ref.py params_from_seed(seed): the fixture stores the seed, not the 5 856 values"""
    sys.path.insert(0, str(HERE.parent))
    from nca_ref import params_from_seed
    w1, b1, w2 = params_from_seed(seed)
    ca = R.CA()
    with torch.no_grad():
        ca.w1.weight.copy_(torch.from_numpy(w1)[:, :, None, None])
        ca.w1.bias.copy_(torch.from_numpy(b1))
        ca.w2.weight.copy_(torch.from_numpy(w2)[:, :, None, None])
    return ca


def trajectory(ca, x0, u, rate=0.5):
    xs, x = [], torch.from_numpy(x0)
    with torch.no_grad(), patch.object(torch, "rand", Uniforms(list(u))):
        for _ in range(len(u)):
            x = ca(x, rate)
            xs.append(x.numpy().copy())
    return np.stack(xs)


def nca_ref_half(a):
    sys.path.insert(0, str(HERE.parent))
    from nca_ref import _half
    return _half(a)


def main():
    torch.set_num_threads(1)
    R = reference_module()
    rng = np.random.default_rng(40)
    out = {}

    ca = make_ca(R, 40)
    out["a_seed"] = np.int64(40)
    x0 = rng.standard_normal((2, 12, 5, 7)).astype(np.float32)
    u = rng.random((5, 2, 5, 7), dtype=np.float32)
    out.update(a_x0=x0, a_u=u, a_traj=trajectory(ca, x0, u))

    cb = make_ca(R, 41)
    out["b_seed"] = np.int64(41)
    xb = nca_ref_half(rng.standard_normal((1, 12, 20, 36)))      # float16 significands: the largest input compresses
    ub = rng.random((5, 1, 20, 36), dtype=np.float32)
    tb = trajectory(cb, xb, ub)
    out.update(b_x0=xb, b_u=ub, b_x1=tb[0], b_x5=tb[4])

    rate_map = (0.05 + 0.9 * rng.random((5, 7))).astype(np.float32)
    um = rng.random((1, 2, 5, 7), dtype=np.float32)
    out.update(m_map=rate_map, m_u=um, m_x1=trajectory(ca, x0, um, torch.from_numpy(rate_map))[0])

    w, models = 5, [ca, cb]
    grid = (rng.random((1, 12, 6, w * len(models) + 2), dtype=np.float32) * np.float32(0.1)).astype(np.float32)
    ug = rng.random((len(models), 1, 6, w + 2), dtype=np.float32)
    x = torch.from_numpy(grid.copy())
    with torch.no_grad(), patch.object(torch, "rand", Uniforms(list(ug))):
        for ci, f in enumerate(models):
            view = x[:, :, :, ci * w: ci * w + w + 2]
            view[:, :, :, 1:-1] = f(view)[:, :, :, 1:-1]
    out.update(g_x0=grid, g_u=ug, g_x1=x.numpy().copy(), g_w=np.int32(w))

    # train.py:221-229 with torch.autograd: three steps of the a_ rule on [2,12,16,16], the reference's calc_styles on the RGB slice with the
    # module global vgg16 replaced by nca_ref.style_net's three convolutions, the batch-mean Grams, style_loss against seeded targets
    import nca_ref
    plan, params, pre, _ = nca_ref.style_net()
    convs = []
    for w_, b_ in params:
        c = torch.nn.Conv2d(w_.shape[1], w_.shape[0], 3, padding=1)
        with torch.no_grad():
            c.weight.copy_(torch.from_numpy(w_).float())
            c.bias.copy_(torch.from_numpy(b_).float())
        convs.append(c)
    R.vgg16 = torch.nn.Sequential(convs[0], torch.nn.ReLU(), convs[1], torch.nn.ReLU(), torch.nn.MaxPool2d(2), convs[2], torch.nn.ReLU())
    xv, uv = nca_ref.style_case()
    targets = nca_ref.style_targets()
    x = torch.from_numpy(xv.copy()).requires_grad_(True)
    with patch.object(torch, "rand", Uniforms(list(uv))):
        y = x
        for _ in range(3):
            y = ca(y)
    y.retain_grad()
    grams = R.calc_styles(R.to_rgb(y))
    loss = R.style_loss([g.mean(0) for g in grams], [torch.from_numpy(t) for t in targets])
    ca.zero_grad()
    loss.backward()
    assert not y.grad[:, 3:].any()          # the loss sees the RGB slice only: the other channels of dL/dx_3 are zero and not stored
    out.update(v_x0=xv, v_u=uv, v_g_img=y.grad.numpy()[:, :3].copy(), v_loss=np.float32(loss.item()),
               v_gram0=grams[0].mean(0).detach().numpy()[::8].copy(), v_gram1=grams[1].mean(0).detach().numpy()[::32].copy(),
               v_g_first=x.grad.numpy().copy(), v_dw1=ca.w1.weight.grad.numpy().reshape(96, 48).copy(),
               v_db1=ca.w1.bias.grad.numpy().copy(), v_dw2=ca.w2.weight.grad.numpy().reshape(12, 96).copy())
    print("loss", loss.item(), "gram magnitudes", [float(g.abs().mean()) for g in grams])

    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes)")
    for k, v in out.items():
        print(f"  {k}: {np.asarray(v).shape} {np.asarray(v).dtype}")


if __name__ == "__main__":
    main()
