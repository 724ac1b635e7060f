"""What tests/test_gpu_nca.py rests on, proved on the CPU: tests/nca_ref.py against the reference's own recorded results
(tests/golden/g40_nca.npz, made by importing maua/nca/train.py), the in-kernel mask's host twin, the exactness of the exact family, a set of
deliberate mistakes that each must change a compared result, and the host logic of maua_amd/nca.py."""
import pickle
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import nca_ref as R  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "g40_nca.npz"


@pytest.fixture(scope="module")
def g40():
    return R.load_g40(GOLDEN)


def _within(name, got32, want64, bound):
    """the reference's float32 result inside the float32 bound around the float64 restatement; prints the worst ratio"""
    err = np.abs(got32.astype(np.float64) - want64)
    ratio = float((err / bound).max())
    print(f"{name}: max |ref32 - f64| {err.max():.3e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, name
    return ratio


def test_restatement_matches_recorded_trajectories(g40):
    a = [g40[f"a_{k}"] for k in ("x0", "w1", "b1", "w2", "u")]
    for n in range(1, 6):
        want, bound = R.steps_bound(*a[:4], a[4][:n])
        _within(f"5x7 step {n}", g40["a_traj"][n - 1], want, bound)
    # on the single 5 x 7 step the reference was observed 2.3e-6 off float64 at |y| ~ 1.6: the bound must hold that with room
    want, bound = R.steps_bound(*a[:4], a[4][:1])
    assert float(bound.max()) > 2.3e-6
    b = [g40[f"b_{k}"] for k in ("x0", "w1", "b1", "w2", "u")]
    for n, key in ((1, "b_x1"), (5, "b_x5")):
        want, bound = R.steps_bound(*b[:4], b[4][:n])
        _within(f"20x36 step {n}", g40[key], want, bound)


def test_restatement_matches_recorded_rate_map_step(g40):
    want, bound = R.step(g40["a_x0"], g40["a_w1"], g40["a_b1"], g40["a_w2"], g40["m_u"][0], g40["m_map"], bound=0.0)
    _within("rate map", g40["m_x1"], want, bound)
    assert not np.array_equal(R.mask_of(g40["m_u"][0], g40["m_map"]), R.mask_of(g40["m_u"][0], 0.5))


def test_restatement_matches_recorded_checkpoint_grid(g40):
    got = R.checkgrid_round(g40)
    # two dependent single steps: the second one's input carries the first one's float32 error only in one column; charge both steps everywhere
    _, b0 = R.step(g40["g_x0"], g40["a_w1"], g40["a_b1"], g40["a_w2"], np.zeros((1, 6, 12), np.float32), 1.0, bound=0.0)
    _, b1 = R.step(got, g40["b_w1"], g40["b_b1"], g40["b_w2"], np.zeros((1, 6, 12), np.float32), 1.0, bound=b0)
    _within("checkpoint grid", g40["g_x1"], got, b1)
    assert np.array_equal(got[..., 0], g40["g_x0"][..., 0]) and np.array_equal(got[..., -1], g40["g_x0"][..., -1])


def test_mask_twin():
    """floor(unit23(word) + rate) in float32: rate 0 never fires, rate 1 - 2^-24 fires wherever u + rate rounds to 1, rate 0.5 splits at
    u = 0.5, a map mixes them; the words are oracle.rng.u32's at offset t B H W."""
    from oracle import rng
    b, h, w, t = 3, 5, 7, 4
    n = b * h * w
    u = R.philox_u(11, 2, t, b, h, w)
    words = rng.u32(11, 2, n, offset=t * n).reshape(b, h, w)
    assert np.array_equal(u, ((words >> 9).astype(np.float64) + 0.5) * 2.0 ** -23)       # exact in float32
    assert u.min() > 0 and u.max() < 1
    assert not R.mask_of(u, 0.0).any()
    assert np.array_equal(R.mask_of(u, 0.5), (u >= 0.5).astype(np.float32))
    near1 = np.float32(1 - 2.0 ** -24)
    want = (u.astype(np.float64) + float(near1) >= 1.0 - 2.0 ** -25).astype(np.float32)    # u >= 2^-23 > 2^-25: every pixel fires
    assert np.array_equal(R.mask_of(u, near1), want) and want.all()
    m = np.linspace(0, 1, h * w, dtype=np.float32).reshape(h, w)
    got = R.mask_of(u, m)
    assert np.array_equal(got, np.floor(u + m[None])) and 0 < got.mean() < 1
    # a run split into calls sees one stream: steps t and t + 1 are consecutive words
    both = R.unit23(rng.u32(11, 2, 2 * n, offset=t * n)).reshape(2, b, h, w)
    assert np.array_equal(both[0], u) and np.array_equal(both[1], R.philox_u(11, 2, t + 1, b, h, w))


@pytest.mark.parametrize("case", R.EXACT_CASES[:3] + R.EXACT_CASES[6:8], ids=lambda c: "x".join(map(str, c)))
def test_exact_family_is_exact(case):
    """float32 in two summation orders and float64 give identical bits, and every operand splits exactly into hi + lo bf16"""
    seed, b, c, h, w, hidden, n, dense = case
    x, w1, b1, w2, u = R.exact_family(seed, b, c, h, w, hidden, n, dense)
    k = dict(rate=0.5, keep=True)
    f64 = R.steps(x, w1, b1, w2, u, **k)
    fwd = R.steps(x, w1, b1, w2, u, dtype=np.float32, **k)
    rev = R.steps(x, w1, b1, w2, u, dtype=np.float32, reverse=True, **k)
    assert fwd.dtype == np.float32 and np.array_equal(fwd, rev) and np.array_equal(fwd.astype(np.float64), f64)
    assert not np.array_equal(f64[-1], f64[0])

    def splits(v):
        v = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
        hi = v.bfloat16().float()
        lo = (v - hi).bfloat16().float()
        return bool((hi + lo == v).all())
    for s in f64[:-1]:
        p = R.perception(s)
        hid = np.maximum(np.einsum("nk,bkyx->bnyx", w1.astype(np.float64), p) + b1[None, :, None, None], 0)
        assert splits(p) and splits(hid)
    assert splits(w1) and splits(w2)


def test_every_mutant_changes_a_compared_result(g40):
    a = [g40[f"a_{k}"] for k in ("x0", "w1", "b1", "w2")]
    u = g40["a_u"][0]
    want, bound = R.step(*a, u, bound=0.0)
    for m in R.MUTANTS[:7]:
        got = R.step(*a, u, mutant=m)
        assert (np.abs(got - want) > bound).any(), m
        # ... and on the exact family, where the comparison is bit for bit
        x, w1, b1, w2, ue = R.exact_family(2, 3, 12, 5, 7, 96, 1, True)
        assert not np.array_equal(R.step(x, w1, b1, w2, ue[0], mutant=m), R.step(x, w1, b1, w2, ue[0])), m
    # the window mutants on the GPU test's window case (nca_ref.WINDOWS: the margin-less window is what shows the torus)
    x, w1, b1, w2, ue = R.exact_family(11, 2, 12, 6, 12, 96, 3, False)
    ref = R.window_rounds(x, w1, b1, w2, ue)
    for m in R.MUTANTS[7:]:
        assert not np.array_equal(R.window_rounds(x, w1, b1, w2, ue, mutant=m), ref), m
    assert not np.array_equal(R.checkgrid_round(g40, "window_no_margin"), R.checkgrid_round(g40))


# ---- host logic of maua_amd/nca.py -----------------------------------------------------------------------------------------------------

def test_frame_schedules_and_fade():
    from maua_amd import nca
    assert [nca.evolution_steps(k) for k in (0, 29, 30, 59, 60, 149, 150, 599)] == [1, 1, 2, 2, 4, 16, 32, 32]
    assert [nca.ratemap_steps(k) for k in (0, 29, 30, 47, 48, 60, 149, 150, 599)] == [1, 1, 2, 2, 3, 4, 31, 32, 32]
    assert any(nca.evolution_steps(k) != nca.ratemap_steps(k) for k in range(150))
    assert nca.fade(0) == 1.0 and nca.fade(400) == 1.0 and nca.fade(450) == 0.5 and nca.fade(500) == 0.0


def test_pool_injection_schedule():
    from maua_amd import nca
    assert [i for i in range(100) if nca.inject_seed(i)] == [0, 32, 64, 96]


class CA(torch.nn.Module):
    """a test-local class of the reference's name and attributes: what train.py:249 pickles"""

    def __init__(self, chn=12, hidden_n=96):
        super().__init__()
        self.chn = chn
        self.w1 = torch.nn.Conv2d(chn * 4, hidden_n, 1)
        self.w2 = torch.nn.Conv2d(hidden_n, chn, 1, bias=False)


def test_load_ca_state_dict_and_pickled_module(tmp_path):
    from maua_amd import nca
    torch.manual_seed(3)
    src = CA(8, 64)
    torch.save(src.state_dict(), tmp_path / "sd.pt")
    torch.save(src, tmp_path / "module.pt")
    for name in ("sd.pt", "module.pt"):
        got = nca.load_ca(tmp_path / name)
        assert isinstance(got, nca.CA) and (got.chn, got.hidden_n) == (8, 64)
        for k, v in src.state_dict().items():
            assert torch.equal(got.state_dict()[k], v), (name, k)
    nca.save(got, tmp_path / "again.pt")
    assert torch.equal(nca.load_ca(tmp_path / "again.pt").w2.weight, src.w2.weight)
    fresh = nca.CA()
    assert fresh.w1.weight.shape == (96, 48, 1, 1) and fresh.w1.bias.shape == (96,) and fresh.w2.weight.shape == (12, 96, 1, 1)
    assert not fresh.w2.weight.any() and "w2.bias" not in fresh.state_dict()


class _Evil:
    def __reduce__(self):
        import os
        return (os.system, ("true",))


def test_load_ca_refuses_other_globals(tmp_path):
    from maua_amd import nca
    bad = CA()
    bad.extra = _Evil()
    torch.save(bad, tmp_path / "bad.pt")
    with pytest.raises(pickle.UnpicklingError, match="may not reference"):
        nca.load_ca(tmp_path / "bad.pt")
    torch.save({"something": torch.zeros(1)}, tmp_path / "other.pt")
    with pytest.raises(ValueError, match="not an NCA checkpoint"):
        nca.load_ca(tmp_path / "other.pt")


def test_module_path_parsers():
    import maua.nca
    import maua.nca.generate as G
    import maua.nca.train as T
    a = T.train_parser().parse_args(["style.jpg", "out"])
    assert (a.style_file, a.out_dir, a.steps) == ("style.jpg", "out", 7500)
    a = G.generate_parser().parse_args(["style.jpg", "out"])
    assert (a.style_file, a.out_dir, a.num_frames, a.products) == ("style.jpg", "out", 600, "split")
    assert maua.nca.CA is T.CA
    with pytest.raises(SystemExit):
        G.generate_parser().parse_args(["only-one"])


def test_step_refusals_name_the_limit():
    """maua_nca_check is host only: the sizes the kernel is built for, and the window's geometry"""
    import ctypes as C
    from maua_amd import _lib as L, nca
    l = L.lib()

    def check(chn, hidden, dtype, **kw):
        f = dict(x=64, B=1, H=8, W=8, w1=64, b1=64, w2=64, n_steps=1, rate=0.5)
        f.update(kw)
        d = nca.NcaDesc(**f)
        rc = l.maua_nca_check(None, chn, hidden, dtype, C.byref(d))
        return rc, l.maua_last_error().decode()
    assert check(12, 96, L.F32)[0] == 0 and check(16, 128, L.F32_SPLIT)[0] == 0 and check(4, 32, L.F32)[0] == 0
    for chn, hidden in ((10, 96), (20, 96), (12, 100), (12, 160), (0, 96)):
        rc, msg = check(chn, hidden, L.F32)
        assert rc != 0 and "multiple of 4 up to 16" in msg and "multiple of 32 up to 128" in msg
    assert "MAUA_F32 or MAUA_F32_SPLIT" in check(12, 96, L.BF16)[1]
    assert "at least 3" in check(12, 96, L.F32, H=2)[1]
    assert check(12, 96, L.F32, steps_per_launch=2)[0] == 0 and check(12, 96, L.F32, steps_per_launch=4)[0] == 0
    assert "1, 2 or 4" in check(12, 96, L.F32, steps_per_launch=3)[1]
    assert "window mode" in check(12, 96, L.F32, steps_per_launch=2, col0=2, W_sub=6, margin=1)[1]
    assert check(12, 96, L.F32, col0=2, W_sub=6, margin=1)[0] == 0
    assert "window" in check(12, 96, L.F32, col0=4, W_sub=6, margin=1)[1]
    assert "margin" in check(12, 96, L.F32, col0=0, W_sub=6, margin=3)[1]


def test_gradient_restatement_matches_recorded_autograd(g40):
    """nca_ref.vjp (float64, on the float64 restatement's own states) against torch.autograd through three of the reference's steps"""
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    states = R.steps(g40["v_x0"], *prm, g40["v_u"], keep=True)
    want, bound = R.vjp(states, *prm, g40["v_u"], g40["v_g_last"], bound=True)
    # autograd differentiates the reference's float32 forward: charge the states' float32 error through the gradient's Lipschitz
    # constant by evaluating the gradient on the reference-precision states as well
    states32 = R.steps(g40["v_x0"], *prm, g40["v_u"], keep=True, dtype=np.float32)
    near = R.vjp(states32, *prm, g40["v_u"], g40["v_g_last"])
    for name, w, b, n in zip(("g_first", "dw1", "db1", "dw2"), want, bound, near):
        _within(f"autograd {name}", g40[f"v_{name}"].reshape(w.shape), w, b + np.abs(n - w))
    # the adjoint is the transpose: <perception(x), q> == <x, adjoint(q)>
    rng = np.random.default_rng(0)
    x, q = rng.standard_normal((2, 3, 5, 7)), rng.standard_normal((2, 12, 5, 7))
    assert abs((R.perception(x) * q).sum() - (x * R.adjoint_perception(q)).sum()) < 1e-12
    # a zero mask passes g through and leaves no parameter gradient
    g, dw1, db1, dw2 = R.vjp(states, *prm, g40["v_u"], g40["v_g_last"], rate=0.0)
    assert np.array_equal(g, g40["v_g_last"].astype(np.float64)) and not dw1.any() and not db1.any() and not dw2.any()


# ---- the training loss (train.py:122-142, 228-229) -----------------------------------------------------------------------------------------

def _style_case(g40):
    import perceptor_ref as P
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    x0, u = R.style_case()
    assert np.array_equal(x0, g40["v_x0"]) and np.array_equal(u, g40["v_u"]), "the fixture's inputs are nca_ref.style_case's"
    net, targets = R.style_net(), [t.astype(np.float64) for t in R.style_targets()]
    img = R.steps(x0, *prm, u)[:, :3]
    return P, net, targets, img, P.forward(net, img)


def test_style_loss_restatement_matches_recorded(g40):
    """calc_styles / style_loss of the reference on the 64-64-pool-128 stand-in against nca_ref.gram_mean_grad, inside the float32 bound of
    the same operations (perceptor_ref's per-layer bounds + gram_mean_bounds).  The image differs by the three steps' float32 error: the
    restatement on the float32-evaluated steps' image measures what that moves."""
    P, net, targets, img, acts = _style_case(g40)
    loss, eloss, grad, bound = R.gram_mean_grad_bound(net, acts, targets, "f32")
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    img32 = R.steps(g40["v_x0"], *prm, g40["v_u"], dtype=np.float32)[:, :3].astype(np.float64)
    loss32, grad32 = R.gram_mean_grad(net, img32, targets)
    r = abs(float(g40["v_loss"]) - loss) / (eloss + abs(loss32 - loss) + 2.0 ** -24 * loss)
    print(f"style loss: error / bound = {r:.3g}")
    assert r <= 1
    _within("dL/dx_3", g40["v_g_last"][:, :3], grad, bound + np.abs(grad32 - grad))
    assert not g40["v_g_last"][:, 3:].any()
    # the reference's activations carry the float32 error of its convolutions: layer by layer, |W| e + the layer's own bound (ReLU is
    # 1-Lipschitz, a pooled value moves by at most the largest error in its window); a Gram entry then moves by (|F| e^T + e |F|^T + e e^T)
    plan, params, pre, rep = net
    ef, k = [], 0
    for i, c in enumerate(plan):
        if c == 0:
            ef.append(P.maxpool2(ef[-1]))
        elif i == 0:
            ef.append(P.conv0_bound(img, pre, *params[0], rep, acts[0], "f32"))
            k = 1
        else:
            w, bias = params[k]
            ef.append(P.conv3x3(ef[-1], np.abs(w)) + P.conv_bound(acts[i - 1], w, bias, acts[i], "f32"))
            k += 1
    for e, key, stride in zip(R.STYLE_TAPS, ("v_gram0", "v_gram1"), (8, 32)):
        hw = acts[e].shape[2] * acts[e].shape[3]
        fa, fe = np.abs(acts[e]).reshape(2, plan[e], -1), ef[e].reshape(2, plan[e], -1)
        moved = (fa @ fe.transpose(0, 2, 1) + fe @ fa.transpose(0, 2, 1) + fe @ fe.transpose(0, 2, 1)).mean(0) / hw
        gm = (P.gram(acts[e]) / hw).mean(0)
        gm32 = R.calc_styles(net, img32)[0][R.STYLE_TAPS.index(e)].mean(0)
        b = P.gram_bound(acts[e]).mean(0) / hw + 4 * R.EPS * np.abs(gm) + np.abs(gm32 - gm) + moved + 1e-300     # (dead channels: 0 against 0)
        _within(f"mean Gram of entry {e}", g40[key], gm[::stride], b[::stride])


def test_head_mutants_change_a_compared_result(g40):
    P, net, targets, img, acts = _style_case(g40)
    loss, eloss, grad, bound = R.gram_mean_grad_bound(net, acts, targets, "f32")
    assert R.HEAD_MUTANTS == ("gram_no_hw", "mean_after_square") and len(R.MUTANTS) + len(R.HEAD_MUTANTS) == 11
    for m in R.HEAD_MUTANTS:
        lm, gm = R.gram_mean_grad(net, img, targets, mutant=m)
        assert abs(lm - loss) > eloss and (np.abs(gm - grad) > bound).any(), m


def test_gram_mean_gradient_is_the_loss_derivative():
    net, targets = R.style_net(), [t.astype(np.float64) for t in R.style_targets()]
    img = R.style_image(5, 2, 16, 16)
    loss, grad = R.gram_mean_grad(net, img, targets)
    d = np.random.default_rng(0).standard_normal(img.shape) * 1e-7
    up, _ = R.gram_mean_grad(net, img + d, targets)
    dn, _ = R.gram_mean_grad(net, img - d, targets)
    assert abs((up - dn) / 2 - (grad * d).sum()) <= 1e-5 * abs((grad * d).sum())


def test_adam_first_step_restatement():
    """nca_ref.adam_first_step against torch.optim.Adam in float64"""
    rng = np.random.default_rng(2)
    p, g = rng.standard_normal(50), rng.standard_normal(50)
    g = R.normalise(g)
    t = torch.nn.Parameter(torch.from_numpy(p.copy()))
    opt = torch.optim.Adam([t], 1e-3)
    t.grad = torch.from_numpy(g.copy())
    opt.step()
    assert np.abs(t.detach().numpy() - R.adam_first_step(p, g)).max() < 1e-15


def test_load_style_thumbnail_and_crop(tmp_path):
    import PIL.Image
    from maua_amd import nca
    a = np.random.default_rng(1).integers(0, 256, (150, 260, 3), dtype=np.uint8)
    PIL.Image.fromarray(a).save(tmp_path / "s.png")
    img = nca.load_style(tmp_path / "s.png")            # thumbnail 128 x 74 -> centre crop to 128 x 64
    assert tuple(img.shape) == (1, 3, 64, 128) and img.dtype == torch.float32 and 0 <= float(img.min()) and float(img.max()) <= 1
    ref = PIL.Image.fromarray(a)
    ref.thumbnail((128, 128), PIL.Image.LANCZOS)
    assert ref.size == (128, 74)
    assert np.array_equal(np.float32(ref)[5:69].transpose(2, 0, 1) / np.float32(255), img[0].numpy())
    PIL.Image.fromarray(a[:20, :10]).save(tmp_path / "tiny.png")
    with pytest.raises(ValueError, match="at least 16"):
        nca.load_style(tmp_path / "tiny.png")


def test_ca_copies_and_backward_needs_step0():
    import copy
    from maua_amd import nca
    ca = nca.CA()
    ca._handles[("f32", 0)] = object()
    assert copy.deepcopy(ca)._handles == {} and len(ca._handles) == 1
    with pytest.raises(FileNotFoundError):
        nca.load_ca("/nonexistent/ca.pt")


def test_restated_training_run_diverges_at_1e_3_and_descends_at_1e_4():
    """tests/test_gpu_nca_train.py runs train() for 20 iterations at lr 1e-4 and not at the reference's 1e-3.  This is that run (same style
    image, initialisation, pool draws and masks) in float64: at 1e-3 the loss passes a million times its first value within 20 iterations
    (normalised gradients move every weight by about lr per iteration, and on the random stand-in network a step's gain passes 1 once
    |w2| is about 0.01); at 1e-4 the 20th loss is below the first."""
    style = np.random.default_rng(6).integers(0, 256, (16, 16, 3), dtype=np.uint8)
    fast = R.train_run(style, 1e-3, 20, stop_above=1e7)
    print(f"lr 1e-3: first loss {fast[0]:.4g}, left at iteration {len(fast) - 1} with {fast[-1]:.4g}")
    assert fast[-1] > 1e6 * fast[0]
    slow = R.train_run(style, 1e-4, 20)
    print(f"lr 1e-4: first loss {slow[0]:.4g}, 20th {slow[-1]:.4g}")
    assert slow[0] == fast[0] and slow[-1] < slow[0]
