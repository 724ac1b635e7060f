"""CPU side of tests/test_gpu_perceptor.py: what its float64 reference (tests/perceptor_ref.py) and its exact family rest on.

  * the reference's full chain - first convolution with either padding and the input affine, convolutions, pooling, both loss heads,
    the hand-walked gradient - equals torch.autograd in float64 on torch.nn.functional's conv2d / max_pool2d, on tie-free Gaussian
    inputs, to 1e-12 of the gradient's maximum; fed its own activations it is that chain's gradient
  * the pool adjoint's tie rule (first maximum, row-major, strict >) is torch's CPU max_pool2d backward on inputs full of ties
  * the exact family: every stored value of every case is representable in the storage types the device test runs it in, every
    partial sum stays below 2^24 units of the values' last bit (so float32 sums are exact in any order), the pooled activations hold
    every one of the 15 possible sets of tied maxima, and whole pixels are zero after ReLU"""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import perceptor_ref as R  # noqa: E402


def _torch_chain(net, img, style, lpips, strength, scale):
    """the same network and heads on torch.nn.functional, float64, autograd: (loss terms, gradient, activations)"""
    plan, params, pre, replicate = net
    mul, add, mean, std = pre
    x = torch.from_numpy(img).requires_grad_(True)
    h = ((x * mul + add) - torch.tensor(mean, dtype=torch.float64).view(1, 3, 1, 1)) / torch.tensor(std, dtype=torch.float64).view(1, 3, 1, 1)
    acts, k = [], 0
    for i, c in enumerate(plan):
        if c == 0:
            h = F.max_pool2d(h, 2)
        else:
            w, b = (torch.from_numpy(p) for p in params[k])
            if i == 0 and replicate:
                h = F.conv2d(F.pad(h, (1, 1, 1, 1), mode="replicate"), w, b)
            else:
                h = F.conv2d(h, w, b, padding=1)
            h = F.relu(h)
            k += 1
        acts.append(h)
    total = 0.0
    for entry, T in style.items():
        f = acts[entry].flatten(2)
        D = f @ f.transpose(1, 2) - torch.from_numpy(T)
        total = total + (strength * (D * D).sum((1, 2)) / (D.abs().sum((1, 2)) + 1e-8) / (D.shape[1] * D.shape[2])).sum()
    for entry, (nt, lin) in lpips.items():
        f = acts[entry]
        n = f / (f.pow(2).sum(1, keepdim=True).sqrt() + R.EPS_LPIPS)
        val = (torch.from_numpy(lin).view(1, -1, 1, 1) * (n - torch.from_numpy(nt)) ** 2).sum(1)
        total = total + scale * val.flatten(1).mean(1).sum()
    total.backward()
    return float(total.detach()), x.grad.numpy(), [a.detach().numpy() for a in acts]


def _gauss_net(plan, replicate, seed):
    rng = np.random.default_rng(seed)
    params, cin = [], 3
    for c in plan:
        if c:
            params.append((rng.normal(size=(c, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9)), rng.normal(size=(c,)) * 0.05))
            cin = c
    return (list(plan), params, R.GAUSS_PRE, replicate)


@pytest.mark.parametrize("plan,taps,H,W,replicate", [((8,), (0,), 1, 1, 1), ((8,), (0,), 3, 5, 0), ((16,), (0,), 1, 7, 1),
                                                    ((8, 0, 8), (2,), 6, 10, 1), ((8, 8, 0, 16, 8), (1, 4), 8, 12, 1),
                                                    ((8, 8, 0, 16, 8), (1, 4), 4, 4, 0), ((8, 8), (0, 1), 5, 3, 1)])
@pytest.mark.parametrize("head", ["style", "lpips"])
def test_reference_chain_equals_autograd(plan, taps, H, W, replicate, head):
    B, seed = 2, H * 31 + W + len(plan)
    rng = np.random.default_rng(seed)
    net = _gauss_net(plan, replicate, seed)
    img = rng.normal(size=(B, 3, H, W))
    acts = R.forward(net, img)
    style, lpips, heads, total = {}, {}, {}, 0.0
    for j, e in enumerate(taps):
        C, (h, w) = plan[e], acts[e].shape[2:]
        if head == "style":
            T = rng.normal(size=(B, C, C) if j % 2 == 0 else (C, C)) * h * w
            style[e] = T
            loss, _, heads[e] = R.style_head(acts[e], T, 2.5)
            total += loss.sum()
        else:
            nt = R.lpips_normalize(np.abs(rng.normal(size=(B if j % 2 == 0 else 1, C, h, w))))
            lin = rng.random(C) / C
            lpips[e] = (nt, lin)
            _, dist, heads[e] = R.lpips_head(acts[e], nt, lin, 3.0)
            total += 3.0 * dist.sum()
    want_total, want, tacts = _torch_chain(net, img, style, lpips, 2.5, 3.0)
    for a, b in zip(acts, tacts):
        assert np.abs(a - b).max() <= 1e-12 * max(np.abs(b).max(), 1.0)
    for i in range(len(plan)):
        if plan[i] == 0:    # tie-free: the top two of every window differ
            top = np.sort(R._windows(acts[i - 1]), -1)
            assert (top[..., 3] > top[..., 2]).all() or (acts[i] == 0).any()
    assert abs(total - want_total) <= 1e-12 * abs(want_total)
    got = R.backward(net, acts, heads)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    # and the walk with its error bound returns the same gradient (the bound is exercised on the device)
    got2, bound = R.backward_with_bound(net, acts, heads, {e: np.zeros_like(v) for e, v in heads.items()}, "f32")
    assert np.array_equal(got, got2) and (bound >= 0).all() and np.isfinite(bound).all()


def test_lpips_head_at_a_zero_feature_vector():
    """value and gradient are finite there, and equal the closed form without the projection term"""
    rng = np.random.default_rng(3)
    Fm = np.abs(rng.normal(size=(1, 64, 2, 2)))
    Fm[:, :, 0, 1] = 0
    nt = R.lpips_normalize(np.abs(rng.normal(size=(1, 64, 2, 2))))
    lin = rng.random(64)
    val, dist, hg = R.lpips_head(Fm, nt, lin, 2.0)
    assert np.isfinite(val).all() and np.isfinite(hg).all()
    assert np.allclose(val[0, 0, 1], (lin * nt[0, :, 0, 1] ** 2).sum(), rtol=1e-14)
    assert np.allclose(hg[0, :, 0, 1], 2 * lin * (-nt[0, :, 0, 1]) * (2.0 / 4) / R.EPS_LPIPS, rtol=1e-14)


def test_pool_adjoint_takes_torch_first_maximum():
    """integer inputs full of ties: the reference's adjoint is torch's CPU max_pool2d backward; and the two windows that tell the rules
    apart - all equal -> the first pixel, [[0, 2], [2, 1]] -> the first 2"""
    rng = np.random.default_rng(0)
    x = rng.integers(0, 3, size=(2, 5, 8, 12)).astype(np.float64)
    g = rng.normal(size=(2, 5, 4, 6))
    pats = set(np.unique(R.tie_patterns(x)).tolist())
    assert pats == set(range(1, 16)), "every set of tied maxima"
    t = torch.from_numpy(x).requires_grad_(True)
    F.max_pool2d(t, 2).backward(torch.from_numpy(g))
    assert np.array_equal(R.maxpool2_adjoint(x, g), t.grad.numpy())
    assert np.array_equal(R.maxpool2(x), F.max_pool2d(t, 2).detach().numpy())
    one = np.ones((1, 1, 1, 1))
    assert np.array_equal(R.maxpool2_adjoint(np.full((1, 1, 2, 2), 7.0), one).reshape(-1), [1, 0, 0, 0])
    assert np.array_equal(R.maxpool2_adjoint(np.array([[[[0.0, 2.0], [2.0, 1.0]]]]), one).reshape(-1), [0, 1, 0, 0])
    for a in (np.full((1, 1, 2, 2), 7.0), np.array([[[[0.0, 2.0], [2.0, 1.0]]]])):
        t = torch.from_numpy(a).requires_grad_(True)
        F.max_pool2d(t, 2).backward(torch.from_numpy(one))
        assert np.array_equal(R.maxpool2_adjoint(a, one), t.grad.numpy())


def test_conv0_adjoint_folds_the_replicate_padding():
    """a 1 x 1 image under replicate padding stands in for all nine taps; a corner of a larger one for three virtual pixels"""
    rng = np.random.default_rng(1)
    w = rng.normal(size=(4, 3, 3, 3))
    g = rng.normal(size=(1, 4, 1, 1))
    got = R.conv0_adjoint(g, w, (1.0, 1.0, 1.0), True)
    assert np.allclose(got.reshape(3), np.einsum("o,ockl->c", g.reshape(4), w), rtol=1e-13)
    assert np.allclose(R.conv0_adjoint(g, w, (1.0, 1.0, 1.0), False).reshape(3), np.einsum("o,oc->c", g.reshape(4), w[:, :, 1, 1]), rtol=1e-13)


@pytest.mark.parametrize("i", range(len(R.EXACT_CASES)))
def test_exact_family_premises(i):
    case = R.EXACT_CASES[i]
    d = R.exact_case(case)
    plan, pre = d["net"][0], d["net"][2]
    mul, add, mean, std = pre
    # the pre-processing is exact in float32: dyadic mul / add / mean, std powers of two (1.f / std and mul * istd exact)
    assert all(np.log2(s) % 1 == 0 for s in std) and all(float(np.float32(v)) == v for v in (mul, add) + tuple(mean))
    assert R.vjp_factors(pre) == [mul / s for s in std]
    assert R.representable(d["img"], "f32") and np.array_equal(R.pre_affine(d["img"], pre), np.round(R.pre_affine(d["img"], pre)))
    for a in d["acts"]:
        assert np.array_equal(a, np.round(a)) and a.max() < 256
    assert (d["acts"][0].max(1) == 0).any() == (d["img"].shape[2] * d["img"].shape[3] >= 8), "whole pixels zero after ReLU"
    assert (R.conv3x3(R.pre_affine(d["img"], pre), *d["net"][1][0], d["net"][3]) < 0).any(), "negative pre-activations"
    for T in d["targets"]:
        assert R.representable(T, "f32")
    assert R.exact_premises(d, "f32") is None, R.exact_premises(d, "f32")
    why = R.exact_premises(d, "bf16")
    if i in R.EXACT_F32_ONLY:
        assert why is not None, "representable in bf16 after all: take the case off EXACT_F32_ONLY"
    else:
        assert why is None, why
    assert np.abs(d["grad"]).max() > 0 and np.isfinite(d["grad"]).all()


def test_exact_pool_cases_hold_every_tie_pattern():
    """most pooling windows of the exact family hold two, three or four equal maxima, in every position order"""
    seen, tied, n = set(), 0, 0
    for case in R.POOL_CASES:
        d = R.exact_case(case)
        p = R.tie_patterns(d["acts"][0])
        seen |= set(np.unique(p).tolist())
        tied += int(np.isin(p, (1, 2, 4, 8), invert=True).sum())
        n += p.size
    assert seen == set(range(1, 16)), sorted(seen)
    assert tied > n / 2, (tied, n)


def test_exact_style_head_sign_of_zero_and_transpose():
    """D0 has zeros (sign 0 contributes nothing), is not symmetric, and Sym is the symmetrised closed form"""
    d = R.exact_case(R.MASK_CASES[1])
    for (name, sym, _) in [s for s in d["stored"] if s[0].startswith("sym")]:
        assert np.array_equal(sym, sym.transpose(0, 2, 1)) and (sym == 0).mean() > 0.9 and (sym != 0).any()
    F0 = d["acts"][1]
    T = d["targets"][0]
    loss, dG, hg = R.style_head(F0, T, d["strength"], eps=0.0)
    assert not np.array_equal(dG, dG.transpose(0, 2, 1))
    assert np.array_equal(hg, d["heads"][1])


def test_gram_workspace_is_not_monotone_in_the_pixel_count():
    """what the one-handle test on the device walks through: B = 3 at 16 x 16 and B = 2 at 16 x 24 have the same B H W, and the second
    needs more Gram partial slices (B ceil(hw / 256)) than the first"""
    need = lambda B, H, W: B * -(-(H * W) // R.GRAM_PX)   # noqa: E731
    assert 3 * 16 * 16 == 2 * 16 * 24 and need(3, 16, 16) == 3 and need(2, 16, 24) == 4
