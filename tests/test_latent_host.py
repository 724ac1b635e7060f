"""What tests/test_gpu_latent_kernels.py rests on, checked without a GPU: the twin tests/latent_ref.py against independent
implementations (F.interpolate, a dense natural-spline solve, oracle/latent.py, oracle/noise.py, torch.round, numpy indexing), the
preconditions of the exact families per input (products and sums exactly representable, no tie in a decision), the library's short
sine and cosine restated on the CPU against the allowance the header claims for them, and that every comparison rejects off-by-one
mutants of the twin."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import latent_ref as R  # noqa: E402
from oracle import latent as OL, noise as ON  # noqa: E402

V = R.V


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def inside(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return bool(np.isfinite(err).all() and (err <= bound).all())


# ----------------------------------------------------------------------------------------------------------------- twins against others
@pytest.mark.parametrize("n,size", R.RESAMPLE + ((3, 7), (11, 64), (64, 11), (100, 333)))
def test_resample_is_torch_interpolate(n, size):
    """torch's CPU kernel, bit for bit, is the twin with its two multiply-adds contracted (this build of torch contracts them); the
    uncontracted chain the library pins differs from it by those roundings alone: the source position by v of scale (j + 0.5), which
    moves the value by that times the step between the two rows (the interpolant is continuous in the position, also across an
    integer), and 2 v of the terms for each form's own roundings"""
    x = R.normal((n, 7), n * 100 + size)
    want = F.interpolate(torch.from_numpy(x).T[None], size=size, mode="linear", align_corners=False)[0].T.numpy()
    assert same(R.resample_linear32(x, size, contract=True), want)
    got = R.resample_linear32(x, size)
    i0, i1, l0, l1, src = R.resample_index32(n, size)
    d_src = V * (np.float64(n) / size * (np.arange(size) + 0.5))[:, None]
    step = np.abs(np.diff(x.astype(np.float64), axis=0)).max(0)[None] if n > 1 else np.zeros((1, 7))
    mag = R.resample_linear64(np.abs(x), size)
    assert inside(got, want.astype(np.float64), 2 * d_src * step + 4 * V * mag)
    assert inside(got, R.resample_linear64(x, size), 2 * d_src * step + 3 * V * mag)
    assert i0.min() >= 0 and i1.max() <= n - 1 and (i1 - i0 <= 1).all() and ((i1 == i0) == (i0 == n - 1)).all()
    assert ((l1 >= 0) & (l1 <= 1)).all() and same(l0.astype(np.float64) + l1, np.ones(size)) and (src >= 0).all()
    if n == size:
        assert same(got, x), "size = n: the identity"
    if n == 1:
        assert inside(got, np.repeat(x.astype(np.float64), size, 0), 3 * V * np.abs(x))


def test_resample_lands_next_to_an_integer():
    """3 -> 9 and 7 -> 21: the exact source position is an integer at some j, the float32 scale is not 1/3, and the float32 position
    lands on the integer or one ulp from it: on either side the result is that row within the continuity bound above"""
    for n, size in ((3, 9), (7, 21)):
        src = R.resample_index32(n, size)[4].astype(np.float64)
        exact = np.maximum((np.arange(size) + 0.5) * n / size - 0.5, 0)
        hit = (exact == np.round(exact)) & (exact > 0)
        assert hit.sum() >= 2 and float(np.float32(n) / np.float32(size)) != n / size
        assert (np.abs(src[hit] - exact[hit]) <= 4 * V * exact[hit]).all()


@pytest.mark.parametrize("n", (2, 3, 4, 7))
def test_spline_is_the_dense_solve_and_the_oracle(n):
    tk = R.spline_knots(n)
    y = R.normal((n, 9), n)
    te = R.spline_eval_points(tk, 16)
    val, bound = R.spline_natural(tk, y, te)
    dense = R.spline_dense(tk, y, te)
    orc = OL.natural_cubic_spline(tk, y, te)
    scale = np.abs(val).max()
    assert np.abs(val - dense).max() <= 1e-12 * scale and np.abs(val - orc).max() <= 1e-12 * scale
    assert (bound >= V * np.abs(val)).all() and (bound <= 1.001 * V * np.abs(val) + 1e-12 * scale).all()
    at_knots = R.spline_natural(tk, y, tk)[0]               # an interpolant: the data at the knots
    assert np.abs(at_knots - y).max() <= 1e-13 * scale
    lo, hi = (te < tk[0]).any(), (te > tk[-1]).any()
    assert lo and hi, "the end cubics are evaluated outside the knots"


def test_spline_loop_points_wrap():
    te = R.loop_eval_points(9, 2)
    assert te[-1] == 0.0 and te[4] == 0.0 and (te[1:4] > 0).all()
    y = torch.from_numpy(R.normal((4, 5), 3))
    tk = np.linspace(0, 1, 5)
    Y = np.concatenate((y.numpy(), y.numpy()[:1]))
    val = R.spline_natural(tk, Y, te)[0]
    assert np.abs(val - OL.spline_loop_latents(y, 9, 2).numpy()).max() <= 1e-6
    assert np.abs(val[-1] - Y[0]).max() <= 1e-14


def test_spline_exact_family():
    """data linear in t on dyadic knots with power-of-two intervals: M = 0 exactly and the value is alpha t + beta, a float32 number"""
    for n in (2, 3, 7):
        tk = R.spline_knots(n)
        assert all(np.log2(h) == np.round(np.log2(h)) for h in np.diff(tk)) and len(set(np.diff(tk))) == min(n - 1, 4)
        y, alpha, beta = R.spline_linear_data(tk, 11, n)
        assert same(y.astype(np.float64), tk[:, None] * alpha + beta)
        te = R.spline_eval_points(tk, 20)
        val = R.spline_natural(tk, y, te)[0]
        assert same(val, te[:, None] * alpha + beta) and R.is_f32(val)
        assert np.abs(val - R.spline_dense(tk, y, te)).max() <= 1e-13


def test_blend_weighted_sum_merge_against_the_oracle():
    T, L, D = 5, 3, 7
    a, b = R.normal((L, D), 1), R.normal((L, D), 2)
    env = R.envelope(T, 3)
    want = OL.single_weighted(torch.from_numpy(a), torch.from_numpy(b), torch.from_numpy(env)).numpy().reshape(T, -1)
    got = R.blend32(a.reshape(1, -1), b.reshape(1, -1), env)
    assert same(got, want)
    assert same(got[0], a.reshape(-1)) and same(got[-1], b.reshape(-1)), "env 0 and 1 return a and b"
    b64 = R.blend64(a.reshape(1, -1), b.reshape(1, -1), env)
    assert inside(got, b64, 3 * V * (np.abs(a.reshape(1, -1)) + np.abs(b.reshape(1, -1))))
    for A, n in ((5, 3), (1, 1), (4, 4)):
        e = np.abs(R.normal((T, A), A)) + np.float32(0.1)
        lat = R.normal((n, L, D), n)
        want = OL.multi_weighted(torch.from_numpy(lat), torch.from_numpy(e)).numpy().reshape(T, -1)
        val, bound = R.weighted_sum(e, lat.reshape(n, -1))
        assert inside(want, val, bound)
    lat, seq, mod = R.normal((T, 18, D), 4), R.normal((T, 18, D), 5), R.envelope(T, 6)
    for mode, name in enumerate(("average", "modulate", "overwrite")):
        for depth, sl in OL.LAYER_SLICES.items():
            want = OL.merge(torch.from_numpy(lat), torch.from_numpy(seq), name, depth, torch.from_numpy(mod)[:, None]).numpy()
            assert same(R.latent_merge32(lat, seq, mod, mode, sl.start, sl.stop), want), (name, depth)
            assert inside(want, R.latent_merge64(lat, seq, mod, mode, sl.start, sl.stop), 3 * V * (np.abs(lat) + np.abs(seq)))


def test_weighted_sum_zero_row_follows_the_reference():
    e = R.f32([[0.0, 0.0], [1.0, -1.0], [1.0, 3.0]])
    lat = R.f32([[1.0, -2.0, 0.5], [1.0, 2.0, -0.5]])
    got = R.weighted_sum32(e, lat)
    with np.errstate(all="ignore"):
        want = OL.multi_weighted(torch.from_numpy(lat)[:, None], torch.from_numpy(e)).numpy().reshape(3, 3)
    assert np.isnan(got[0]).all() and np.isnan(got[1, 0]) and np.isinf(got[1, 1:]).all() and np.isfinite(got[2]).all()
    assert same(got[:2], want[:2])


def test_round_and_gather():
    x = R.round_input()
    for scale in (1.0, 0.5, -1.0, 0.0, 3.0):
        want = torch.round(torch.from_numpy(x) * scale).long().numpy()
        assert same(R.scale_round_index(x, scale), want), scale
    got = R.scale_round_index(R.f32([0.5, 1.5, 2.5, -0.5, -1.5, -2.5]), 1.0)
    assert got.tolist() == [0, 2, 2, 0, -2, -2]
    assert (R.scale_round_index(x, 0.0) == 0).all()
    src = R.normal((5, 4), 0)
    idx = R.gather_input(5, 9, 1)
    assert -1 in idx and -5 in idx and 0 in idx and 4 in idx
    assert same(R.gather_rows(src, idx), src[idx])


@pytest.mark.parametrize("D", R.SLERP_D)
def test_slerp_against_the_oracle(D):
    y = R.slerp_input(2, 3, D, D)
    t = R.f32([0.0, 1.0, 0.25, 0.7])
    out, _, dot, p = R.slerp(y, t)
    ad = 4 * R.measured_dev(np.arccos, np.arccos, [dot])
    cd, sd = 4 * R.measured_dev(np.cos, np.cos, [p]), 4 * R.measured_dev(np.sin, np.sin, [p])
    assert 0 < ad < 1e-6 and 0 < cd < 1e-6 and 0 < sd < 1e-6
    out, bound, dot, p = R.slerp(y, t, ad, cd, sd)
    yt = torch.from_numpy(y)
    want = OL.slerp(yt[:-1], yt[1:], torch.from_numpy(t)).numpy()
    assert want.shape == out.shape and inside(want, out, bound)
    assert (bound < 1e-4).all() and (bound > 0).all()
    ah = y[:-1].astype(np.float64) / np.linalg.norm(y[:-1].astype(np.float64), axis=-1, keepdims=True)
    bh = y[1:].astype(np.float64) / np.linalg.norm(y[1:].astype(np.float64), axis=-1, keepdims=True)
    assert np.abs(out[0] - ah).max() <= 1e-14 and np.abs(out[1] - bh).max() <= 1e-14, "t of 0 and 1: the normalised endpoints"
    assert np.abs(np.linalg.norm(out, axis=-1) - 1).max() <= 1e-14


def test_slerp_parallel_vectors_are_nan_like_the_reference():
    y = np.zeros((2, 1, 4), np.float32)
    y[:, 0, 0] = (2.0, 3.0)
    out = R.slerp(y, R.f32([0.0, 0.5]))[0]
    yt = torch.from_numpy(y)
    want = OL.slerp(yt[:-1], yt[1:], torch.tensor([0.0, 0.5])).numpy()
    assert np.isnan(out).all() and np.isnan(want).all()


# ----------------------------------------------------------------------------------------------------------------- noise
@pytest.mark.parametrize("sigma", R.NOISE_SIGMA)
def test_loop_against_the_oracle(sigma):
    hw, T, i0, B = 1023, 7, 2, 3
    planes = R.normal((3, hw), int(sigma * 100))
    idx = R.loop_idx(T)
    val, _, x0, x1 = R.loop_values(planes, idx[i0:i0 + B], sigma)
    cd, sd = 4 * R.measured_dev(np.cos, np.cos, [x0]), 4 * R.measured_dev(np.sin, np.sin, [x1])
    val, dval, _, _ = R.loop_values(planes, idx[i0:i0 + B], sigma, cd, sd)
    out, bound, scale, rel = R.loop_normalised(val, dval, R.noise_path(hw)[3])
    want = ON.loop(torch.from_numpy(planes).reshape(3, hw, 1), torch.from_numpy(idx), i0, B, sigma).numpy().reshape(B, hw)
    # (the oracle divides by float32(sigma / 50) and sums in torch's order: two more roundings of the argument, the same tree bound)
    extra = 2 * V * np.abs(x1) * np.abs(planes[2].astype(np.float64))[None] * scale[:, None]
    assert inside(want, out, bound + extra)
    assert np.abs(np.sqrt((out ** 2).mean(1)) - 1).max() <= 1e-6
    assert np.abs(x1).max() > {5.0: 10, 0.5: 100, 0.05: 900}[sigma] * 0.9


def test_fast_sin_cos_meet_the_allowance_the_header_claims():
    """noise.hip's sine and cosine, restated operation by operation, against float64: inside 4 x the deviation of the float32 libm
    function over the same arguments, for |x| up to 1e4 (the range the header gives); and what breaks first beyond it"""
    rng = np.random.default_rng(0)
    for lim in (1.0, 20.0, 1e3, 1e4):
        x = R.f32(np.concatenate((rng.uniform(-lim, lim, 400000), np.arange(1, 64) * (np.pi / 4), np.arange(1, 64) * (np.pi / 2) * (lim / 100))))
        x = x[np.abs(x) <= lim]
        for fast, fn in ((R.fast_sin32, np.sin), (R.fast_cos32, np.cos)):
            dev = R.measured_dev(fn, fn, [x])
            err = np.abs(fast(x).astype(np.float64) - fn(x.astype(np.float64))).max()
            print(f"[latent host] {fn.__name__} on |x| <= {lim:g}: libm float32 deviation {dev:.3e}, the short form {err:.3e} ({err / dev:.2f} x)")
            assert 0 < dev < 1.2e-7 and err <= 4 * dev, (lim, fn.__name__, err, dev)


def test_mix_and_combine_against_the_oracle():
    M, hw, B = 3, 12, 4
    n1, n2 = R.normal((M, hw), 1), R.normal((M, hw), 2)
    mod = R.f32(np.random.default_rng(3).uniform(0, 1, (B, M)))
    tn = torch.from_numpy
    val, bound = R.noise_mix(n1, n2, mod)
    want = ON.blend(torch.stack((tn(n1), tn(n2))).reshape(2, M, hw, 1), tn(mod), 0, B).numpy().reshape(B, hw)
    assert inside(want, val, bound)
    val, bound = R.noise_mix(n1, None, mod)
    assert inside(ON.multiply(tn(n1).reshape(M, hw, 1), tn(mod), 0, B).numpy().reshape(B, hw), val, bound)
    x, y = R.normal((B, hw), 4), R.normal((B, hw), 5)
    m = mod[:, :1].copy()
    assert same(R.noise_combine32(x, y, None, 0, 0, 0), ON.average(tn(x), tn(y)).numpy())
    want = ON.modulate(tn(x).reshape(B, hw, 1), tn(y).reshape(B, hw, 1), tn(m), 0, B).numpy().reshape(B, hw)
    assert same(R.noise_combine32(x, y, m[:, 0], 1, 0, 0), want)
    assert same(R.noise_combine32(x, None, None, 2, 0.75, -2.5), ON.scale_bias(tn(x), 0.75, -2.5).numpy())


# ----------------------------------------------------------------------------------------------------------------- preconditions
def test_exact_families_are_exact():
    for M in R.MIX_M:
        n1, n2, mod = R.mix_exact_input(M, 9, 3, M)
        w2 = np.float32(1) - mod
        assert R.products_exact(n1[None], mod[:, :, None]) and R.products_exact(n2[None], w2[:, :, None])
        assert same((1 - mod.astype(np.float64)), w2.astype(np.float64))
        mag = np.abs(mod) @ np.abs(n1) + np.abs(w2) @ np.abs(n2)
        assert mag.max() * 4 < 2 ** 24, "every partial sum, in any order, is a multiple of 1/4 below 2^22"
        val, _ = R.noise_mix(n1, n2, mod)
        assert R.is_f32(val)
    for hw in (5, 300):
        x, y, mod, scale, bias = R.combine_exact_input(3, hw, hw)
        assert R.products_exact(x, mod[:, None]) and R.products_exact(y, (np.float32(1) - mod)[:, None]) and R.products_exact(x, np.float32(scale))
        assert set(mod.tolist()) <= {0.0, 0.25, 0.5, 1.0}


def test_noise_geometry_of_the_cases():
    """the sizes of the cases reach both paths, both sides of both caps, and the first size past each"""
    path = {hw: R.noise_path(hw) for hw in R.NOISE_HW}
    assert [hw for hw in R.NOISE_HW if not path[hw][0]] == [1, 3, 5, 1023, 1025, 8193, 65537]
    assert path[8193][2:] == (33, 33) and path[32 * 1024 + 4][2:] == (33, 33), "one block more than 32 sweeps"
    assert path[65537][2:] == (257, 256) and path[256 * 1024 + 4][2:] == (257, 256), "one block more than the cap of 256: grid-stride"
    assert path[1024][2:] == (1, 1) and path[1028][2:] == (2, 2) and path[4100][2:] == (5, 5) and path[1025][2:] == (5, 5)
    assert set(R.BATCH_HW) <= set(R.NOISE_HW)
    big = [R.noise_path(hw)[3] > 32 for hw in R.BATCH_HW]
    assert big[:3] == [True, False, True] and len({R.noise_path(hw)[0] for hw in R.BATCH_HW}) == 2
    assert {R.noise_path(hw)[2] > 256 for hw in R.BATCH_HW} == {True, False}


# ----------------------------------------------------------------------------------------------------------------- mutants
def test_mutants_are_rejected():
    T, C = 5, 7
    a, b, env = R.normal((T, C), 1), R.normal((T, C), 2), R.envelope(T, 3)
    good = R.blend32(a, b, env)
    for m in ("swap", "row+1"):
        assert not same(good, R.blend32(a, b, env, mutant=m)), m
    e, lat = np.abs(R.normal((T, 5), 4)) + np.float32(0.1), R.normal((3, C), 5)
    val, bound = R.weighted_sum(e, lat)
    assert not inside(R.weighted_sum(e, lat, mutant="no_mod")[0], val, bound), "a % n dropped"
    x = R.round_input()
    for m in ("half_away", "floor"):
        assert not same(R.scale_round_index(x, 1.0), R.scale_round_index(x, 1.0, mutant=m)), m
    src, idx = R.normal((5, C), 6), R.gather_input(5, 9, 1)
    for m in ("neg-1", "lt-1", "row+1"):
        assert not same(R.gather_rows(src, idx), R.gather_rows(src, idx, mutant=m)), m
    for n, size in ((5, 13), (13, 5), (3, 7)):
        xr = R.normal((n, C), n)
        for m in ("no_low_clamp", "clamp_end", "i1+1", "i0-1"):
            if (m, n, size) == ("no_low_clamp", 13, 5):     # (down-sampling never reaches below 0)
                continue
            assert not same(R.resample_linear32(xr, size), R.resample_linear32(xr, size, mutant=m)), (m, n, size)
    tk = R.spline_knots(4)
    y, te = R.normal((4, C), 7), R.spline_eval_points(R.spline_knots(4), 11)
    val, bound = R.spline_natural(tk, y, te)
    for m in ("no_clip_hi", "idx+1"):
        assert not inside(R.spline_natural(tk, y, te, mutant=m)[0], val, bound), m
    # (the interval search's <= against <, mutant "left", cannot show in a value: the spline is continuous at its knots)
    assert inside(R.spline_natural(tk, y, te, mutant="left")[0], val, 1e-13 * np.abs(val).max())
    ys = R.slerp_input(2, 2, 8, 8)
    t = R.f32([0.0, 0.25, 1.0])
    out, bound, _, _ = R.slerp(ys, t, 3e-7, 3e-7, 3e-7)
    assert not inside(R.slerp(ys, t, mutant="1-t")[0], out, bound)
    lat3, seq3, mod = R.normal((T, 4, C), 8), R.normal((T, 4, C), 9), R.envelope(T, 10)
    for mode in (0, 1, 2):
        good = R.latent_merge32(lat3, seq3, mod, mode, 1, 3)
        for m in ("l0+1", "l1+1") + (("swap",) if mode == 1 else ()):
            assert not same(good, R.latent_merge32(lat3, seq3, mod, mode, 1, 3, mutant=m)), (mode, m)
    planes = R.normal((3, 9), 11)
    idx = R.loop_idx(6)
    val, dval, _, _ = R.loop_values(planes, idx[2:4], 5.0, 3e-7, 3e-7)
    for other in (R.loop_values(planes, idx[1:3], 5.0)[0], R.loop_values(planes, idx[3:5], 5.0)[0], R.loop_values(planes, idx[2:4], 5.0, mutant="planes")[0]):
        assert not inside(other, val, dval), "idx[i0 - 1], idx[i0 + 1], planes swapped"
    xc, yc, mc, sc, bi = R.combine_exact_input(3, 9, 12)
    mc = R.f32([0.25, 0.5, 1.0])
    good = R.noise_combine32(xc, yc, mc, 1, sc, bi)
    for m in ("swap", "row+1"):
        assert not same(good, R.noise_combine32(xc, yc, mc, 1, sc, bi, mutant=m)), m
