"""CPU side of tests/test_gpu_image_kernels.py: the twin tests/image_ref.py against everything else the repository has for the same
operations - torch (F.interpolate, F.pad, F.conv2d, autograd in float64), tests/image_pipeline_ref.py (resize_right, adjust_sharpness,
the perlin image), the oracle, maua_amd/image.py's tables and the fixtures g33 / g34 / g37 - the preconditions of the bit-exact
families, and the proof that the GPU file's comparisons (its shapes, its bounds) reject off-by-one mutants of the twin: a mutant is
"rejected" when its distance from the twin exceeds twice the bound somewhere (a kernel computing the mutant would then sit outside the
bound whatever its own rounding), or, for an exact family, when any bit differs."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

sys.path.insert(0, str(Path(__file__).resolve().parent))
import image_pipeline_ref as H  # noqa: E402
import image_ref as R  # noqa: E402

F = np.float32


def load_image_tables():
    """maua_amd/image.py's host functions (resize_tables, tile_origins, blend_weight1d) without the device library"""
    import maua_amd.image as I
    return I


@pytest.fixture(scope="module")
def g37(golden):
    g = golden("g37_image_pipeline")
    g["meta"] = json.loads(str(g["meta_json"]))
    return g


def rejected(mutant, want, bound):
    return bool((np.abs(np.asarray(mutant, np.float64) - want) > 2 * bound).any())


# ---------------------------------------------------------------------------------------------------------------- image_resize
@pytest.mark.parametrize("kernel", ["cubic", "lanczos3"])
def test_image_resize_twin_is_resize_right(kernel):
    I = load_image_tables()
    for Hh, W, Ho, Wo in R.IMAGE_RESIZE_CASES:
        x = R.normal((5 if W <= 4096 else 1, Hh, W), Hh + W)      # (one plane of the 16384-wide case: 20000 taps per output sample)
        ty = [t.numpy() for t in I.resize_tables(Hh, Ho, kernel)] if Hh != Ho else (None, None)
        tx = [t.numpy() for t in I.resize_tables(W, Wo, kernel)] if W != Wo else (None, None)
        for (l, w), (n_in, n_out) in ((ty, (Hh, Ho)), (tx, (W, Wo))):
            if l is not None:                                     # the library's tables are the restated package's
                l2, w2 = H.resize_tables(n_in, n_out, getattr(H, kernel))
                assert np.array_equal(l, l2.numpy()) and np.array_equal(w, w2.float().numpy())
        want, bound = R.image_resize(x, Ho, Wo, *ty, *tx)
        ref = H.resize(torch.from_numpy(x).double(), out_shape=(Ho, Wo), interp_method=getattr(H, kernel)).numpy()
        # resize_right orders the axes by scale; both orders are the same sum in float64 (up to 1e-13)
        assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(ref).max())
        assert (bound > 0).all()
        for mutant in ("tap+1", "tap-1", "clamp_n"):
            bad, _ = R.image_resize(x, Ho, Wo, *ty, *tx, mutant=mutant)
            assert rejected(bad, want, bound), (mutant, Hh, W, Ho, Wo)


# ---------------------------------------------------------------------------------------------------------------- destitch / restitch
def test_restitch_twin_reproduces_the_reference_bit_for_bit(g37):
    I = load_image_tables()
    for name in ("s23", "s33"):
        m = g37["meta"][name]
        Hh, W, T = m["H"], m["W"], m["T"]
        ys, xs = I.tile_origins(Hh, T), I.tile_origins(W, T)
        fade = T - ys[1]
        wy = torch.stack([I.blend_weight1d(T, 0 if y == 0 else fade, 0 if y == ys[-1] else fade) for y in ys]).numpy()
        wx = torch.stack([I.blend_weight1d(T, 0 if x == 0 else fade, 0 if x == xs[-1] else fade) for x in xs]).numpy()
        img = g37[f"{name}_img"].numpy()
        assert np.array_equal(R.destitch(img, T, ys, xs), g37[f"{name}_tiles"].numpy())
        for tiles, out in ((g37[f"{name}_rnd"], g37[f"{name}_rnd_out"]), (g37[f"{name}_tiles"], g37[f"{name}_back"])):
            got, _, _ = R.restitch32(tiles.numpy(), T, ys, xs, wy, wx, Hh, W)
            assert np.array_equal(got, out.numpy()[0], equal_nan=True)


def test_restitch_and_destitch_mutants_are_rejected_on_the_gpu_grids():
    """columns first: destitch differs wherever the grid has two rows and two columns.  restitch sums a pixel's covering tiles in
    visiting order; the two orders are the same sequence for every pixel unless tile rows overlap AND tile columns overlap (only then
    is a pixel under tiles (r, c'), (r', c) with r < r', c < c'): there the bits differ, elsewhere the mutant is the same function."""
    for Hh, W, T, ys, xs in R.GRIDS:
        n = len(ys) * len(xs)
        img = R.normal((2, 3, Hh, W), Hh * W)
        tiles = R.normal((n, 3, T, T), n + T)
        wy, wx = R.uniform((len(ys), T), 1, 0.05, 1.0), R.uniform((len(xs), T), 2, 0.05, 1.0)
        if len(ys) > 1 and len(xs) > 1:
            assert not np.array_equal(R.destitch(img, T, ys, xs), R.destitch(img, T, ys, xs, mutant="columns_first"))
        want, _, _ = R.restitch32(tiles, T, ys, xs, wy, wx, Hh, W)
        bad, _, _ = R.restitch32(tiles, T, ys, xs, wy, wx, Hh, W, mutant="columns_first")
        both = any(b - a < T for a, b in zip(ys, ys[1:])) and any(b - a < T for a, b in zip(xs, xs[1:]))
        assert np.array_equal(bad, want) != both, (Hh, W, ys, xs)
    assert sum(any(b - a < T for a, b in zip(ys, ys[1:])) and any(b - a < T for a, b in zip(xs, xs[1:])) for _, _, T, ys, xs in R.GRIDS) >= 2


# ---------------------------------------------------------------------------------------------------------------- sharpen
@pytest.mark.parametrize("Hh,W", [(1, 1), (2, 5), (3, 3), (3, 257), (17, 19)])
def test_sharpen_twin_is_adjust_sharpness(Hh, W):
    img = R.uniform((6, Hh, W), Hh + W, -1.5, 1.5)
    k = torch.ones(3, 3)
    k[1, 1] = 5.0
    k /= k.sum()
    assert float(k[0, 0]) == float(R.K1) and float(k[1, 1]) == float(R.K5)
    for s in (0.0, 0.5, 1.0, 2.5, -0.75):
        want, bound = R.sharpen(img, s)
        x64 = torch.from_numpy(img).double().reshape(2, 3, Hh, W)
        k64 = k.double()
        if Hh <= 2 or W <= 2:
            ref = x64
        else:                                                      # the restated adjust_sharpness with the float32 kernel's numbers
            v = x64.add(1).div(2)
            deg = v.clone()
            deg[..., 1:-1, 1:-1] = TF.conv2d(v.reshape(-1, 1, Hh, W), k64[None, None]).reshape(2, 3, Hh - 2, W - 2)
            ref = (float(F(s)) * v + (1.0 - float(F(s))) * deg).clamp(0, 1).mul(2).sub(1)
        assert np.abs(ref.numpy().reshape(6, Hh, W) - want).max() <= 1e-14
        f32 = H.sharpen(torch.from_numpy(img).reshape(2, 3, Hh, W), s).numpy().reshape(6, Hh, W)
        assert (np.abs(f32 - want) <= bound).all(), "the float32 restatement is inside the bound"
        if Hh > 2 and W > 2 and s != 1.0:
            assert rejected(R.sharpen(img, s, mutant="tap+1")[0], want, bound)


# ---------------------------------------------------------------------------------------------------------------- moments / match_apply
@pytest.mark.parametrize("HW", [1, 4095, 4096, 4097])
def test_moments_twin(HW):
    for navg in (1, 3):
        img = R.uniform((2 * navg, 3, HW), HW + navg, -1.2, 1.2)
        noise = R.normal((2, 3, HW), HW)
        part, bound = R.moments(img, navg, noise, 1e-3)
        v = img.astype(np.float64).reshape(2, navg, 3, HW).mean(1) + float(F(1e-3)) * noise.astype(np.float64)
        tot = part.sum(1)
        assert np.allclose(tot[:, :3], v.sum(-1), rtol=0, atol=1e-9)
        prods = np.stack([(v[:, a] * v[:, b]).sum(-1) for a, b in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))], 1)
        assert np.allclose(tot[:, 3:9], prods, rtol=0, atol=1e-9)
        assert np.array_equal(part[:, :, 9].min(1), img.reshape(2, -1).min(1)) and np.array_equal(part[:, :, 10].max(1), img.reshape(2, -1).max(1))
        assert (bound[..., :9] > 0).all() and (bound[..., 9:] == 0).all()
        # dropping the last pixel of the last slice (an off-by-one in the slice's end) is outside, or loses a whole slice
        if HW > 1:
            short, _ = R.moments(img[..., :HW - 1], navg, noise[..., :HW - 1], 1e-3)
            S = R.moments_slices(HW)
            assert short.shape[1] == S - 1 or rejected(short[:, S - 1, :9], part[:, S - 1, :9], bound[:, S - 1, :9])


def test_match_apply_twin():
    for HW in (1, 257):
        img, noise, prior = R.normal((3, HW), HW), R.normal((3, HW), HW + 1), R.normal((3, HW), HW + 2)
        m, mu_t, mu_s = R.normal((9,), 4), R.normal((3,), 5), R.normal((3,), 6)
        want, bound = R.match_apply(img, noise, 1e-3, m, mu_t, mu_s, 0.5, prior, 1, -0.4, 0.6)
        x = torch.from_numpy(img).double() + float(F(1e-3)) * torch.from_numpy(noise).double() - torch.from_numpy(mu_t).double()[:, None]
        ref = (0.5 * (torch.from_numpy(m).double().reshape(3, 3) @ x + torch.from_numpy(mu_s).double()[:, None]) + torch.from_numpy(prior).double())
        ref = ref.clamp(float(F(-0.4)), float(F(0.6))).numpy()
        assert np.abs(ref - want).max() <= 1e-14
        free, bound_free = R.match_apply(img, noise, 1e-3, m, mu_t, mu_s, 0.5, None, 0, 0, 0)
        assert rejected(R.match_apply(img, noise, 1e-3, m, mu_t, mu_s, 0.5, None, 0, 0, 0, mutant="transposed")[0], free, bound_free)


# ---------------------------------------------------------------------------------------------------------------- perlin
def test_perlin_restatement_reproduces_the_reference_bit_for_bit(g37):
    for name in ("pc", "pg"):
        m = g37["meta"][name]
        grads = [g37[f"{name}_grad{k:02d}"].numpy() for k in range(m["n_grads"])]
        octs = list(g37[f"{name}_octaves"].numpy())
        n = len(octs)
        for k, g in enumerate(grads):                             # preconditions of the exact family, per input
            assert g.dtype == F and g.shape == (2, (m["width"] << (k % n)) + 1, (m["height"] << (k % n)) + 1)
        assert all(float(F(o)) == float(torch.tensor(o, dtype=torch.float32)) for o in octs)
        got = R.perlin32(grads, octs, m["width"], m["height"], m["grayscale"])
        want_raw = g37[f"{name}_raw"].numpy().reshape(got["raw"].shape)
        assert want_raw.dtype == F and np.array_equal(got["raw"], want_raw), "perlin_ms, bit for bit"
        assert np.array_equal(got["out"], g37[f"{name}_img"].numpy()), "to_pil_image, autocontrast, to_tensor, bit for bit"
        assert np.array_equal(got["out"], H.perlin_image(torch.from_numpy(want_raw.reshape(-1, want_raw.shape[-1])), m["grayscale"]).numpy())
        bad = R.perlin32(grads, octs, m["width"], m["height"], m["grayscale"], mutant="corner")
        assert not np.array_equal(bad["raw"], got["raw"])
    g = g37["perlin_single_grad"].numpy()
    assert np.array_equal(R.perlin_at32(g, 4), g37["perlin_single"].numpy())
    for scale in (1, 2, 16):                                       # a / scale is torch.linspace(0, 1, scale + 1)[:-1], exactly
        assert np.array_equal((np.arange(scale).astype(F) / F(scale)), torch.linspace(0, 1, scale + 1)[:-1].numpy())


def test_perlin_cases_of_the_gpu_file():
    """the GPU file's own shapes: a flat channel gives the identity table and byte 127; a mutant corner index moves bits at every shape"""
    for width, height, n in ((1, 1, 1), (2, 3, 3), (3, 2, 4)):
        grads = [R.normal((2, (width << k) + 1, (height << k) + 1), 7 * width + n + k) for k in range(n)]
        octs = [1.0, 0.5, 0.3, 0.7][:n]
        a = R.perlin32(grads, octs, width, height, True)
        assert a["raw"].dtype == F and a["out"].shape == (3, width << n, height << n)
        assert not np.array_equal(a["raw"], R.perlin32(grads, octs, width, height, True, mutant="corner")["raw"])
        flat = R.perlin32([np.zeros_like(g) for g in grads], octs, width, height, True)
        assert (flat["q"] == 127).all() and (flat["lut"][0] == np.arange(256)).all()


# ---------------------------------------------------------------------------------------------------------------- pad, conv1d_reflect
PAD_NAME = {R.PAD_CONSTANT: "constant", R.PAD_REFLECT: "reflect", R.PAD_REPLICATE: "replicate", R.PAD_CIRCULAR: "circular"}


def test_pad_twin_is_torch_pad():
    for Hh, W, oh, ow, pl, pt, hows in R.PAD_CASES:
        x = R.normal((2, 3, Hh, W), Hh * W + oh)
        pr, pb = ow - W - pl, oh - Hh - pt
        for how in hows or PAD_NAME:
            got = R.pad2d(x, oh, ow, pl, pt, how, F(-0.3))
            if how == R.PAD_CIRCULAR and max(pl, pr) > W or how == R.PAD_CIRCULAR and max(pt, pb) > Hh:
                with pytest.raises(RuntimeError):                  # torch refuses a wrap of more than once; the library wraps again
                    TF.pad(torch.from_numpy(x), (pl, pr, pt, pb), mode="circular")
                want = np.tile(x, (1, 1, 7, 3))[..., (-pt) % Hh:, (-pl) % W:][..., :oh, :ow]
            elif how == R.PAD_CONSTANT:
                want = TF.pad(torch.from_numpy(x), (pl, pr, pt, pb), mode="constant", value=float(F(-0.3))).numpy()
            else:                                                   # pad the positive sides, then crop the negative ones
                want = TF.pad(torch.from_numpy(x), (max(pl, 0), max(pr, 0), max(pt, 0), max(pb, 0)), mode=PAD_NAME[how]).numpy()
                want = want[..., max(-pt, 0):want.shape[-2] - max(-pb, 0), max(-pl, 0):want.shape[-1] - max(-pr, 0)]
            assert np.array_equal(got, want), (Hh, W, oh, ow, pl, pt, how)
        if hows is None and pl > 0:
            assert not np.array_equal(R.pad2d(x, oh, ow, pl, pt, R.PAD_REFLECT, 0, mutant="period_2n"), R.pad2d(x, oh, ow, pl, pt, R.PAD_REFLECT, 0))


def test_conv1d_twin_is_conv2d_on_a_reflect_padded_input_and_its_autograd():
    for planes, Hh, W in R.CONV_SHAPES:
        x, dy = R.normal((planes, Hh, W), Hh + W), R.normal((planes, Hh, W), Hh * W)
        for axis in (0, 1):
            n = (Hh, W)[axis]
            for radius in sorted({0, 1, n - 1} & set(range(n))):
                taps = R.normal((2 * radius + 1,), radius + n)
                want, bound = R.conv1d_reflect(x, taps, axis)
                xt = torch.from_numpy(x).double()[None].requires_grad_()
                pad = (0, 0, radius, radius) if axis == 0 else (radius, radius, 0, 0)
                k = torch.from_numpy(taps).double().reshape((1, 1, -1, 1) if axis == 0 else (1, 1, 1, -1)).expand(planes, 1, -1, -1)
                y = TF.conv2d(TF.pad(xt, pad, mode="reflect") if radius else xt, k, groups=planes)
                assert np.abs(y.detach().numpy()[0] - want).max() <= 1e-12
                gx, = torch.autograd.grad(y, xt, torch.from_numpy(dy).double()[None])
                adj, badj = R.conv1d_reflect(dy, taps, axis, vjp=True)
                assert np.abs(gx.numpy()[0] - adj).max() <= 1e-12
                if radius:
                    for mutant in ("tap+1", "period_2n"):
                        assert rejected(R.conv1d_reflect(x, taps, axis, mutant=mutant)[0], want, bound), (mutant, planes, Hh, W, axis, radius)
                        assert rejected(R.conv1d_reflect(dy, taps, axis, vjp=True, mutant=mutant)[0], adj, badj)


def test_grad_accumulate_twin():
    s, a = R.normal((5,), 1), R.normal((5,), 2)
    assert np.array_equal(R.grad_accumulate32(s, a, 1), s) and np.array_equal(R.grad_accumulate32(s, a, 0), a + s)
    s[2] = np.nan
    assert np.array_equal(R.grad_accumulate32(s, a, 1), np.zeros(5, F)) and np.array_equal(R.grad_accumulate32(s, a, 0), a)
    s[2] = np.inf
    assert R.grad_accumulate32(s, a, 0)[2] == np.inf


# ---------------------------------------------------------------------------------------------------------------- bicubic and its vjp
@pytest.mark.parametrize("Hh,W,oh,ow", R.BICUBIC_SHAPES + R.BICUBIC_VJP_EXTRA)
def test_bicubic_twin_is_interpolate_and_its_autograd(Hh, W, oh, ow):
    x, g = R.normal((2, 3, Hh, W), Hh * W + ow), R.normal((2, 3, oh, ow), Hh * W + oh)
    for align in (False, True):
        want, bound = R.bicubic(x, oh, ow, align)
        xt = torch.from_numpy(x).double().requires_grad_()
        y = TF.interpolate(xt, (oh, ow), mode="bicubic", align_corners=align)
        # torch in float64 takes the source coordinate in float64: the twin's float32 coordinate is within the bound's coordinate term
        assert (np.abs(y.detach().numpy() - want) <= bound).all()
        y32 = TF.interpolate(torch.from_numpy(x), (oh, ow), mode="bicubic", align_corners=align).numpy()
        assert (np.abs(y32 - want) <= bound).all(), "ATen's float32 kernel is inside the bound"
        adj, badj = R.bicubic_vjp(g, Hh, W, align)
        ref, = torch.autograd.grad(y, xt, torch.from_numpy(g).double())
        assert (np.abs(ref.numpy() - adj) <= badj).all()
        assert np.abs(ref.numpy() - adj).max() <= 1e-4 * max(np.abs(adj).max(), 1e-30)


def test_bicubic_mutants_are_rejected_at_the_gpu_shapes():
    """a mutant is rejected wherever it computes another function: at some shapes it does not (one output from the middle of the image
    reaches no border; an identity resize gives the clamped taps weight 0; the 8-fold reduction's last taps stop short of the last
    sample), and every mutant is rejected at one shape at least, for both align_corners"""
    seen = {}
    for Hh, W, oh, ow in R.BICUBIC_SHAPES:
        x, g = R.normal((2, 3, Hh, W), Hh * W + ow), R.normal((2, 3, oh, ow), Hh * W + oh)
        for align in (False, True):
            want, bound = R.bicubic(x, oh, ow, align)
            for mutant in ("tap+1", "tap-1", "clamp_n"):
                bad = R.bicubic(x, oh, ow, align, mutant=mutant)[0]
                hit = rejected(bad, want, bound)
                assert hit or np.array_equal(bad, want), (mutant, align, Hh, W, oh, ow)
                seen[mutant, align] = seen.get((mutant, align), 0) + hit
            adj, badj = R.bicubic_vjp(g, Hh, W, align)
            bad = R.bicubic_vjp(g, Hh, W, align, mutant="no_clamped_taps")[0]
            hit = rejected(bad, adj, badj)
            assert hit or np.array_equal(bad, adj)
            seen["no_clamped_taps", align] = seen.get(("no_clamped_taps", align), 0) + hit
    assert all(v >= 2 for v in seen.values()), seen


def test_bicubic_coordinate_term_dominates_when_wide():
    """at 515 -> 1029 samples the source coordinate's float32 rounding (2 ulp of up to 515) outweighs the arithmetic: what held the old
    2e-6 test to sizes up to 32"""
    x = R.normal((1, 1, 3, 515), 1)
    _, wide = R.bicubic(x, 2, 1029, False)
    _, small = R.bicubic(x[..., :32], 2, 64, False)
    assert wide.max() > 8 * small.max()


# ---------------------------------------------------------------------------------------------------------------- cutouts
def ulp_distance(a, b):
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)))
    return np.abs(ia - ib)


@pytest.mark.parametrize("cs", [8, 32])
def test_cutout_tables_are_the_oracles(cs):
    """left() and the tap count exactly.  The weights exactly with four taps; with more the oracle's `w.sum(1)` is torch's vectorised
    reduction, whose order is not defined element by element - the kernel and the twin add the taps in order, and the normalised weights
    then sit within the two orders' distance of the oracle's (3 ulp at most over these sizes)."""
    from oracle import clip as OC
    for size in range(1, 4 * cs):
        left, w = R.cutout_tables32(size, cs)
        l2, w2 = OC.resize_tables(size, cs)
        assert np.array_equal(left, l2.numpy()) and w.shape == tuple(w2.shape), size
        if w.shape[1] <= 4:
            assert np.array_equal(w, w2.numpy()), size
        else:                     # two orders of one sum differ by at most 2 (taps - 1) u sum |w| of it; the division adds a rounding each
            tol = (2 * (w.shape[1] - 1) * np.abs(w).sum(1, keepdims=True, dtype=np.float64) + 2) * R.U * np.abs(w)
            assert (np.abs(w.astype(np.float64) - w2.numpy()) <= tol).all() and ulp_distance(w, w2.numpy()).max() <= 8, size
        assert not np.array_equal(R.cutout_tables32(size, cs, mutant="left_floor")[0], left)
    assert np.array_equal(R.cutout_matrix(cs, cs)[0], np.eye(cs))                    # size == cut size: weights 0, 0, 1, 0


@pytest.mark.parametrize("cs", [8, 32])
def test_cutouts_twin_is_the_oracle_and_its_autograd(cs, golden):
    from oracle import clip as OC
    from oracle import grads as OG
    for Hh, W in R.CUTOUT_IMAGES[cs]:
        rects = R.cutout_rects(cs, Hh, W)
        for rs, top, left in rects:                                                 # the GPU test's rectangles are legal
            size = rs & R.CUT_SIZE_MASK
            assert 1 <= size <= 4 * cs - 1 and top >= 0 and left >= 0 and top + size <= Hh and left + size <= W
        sizes = {r[0] & R.CUT_SIZE_MASK for r in rects}
        assert {1, min(Hh, W, 4 * cs - 1)} <= sizes and {r[0] >> 29 for r in rects} == {0, 1, 2, 3}
        assert any(t + (s & R.CUT_SIZE_MASK) == Hh and l + (s & R.CUT_SIZE_MASK) == W for s, t, l in rects)
        img = R.uniform((2, 3, Hh, W), Hh + cs, -1.1, 1.1)
        d_out = R.normal((len(rects) * 2, 3, cs, cs), W + cs)
        want, bound = R.cutouts(img, rects, cs, 0.5, 0.5, (0, 0, 0), (1, 1, 1))
        xt = torch.from_numpy(img).double().requires_grad_()
        outs = []
        for rs, top, left in rects:                                                 # the oracle per rectangle, with DangoCutouts' grey and flip
            size = rs & R.CUT_SIZE_MASK
            c = xt.add(1).div(2)[:, :, top:top + size, left:left + size]
            if rs & R.CUT_GREY:
                c = OG.grayscale3(c)
            o = OC.resize(c, (cs, cs))
            outs.append(o.flip(-1) if rs & R.CUT_FLIP else o)
        y = torch.cat(outs)
        # (the oracle's weights sit up to 2 ulp from the sequentially summed ones, twice: 8 u of the largest magnitude, ~1.5 with overshoot)
        assert np.abs(y.detach().numpy() - want).max() <= 8 * R.U * 1.5
        adj, badj = R.cutouts_vjp(d_out, 2, Hh, W, rects, cs, 0.5, (1, 1, 1))
        ref, = torch.autograd.grad(y, xt, torch.from_numpy(d_out).double())
        assert np.abs(ref.numpy() - adj).max() <= 1e-5 * np.abs(adj).max()
        for mutant in ("left_floor", "grey_one_plane", "no_flip"):
            assert rejected(R.cutouts(img, rects, cs, 0.5, 0.5, (0, 0, 0), (1, 1, 1), mutant=mutant)[0], want, bound), mutant
        for mutant in ("store_only_flip", "grey_one_plane"):
            assert rejected(R.cutouts_vjp(d_out, 2, Hh, W, rects, cs, 0.5, (1, 1, 1), mutant=mutant)[0], adj, badj), mutant
    if cs == 32:                                                                     # the reference's own outputs (g33)
        g = golden("g33_cutouts")
        for k in (0, 1, 2, 4):
            rects = [tuple(int(v) for v in r) for r in g[f"cut{k}_rects"].numpy()]
            out, bound = R.cutouts(g[f"cut{k}_img"].numpy(), rects, 32, 1.0, 0.0, (0, 0, 0), (1, 1, 1))
            assert np.abs(out - g[f"cut{k}_out"].numpy()).max() <= 1e-6


def test_grayscale_of_the_oracle_is_the_twins_luma():
    from oracle import grads as OG
    x = torch.rand(1, 3, 4, 4, dtype=torch.float64)
    lum = sum(float(c) * x[:, k] for k, c in enumerate(R.LUMA))
    assert float((OG.grayscale3(x)[:, 0] - lum).abs().max()) <= 1e-7             # (0.2989, 0.587, 0.114 as float32 numbers against doubles)


# ---------------------------------------------------------------------------------------------------------------- colour match
def test_colormatch_odd_bin_count():
    odd = R.cm_odd_nbins()
    assert odd[0] == 42 and len(odd) == 137
    assert F(41) * F(1.0 / 41) != F(1) and all(F(n - 1) * F(1.0 / (n - 1)) == F(1) for n in R.CM_NBINS)


@pytest.mark.parametrize("nbins", R.CM_NBINS + (42,))
def test_colormatch_twin_is_the_oracle(nbins):
    from oracle import grads as OG
    img = R.cm_random_image()
    t4 = torch.from_numpy(img).reshape(3, 3, 37, 53)
    assert np.array_equal(R.cm_edges32(nbins)[:nbins + 1], OG.histogram_bins(nbins).numpy())
    for sat in (1, 0):
        fix = R.cm_hist_fix(img, nbins, sat)
        assert int(fix.max()) < 2 ** 63
        Hn = R.cm_final32(fix)[2]
        ref = OG.colormatch_histogram(t4.double(), bool(sat), nbins).numpy()
        assert np.abs(Hn - ref).max() <= 1e-6
        h = R.cm_pixel32(img[0, 0], img[0, 1], img[0, 2], bool(sat))
        hsv = OG.rgb_to_hsv(t4[:1].add(1).div(2).clamp(1e-8, 1 - 1e-8)).clamp(0, 1).reshape(3, -1).numpy()
        assert np.array_equal(h["x"], hsv[0]) and np.array_equal(h["sc"], hsv[1]) and np.array_equal(h["vc"], hsv[2]), "the float32 pixel chain, bit for bit"
        Hn64 = Hn.astype(np.float64)
        bound = (-(-nbins // 256) + 11) * R.U * Hn64
        for mutant in ("bins_swapped", "delta_nbins"):
            bad = R.cm_final32(R.cm_hist_fix(img, nbins, sat, mutant=mutant))[2]
            assert rejected(bad, Hn64, bound), mutant
        target = R.cm_target(nbins, sat, 1)
        grad, gb, loss, _ = R.cm_grad(img, nbins, sat, target[0], 1000.0)
        ref, lref = OG.colormatch_grads(t4.double(), torch.from_numpy(target).double(), 1000.0, bool(sat), nbins)
        ref = ref.numpy().reshape(3, 3, -1)
        ok = ~np.isnan(ref)                                        # the reference's autograd gives NaN at weight 0 (sqrt'), the kernel and the twin none
        # (the oracle's float64 hue against the float32 hue the kernel and the twin share: u of a hue, relative to a bin 1 / (nbins - 1) wide)
        assert np.abs(grad - ref)[ok].max() <= (2e-5 + 4 * nbins * R.U) * np.abs(grad).max() and abs(loss.sum() - float(lref)) <= 1e-5 * float(lref)
        assert (gb[ok] >= 0).all() and (gb[np.abs(grad) > 0] > 0).all()


@pytest.mark.parametrize("nbins", R.CM_NBINS + (42,))
def test_colormatch_special_pixels(nbins):
    px, tags = R.cm_special_pixels(nbins)
    h = R.cm_pixel32(px[:, 0], px[:, 1], px[:, 2], True)
    at = {t: i for i, t in enumerate(tags)}
    assert h["delta"][at["grey"]] == 0 and h["w"][at["grey"]] == 0
    assert [int(h["im"][at[t]]) for t in ("red max", "green max", "blue max", "tie r g", "tie g b", "tie r b", "tie of three at 1")] == [0, 1, 2, 0, 1, 0, 0]
    assert int(h["imin"][at["min tie"]]) == 1
    assert not h["live"][:, at["below -1 and above 1"]][[0, 2]].any() and h["live"][:, at["exactly -1 and 1"]].tolist() == [False, True, True]
    assert h["live"][0, at["u = 2^-25"]] and not h["live"][0, at["u = 0"]]
    assert h["hue_raw"][at["q tiny negative (1 steps)"]] == R.TWO_PI32 and h["x"][at["hue above one radian"]] == 1
    edges = R.cm_edges32(nbins)
    on_edge = [t for t in tags if t.startswith("hue on edge")]
    assert (len(on_edge) > 0) == (nbins > 2)
    for t in on_edge:
        assert h["x"][at[t]] == edges[int(t.split()[-1])]
    for sat in (1, 0):
        img = px.reshape(-1, 3, 1)
        fix = R.cm_hist_fix(img, nbins, sat)
        assert ((fix > 0).sum(1) <= 2).all()
        good = R.cm_final32(fix)[2]
        for mutant in ("bins_swapped", "delta_nbins"):
            bad = R.cm_final32(R.cm_hist_fix(img, nbins, sat, mutant=mutant))[2]
            assert not np.array_equal(bad, good, equal_nan=True), mutant


def test_colormatch_all_grey_is_nan_in_the_reference_too():
    from oracle import grads as OG
    img = np.repeat(R.uniform((2, 1, 35), 3), 3, 1)
    ref = OG.colormatch_histogram(torch.from_numpy(img).reshape(2, 3, 5, 7), True, 64).numpy()
    assert np.isnan(ref).all() and np.isnan(R.cm_final32(R.cm_hist_fix(img, 64, 1))[2]).all()
    g, _ = OG.colormatch_grads(torch.from_numpy(img).reshape(2, 3, 5, 7), torch.full((1, 64), 1 / 64), 1.0, True, 64)
    twin = R.cm_grad(img, 64, 1, np.full(64, 1 / 64, F), 1.0)[0]
    assert np.isnan(g.numpy()).any() and np.isnan(twin).any()


# ---------------------------------------------------------------------------------------------------------------- the reference's own outputs (g34)
def test_colormatch_twin_against_the_reference_class(golden):
    """g34: ColorMatchGrads' own histograms and gradients (255 bins, scale 3, the style image's histogram as the shared target)"""
    g = golden("g34_grads")
    img = g["cm_img"].numpy()
    B, _, Hh, W = img.shape
    flat = img.reshape(B, 3, Hh * W)
    for sw in (1, 0):
        hist = R.cm_final32(R.cm_hist_fix(flat, 255, sw))[2]
        assert np.abs(hist - g[f"cm_hist_{sw}"].numpy()).max() <= 2e-7            # (the bar of tests/test_oracle_grads.py)
        style = g["cm_style"].numpy()
        target = R.cm_final32(R.cm_hist_fix(style.reshape(1, 3, -1), 255, sw))[2]
        assert np.abs(target - g[f"cm_target_{sw}"].numpy()).max() <= 2e-7
        grad, _, _, _ = R.cm_grad(flat, 255, sw, g[f"cm_target_{sw}"].numpy()[0], 3.0)
        want = g[f"cm_grad_{sw}"].numpy().reshape(B, 3, -1)
        ok = ~np.isnan(want)                                                       # (the reference's NaN at weight 0: the twin has none there)
        assert ok.mean() > 0.9 and np.abs(grad - want)[ok].max() <= 1e-5 * np.abs(want[ok]).max() + 1e-12


def dango_rects(plan, side):
    return [((side if size < 0 else size) | (R.CUT_GREY if grey else 0) | (R.CUT_FLIP if flip else 0), top, left) for size, top, left, grey, flip in plan]


def test_cutouts_twin_against_dango_cutouts_and_cutouts_from_rects(golden):
    """oracle/grads.py dango_cutouts on g34's plans (and the reference's outputs), oracle/clip.py cutouts_from_rects on g34's "normal"
    rectangles: the overview cutouts are the reflect-padded square as one rectangle with the grey and mirror flags, the inner crops
    rectangles of the input with the grey flag"""
    from maua_amd.grad import Cutouts
    from oracle import clip as OC
    from oracle import grads as OG
    g = golden("g34_grads")
    ident = (1.0, 0.0, (0, 0, 0), (1, 1, 1))
    for k in range(3):
        Hh, W, cs, _t, seed, overview, inner = (int(v) for v in g[f"dango{k}_cfg"])
        torch.manual_seed(seed)
        plan = OG.dango_plan(Hh, W, cs, overview, inner, float(g[f"dango{k}_grey_p"]))
        img = g[f"dango{k}_img"]
        ref = OG.dango_cutouts(img.double(), plan, cs, OC.resize).numpy()
        side = min(Hh, W)
        pad = ((Hh - side) // 2, (Hh - side) // 2, (W - side) // 2, (W - side) // 2)
        square = TF.pad(img, pad, mode="reflect").numpy() if any(pad) else img.numpy()
        parts = []
        for entry in plan:                                         # one rectangle at a time: the overview reads the padded square
            src = square if entry[0] < 0 else img.numpy()
            parts.append(R.cutouts(src, dango_rects([entry], square.shape[-1]), cs, *ident)[0])
        got = np.concatenate(parts)
        # (the oracle's weights sit up to 3 ulp from the in-order sum, twice; magnitudes up to ~1.5 with the cubic's overshoot)
        assert got.shape == ref.shape and np.abs(got - ref).max() <= 12 * R.U * 1.5, k
        assert np.abs(got - g[f"dango{k}_out"].numpy()).max() <= 1e-6, k
    for k in range(2):
        S, cs, cutn, seed = (int(v) for v in g[f"normal{k}_cfg"])
        p = Cutouts(cs, cutn, skip_augs=True).pad_of(S)
        rects = [tuple(int(v) for v in r) for r in g[f"normal{k}_rects"].numpy()]
        padded = TF.pad(torch.rand(1, 3, S, S, generator=torch.Generator().manual_seed(350 + k)), (p,) * 4)
        ref = OC.cutouts_from_rects(padded.double(), rects, cs).numpy()
        if max(r[0] for r in rects) <= 4 * cs - 1:
            got = R.cutouts(padded.numpy(), rects, cs, *ident)[0]
            assert np.abs(got - ref).max() <= 12 * R.U * 1.5 and np.abs(got - g[f"normal{k}_out"].numpy()).max() <= 1e-6, k
