"""The Farneback estimator's kernels (csrc/flow.hip: fb_gray, fb_blur<0 / 1>, fb_resize, fb_poly_v, fb_poly_h, fb_matrices, fb_iterate),
launched through maua_farneback_pair_ex with the level range, the iteration count, the entering flow and the dumps chosen here, stage
by stage against the float64 restatement tests/flow_ref.py.  The method of tests/test_gpu_groupnorm.py: every device buffer between
guard regions (NaN around the inputs, a sentinel pattern around the outputs and dumps: the guards must be intact afterwards and every
element of the body written), exact families compared with torch.equal, and derived element-wise bounds elsewhere.

Each stage is judged on the input the device gave it: the float64 reference of stage k runs on the device's dump of stage k - 1, so
an error belongs to one kernel and the bound is that kernel's own float32 rounding (V = 2^-24 per rounding; a float32 sum of n products,
in any order and contracted or not, lies within n V sum|terms| of exact).  The derivations are with the functions that compute them
(flow_ref.pyr_blur, fb_resize_bound, poly_exp_bound, update_matrices, blur_solve); tests/test_farneback_host.py proves on the CPU that
the float32 restatement stays inside every one of them on the inputs used here.  No further margin.

    gray        torch.equal: the same sequence of correctly rounded float32 operations on both sides (no contraction: a planted pixel
                tells); nothing excluded
    blur        n taps: n V sum|terms| a pass, chained through the two passes
    resize      3 V sum|terms| each way (the rounded weight 1 - t, two products, one sum); level 0 is the identity, bit-equal
    expansion   9 V sum|terms| a pass (8 terms tap * (left +- right)), then the one- and two-term combinations
    matrices    the expression tree's operation count on the absolute intermediate terms, at every pixel: the positions (float)x + dx and
                their floors are exact float32 on both sides, so the reference takes the device's branch everywhere
    iteration   box mean 31 V mean|M_c|, carried through det = g0 g2 - g1^2 + 1e-3 and the numerators; a pixel with E_det >= det / 2 has
                no bound and is left out (at most 0.5 %; none on these inputs)
    upsample    the resize bound and one rounding for the factor (float)(1 / 0.8)

Worst error / bound seen on one MI355X: see DESIGN 5e (test_zz_report prints them)."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flow_ref as FR  # noqa: E402
from test_farneback_host import (BLUR_CASES, CHAIN_INPUTS, CHAIN_SIZES, GRAY_SIZES, ITER_SIZES, MAT_SIZES, POLY_SIZES, RESIZE_CASES,  # noqa: E402
                                 SPREAD_LIMIT, UPSAMPLE, chain_references, stage_pair)

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENT = 0x5A5A5A5A
G = 1024                                            # guard elements on either side of every buffer
MAX_H, MAX_W = 123, 160                             # the one handle every test but the reuse test runs on
WORST = {}                                          # family -> worst error / bound seen (test_zz_report prints it)
_handles = {}


class Buf:
    """A float32 device buffer of ``shape`` between guard regions.  Inputs (data given): NaN in the guards.  Outputs: a sentinel bit
    pattern everywhere; check() wants the guards intact and every element of the body written."""

    def __init__(self, shape, data=None):
        self.shape = tuple(shape)
        self.n = int(torch.Size(self.shape).numel())
        self.full = torch.empty((2 * G + self.n,), dtype=torch.float32, device=DEV)
        if data is None:
            self.full.view(torch.int32).fill_(SENT)
        else:
            self.full.fill_(float("nan"))
            self.full[G:G + self.n] = torch.as_tensor(data, dtype=torch.float32).reshape(-1).to(DEV)
        self.t = self.full[G:G + self.n].view(self.shape)
        self.ptr = self.t.data_ptr()

    def get(self):
        return self.t.cpu()

    def check(self, what):
        b = self.full.view(torch.int32)
        assert bool((b[:G] == SENT).all()) and bool((b[G + self.n:] == SENT).all()), f"{what}: a store outside the buffer"
        assert bool((b[G:G + self.n] != SENT).all()), f"{what}: elements of the result were never written"
        assert not bool(torch.isnan(self.t).any()), f"{what}: NaN in the result (a guard was read)"


def handle(max_h=MAX_H, max_w=MAX_W):
    import maua_amd.flow as F
    if (max_h, max_w) not in _handles:
        _handles[max_h, max_w] = F.Farneback(max_h, max_w)
    return _handles[max_h, max_w]


def run(a, b, level_hi=-1, level_lo=-1, iterations=0, init=None, dumps=(), fb=None):
    """One guarded maua_farneback_pair_ex -> dict of CPU tensors: flow [2, h, w, 2] (a -> b, b -> a) and the dumps asked for."""
    import maua_amd.flow as F
    H, W = int(a.shape[-2]), int(a.shape[-1])
    top = F.farneback_levels(H, W) - 1
    h, w = F.farneback_level_size(H, W, 0 if level_lo < 0 else level_lo)
    shapes = dict(gray=(2, H, W), blur=(2, H, W), level=(2, h, w), coef=(2, 5, h, w), flow_in=(2, h, w, 2), mat=(2, 5, h, w))
    ia, ib = Buf(a.shape, a), Buf(b.shape, b)
    out = {"ab": Buf((h, w, 2)), "ba": Buf((h, w, 2))}
    out.update({k: Buf(shapes[k]) for k in dumps})
    ini = None
    if init is not None:
        assert tuple(init.shape) == (2, *F.farneback_level_size(H, W, top if level_hi < 0 else level_hi), 2)
        ini = (Buf(init[0].shape, init[0]), Buf(init[1].shape, init[1]))
    (fb or handle()).pair_ex(ia.ptr, ib.ptr, H, W, out["ab"].ptr, out["ba"].ptr, level_hi, level_lo, iterations,
                             ini and ini[0].ptr, ini and ini[1].ptr, **{k: out[k].ptr for k in dumps})
    torch.cuda.synchronize()
    for k, v in out.items():
        v.check(f"{k} of {W}x{H} levels {level_hi}..{level_lo}")
    res = {k: out[k].get() for k in dumps}
    res["flow"] = torch.stack([out["ab"].get(), out["ba"].get()])
    return res


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))
    return ratio


# ------------------------------------------------------------------------------------------------------------------ stage by stage
@pytest.mark.parametrize("rows,cols", GRAY_SIZES)
def test_gray_is_exact(rows, cols):
    a, b, planted = FR.gray_images(rows, cols)
    d = run(a, b, 0, 0, 1, dumps=("gray",))
    want = torch.stack([FR.to_gray_u8(a), FR.to_gray_u8(b)])
    for x, kind, value in planted:
        assert float(d["gray"][0, 0, x]) == value, (x, kind)
    assert torch.equal(d["gray"], want)
    assert float(want.min()) == 0 and float(want.max()) == 255


@pytest.mark.parametrize("rows,cols,k", BLUR_CASES)
def test_blur(rows, cols, k):
    d = run(*stage_pair(rows, cols), k, k, 1, dumps=("gray", "blur"))
    r = note("blur", FR.check_blur(d, k))
    print(f"blur {cols}x{rows} level {k} ({FR.level_taps(k).shape[0]} taps): worst error / bound {r:.3f}")
    assert r <= 1


@pytest.mark.parametrize("rows,cols,k", RESIZE_CASES)
def test_resize(rows, cols, k):
    d = run(*stage_pair(rows, cols), k, k, 1, dumps=("blur", "level"))
    assert tuple(d["level"].shape) == (2, *FR.level_size(rows, cols, k))
    r = note("resize", FR.check_resize(d))
    print(f"resize {cols}x{rows} level {k} -> {tuple(d['level'].shape[1:])}: worst error / bound {r:.3f}")
    assert r <= 1
    if k == 0:
        assert torch.equal(d["level"], d["blur"])


@pytest.mark.parametrize("rows,cols", POLY_SIZES)
def test_polynomial_expansion(rows, cols):
    d = run(*stage_pair(rows, cols), 0, 0, 1, dumps=("level", "coef"))
    r = note("expansion", FR.check_poly(d))
    print(f"polynomial expansion {cols}x{rows}: worst error / bound {r:.3f}")
    assert r <= 1


@pytest.mark.parametrize("rows,cols", MAT_SIZES)
def test_matrices(rows, cols):
    """Constructed entering flows (about a third of the pixels sample outside the frame, the planted pixels sit on the predicate's edges,
    a few flows are +- 10 w): every pixel of both directions inside the bound of the branch the float32 positions take."""
    flows, planted = FR.matrices_flows(rows, cols)
    d = run(*stage_pair(rows, cols), 0, 0, 1, init=flows, dumps=("coef", "flow_in", "mat"))
    assert torch.equal(d["flow_in"], flows)
    r, inside = FR.check_matrices(d)
    ref = [FR.update_matrices(d["coef"][i].double(), d["coef"][1 - i].double(), flows[i], True) for i in range(2)]
    for i, y, x, want in planted:
        assert bool(inside[i, y, x]) == want
        assert bool(((d["mat"][i, :, y, x].double() - ref[i][0][:, y, x]).abs() <= ref[i][1][:, y, x]).all()), (i, y, x, want)
    note("matrices", r)
    print(f"matrices {cols}x{rows}: worst error / bound {r:.3f}, outside the frame {1 - float(inside.float().mean()):.3f}")
    assert r <= 1


@pytest.mark.parametrize("rows,cols", ITER_SIZES)
def test_one_and_two_iterations(rows, cols):
    """iterations = 1: the LDS tile, the box mean and the solve against the matrices dump.  iterations = 2: the update branch and the
    second matrix buffer - the matrices of the one-iteration device flow (a rerun is bit-identical, so that flow is the second run's
    intermediate), then the box mean and the solve, the two bounds composed."""
    a, b = stage_pair(rows, cols)
    d1 = run(a, b, 0, 0, 1, dumps=("coef", "mat"))
    r1, out1 = FR.check_iteration(d1)
    d2 = run(a, b, 0, 0, 2, dumps=("coef", "mat"))
    assert torch.equal(d2["coef"], d1["coef"]) and torch.equal(d2["mat"], d1["mat"])
    r2, out2 = FR.check_second_iteration(d1, d2)
    note("one iteration", r1)
    note("two iterations", r2)
    print(f"iterations {cols}x{rows}: one {r1:.3f} ({out1:.4f} left out), two {r2:.3f} ({out2:.4f} left out)")
    assert out1 <= 0.005 and out2 <= 0.005
    assert r1 <= 1 and r2 <= 1
    assert not torch.equal(d1["flow"], d2["flow"])


def test_flow_upsample():
    rows, cols, k = UPSAMPLE
    a, b = stage_pair(rows, cols)
    top = run(a, b, k, k)["flow"]
    d = run(a, b, k, k - 1, dumps=("flow_in",))
    h, w = FR.level_size(rows, cols, k - 1)
    assert tuple(d["flow_in"].shape) == (2, h, w, 2) and float(top.abs().max()) > 0.5
    r = note("upsample", FR.check_upsample(top, d["flow_in"], h, w))
    print(f"flow upsample {cols}x{rows} level {k} -> {k - 1}: worst error / bound {r:.3f}")
    assert r <= 1


# ------------------------------------------------------------------------------------------------------------------ exact properties
def test_directions_swap_with_the_images():
    """grid z only swaps which image's coefficients are the first"""
    a, b = stage_pair(45, 40)
    f, g = run(a, b)["flow"], run(b, a)["flow"]
    assert torch.equal(f[1], g[0]) and torch.equal(f[0], g[1]) and not torch.equal(f[0], f[1])


def test_default_descriptor_is_the_plain_entry_point():
    rows, cols = 47, 40
    a, b = stage_pair(rows, cols)
    ab, ba = handle().pair(a, b)
    f = run(a, b)["flow"]
    assert torch.equal(ab[0].cpu(), f[0]) and torch.equal(ba[0].cpu(), f[1])
    assert torch.equal(run(a, b, 1, 0, 15)["flow"], f)


def test_a_run_split_in_two_is_the_whole_run():
    """levels 2 .. 1, whose dump is the flow entering level 1; then levels 1 .. 0 from that flow"""
    rows, cols, _ = UPSAMPLE
    a, b = stage_pair(rows, cols)
    whole = run(a, b)["flow"]
    first = run(a, b, 2, 1, dumps=("flow_in",))
    second = run(a, b, 1, 0, init=first["flow_in"])
    assert torch.equal(second["flow"], whole)


def test_a_handle_reused_at_other_sizes():
    import maua_amd.flow as F
    big = F.Farneback(128, 128)
    for rows, cols in ((80, 96), (200, 15), (128, 128)):
        a, b = FR.textured_pair(rows, cols, seed=rows)
        fresh = F.Farneback(rows, cols)
        assert torch.equal(run(a, b, fb=big)["flow"], run(a, b, fb=fresh)["flow"]), (rows, cols)
        fresh.close()
    big.close()


def test_refusals_that_need_a_handle():
    import maua_amd.flow as F
    from maua_amd import _lib as L
    small = F.Farneback(15, 15)
    d = F.farneback_desc(0x1000, 0x2000, 15, 16, 0x3000, 0x4000)
    assert F.farneback_check(d) is None
    assert F.farneback_check(d, small) == "maua_farneback: the image exceeds the size the handle was created for"
    with pytest.raises(L.MauaHipError, match="exceeds the size the handle was created for"):
        small.pair(torch.zeros(3, 15, 16), torch.zeros(3, 15, 16))
    small.close()


# ------------------------------------------------------------------------------------------------------------------ the whole chain
@pytest.mark.parametrize("kind", CHAIN_INPUTS)
@pytest.mark.parametrize("rows,cols", CHAIN_SIZES)
def test_whole_chain(rows, cols, kind):
    """Every level and 15 iterations against the float64 restatement; the bar is four times the restatement's own float32 / float64
    spread on these inputs (tests/test_gpu_video_pipeline.py's, at the smallest size, sizes without a coarser level, and a textured input).

    Measured on one MI355X (device error forward / backward, spread, bar):
        textured 15x15 1.1e-6 / 1.1e-6, 1.5e-6, 6.0e-6;  sinusoid 15x15 8.0e-7 / 8.3e-7, 1.2e-6, 4.6e-6
        textured 39x39 2.4e-6 / 1.5e-6, 2.3e-6, 9.2e-6;  sinusoid 39x39 4.0e-6 / 3.0e-6, 4.2e-6, 1.7e-5
        textured 40x47 2.0e-6 / 1.4e-6, 1.3e-6, 5.1e-6;  sinusoid 40x47 3.1e-6 / 3.5e-6, 4.4e-6, 1.8e-5
        textured 33x130 2.1e-6 / 1.8e-6, 1.7e-6, 7.0e-6; sinusoid 33x130 2.2e-6 / 1.8e-6, 2.5e-6, 1.0e-5
    Before that, the sinusoid pair at 33x130 found fb_gray wrong: 2.687e-4 / 3.773e-4 px against a bar of 1.004e-5.  One pixel of its second image has a
    luminance of 106.0000009; the kernel's 0.7152 g + 0.2126 r had been contracted into one fused multiply-add, the float32 value landed
    one ulp lower and the byte at 105 where torch has 106 - and one grey level at one pixel moves the flow by exactly these figures (the
    float64 restatement with that pixel at 105).  The kernel now rounds every product and sum on its own; test_gray_is_exact plants the
    pixel."""
    r = chain_references(kind, rows, cols)
    assert r["spread"] <= SPREAD_LIMIT
    f = run(r["a"], r["b"])["flow"]
    e_ab, e_ba = float((f[0].double() - r["ab64"]).abs().max()), float((f[1].double() - r["ba64"]).abs().max())
    print(f"farneback {kind} {cols}x{rows}: device vs float64 restatement max abs {e_ab:.3e} / {e_ba:.3e}; spread {r['spread']:.3e}, "
          f"bar {4 * r['spread']:.3e}")
    note("whole chain / (4 x spread)", max(e_ab, e_ba) / (4 * r["spread"]))
    assert max(e_ab, e_ba) <= 4 * r["spread"]


def test_zz_report():
    for h in _handles.values():
        h.close()
    _handles.clear()
    for k, v in WORST.items():
        print(f"worst error / bound  {k:28s} {v:.3f}")
