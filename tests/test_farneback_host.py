"""CPU-only side of tests/test_gpu_farneback.py: the cases and inputs both files share, every refusal of maua_farneback_check by its
text, maua_farneback_level_size against tests/flow_ref.py, and the proof that the reference alone stays inside what the GPU test
demands - every stage bound of flow_ref holds for the float32 restatement against the float64 one on the GPU test's own inputs with
ratio <= 1, the share of pixels the one-iteration bound leaves out is within 0.5 %, the constructed flows of the matrices test take
both branches where they are meant to, and the whole-chain inputs are well enough conditioned for the 4 x spread bar.

No level size of this pyramid rounds half to even: rows 0.8^k = n + 1/2 needs rows 2^(2k+1) = 5^k (2n + 1), an even number equal to an
odd one.  The sizes below whose level lands closest to a half (57 -> 36.48, 82 -> 52.48, 68 -> 43.52 at level 2) stand in for it."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flow_ref as FR  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
NEW_SYMBOLS = ["maua_farneback_level_size", "maua_farneback_check", "maua_farneback_pair_ex"]

# (rows, cols[, level]) of every family of tests/test_gpu_farneback.py
GRAY_SIZES = [(15, 17), (45, 40)]
BLUR_CASES = [(45, 40, 0), (104, 128, 5), (123, 160, 6)]   # level 0; the top level of 128 x 104 (5 taps) and of 160 x 123 (7 taps)
RESIZE_CASES = [(57, 71, 2), (45, 40, 0)]                  # 57 x 0.64 = 36.48, 71 x 0.64 = 45.44; level 0: the identity
POLY_SIZES = [(15, 15), (15, 40), (33, 15), (45, 40)]
MAT_SIZES = [(15, 15), (15, 41), (37, 15), (26, 35)]       # 15: the border table's two ends meet (x = 4 / 5 .. 9 / 10)
ITER_SIZES = [(15, 15), (17, 33), (16, 64), (45, 40)]      # one partial tile; ragged by one pixel each way; exact tiles; 40 x 45
UPSAMPLE = (57, 71, 2)                                     # level 2 -> level 1
CHAIN_SIZES = [(15, 15), (39, 39), (47, 40), (130, 33)]
CHAIN_INPUTS = ["textured", "sinusoid"]
SPREAD_LIMIT = 1e-3

_pairs, _chain = {}, {}


def stage_pair(rows, cols):
    """The textured pair the stage tests run on (computed once per size)."""
    if (rows, cols) not in _pairs:
        _pairs[rows, cols] = FR.textured_pair(rows, cols, seed=1000 * rows + cols)
    return _pairs[rows, cols]


def chain_references(kind, rows, cols):
    """A whole-chain input and the restatement's flows of it in float32 and float64, both directions (computed once)."""
    key = (kind, rows, cols)
    if key not in _chain:
        a, b = FR.textured_pair(rows, cols, seed=7) if kind == "textured" else FR.sinusoid_pair(rows, cols)
        r = dict(a=a, b=b, ab32=FR.farneback(a, b), ab64=FR.farneback(a, b, torch.float64), ba32=FR.farneback(b, a),
                 ba64=FR.farneback(b, a, torch.float64))
        r["spread"] = max(float((r["ab32"].double() - r["ab64"]).abs().max()), float((r["ba32"].double() - r["ba64"]).abs().max()))
        _chain[key] = r
    return _chain[key]


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_counted():
    from maua_amd import _lib as L
    from maua_amd.build import build
    syms = L.declared_symbols()
    assert all(s in syms for s in NEW_SYMBOLS)
    lib = ctypes.CDLL(str(build()))
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    stated = re.search(r"\*\*(\d+) entry points\*\*", (ROOT / "DESIGN.md").read_text())
    assert stated and int(stated.group(1)) == len(syms), (stated and stated.group(1), len(syms))
    # the descriptor's fields, in the header's order
    header = (ROOT / "include" / "maua_hip.h").read_text()
    body = re.search(r"typedef struct \{([^}]*)\} maua_farneback_desc;", header).group(1)
    names = re.findall(r"(\w+)\s*[;,]", body)
    assert names == [f[0] for f in L.FbDesc._fields_], names


def refusal(**kw):
    import maua_amd.flow as F
    args = dict(im_a=0x1000, im_b=0x2000, height=40, width=48, flow_ab=0x3000, flow_ba=0x4000)
    args.update(kw)
    return F.farneback_check(F.farneback_desc(**args))


def test_every_refusal_by_its_text():
    """Without a handle (there is none without a device) the descriptor alone is checked; the handle's pixel count and device are
    refused in tests/test_gpu_farneback.py.  "pyramid blur wider than the image" cannot be reached from outside: the top level keeps
    the smaller side at 32 px or more of a blur whose radius is 1.25 (1 / scale - 1) < 32 / scale."""
    from maua_amd import _lib as L
    assert refusal() is None
    assert refusal(level_hi=1, level_lo=0) is None and refusal(level_hi=1, level_lo=1, iterations=15, init_ab=0x5000, init_ba=0x6000) is None
    assert refusal(gray=0x7000, mat=0x8000) is None
    null = "maua_farneback: NULL or aliased argument"
    for kw in (dict(im_a=0), dict(im_b=0), dict(flow_ab=0), dict(flow_ba=0), dict(flow_ba=0x3000), dict(flow_ab=0x1000), dict(flow_ba=0x2000)):
        assert refusal(**kw) == null, kw
    small = "maua_farneback: the image must be at least 15 x 15"
    assert refusal(height=14) == small and refusal(width=14, height=15) == small and refusal(height=15, width=15) is None
    assert refusal(height=8193, width=8192) == "maua_farneback: the image exceeds 2^26 pixels"
    order = "maua_farneback: level_hi .. level_lo must run downwards to a level >= 0 (-1, -1: every level)"
    assert refusal(level_hi=0, level_lo=1) == order and refusal(level_hi=-1, level_lo=0) == order and refusal(level_hi=0, level_lo=-1) == order
    above = "maua_farneback: level_hi is above the top level of this size (maua_farneback_levels - 1)"
    assert refusal(level_hi=2, level_lo=0) == above and refusal(height=39, level_hi=1, level_lo=1) == above
    its = "maua_farneback: iterations must be 1 .. 15 (0: 15)"
    assert refusal(iterations=16) == its and refusal(iterations=-1) == its
    assert refusal(init_ab=0x5000) == refusal(init_ba=0x5000) == "maua_farneback: init_ab and init_ba go together"
    alias = "maua_farneback: the initial flows must not alias each other or the outputs"
    assert refusal(init_ab=0x5000, init_ba=0x5000) == alias and refusal(init_ab=0x3000, init_ba=0x5000) == alias
    assert L.lib().maua_farneback_check(None, None) != 0 and L.lib().maua_last_error().decode() == "maua_farneback: the descriptor is NULL"
    assert L.lib().maua_farneback_pair_ex(None, None, None) != 0 and L.lib().maua_last_error().decode() == "maua_farneback: NULL handle or ctx"
    h = w = ctypes.c_int()
    assert L.lib().maua_farneback_level_size(40, 48, 2, ctypes.byref(h), ctypes.byref(w)) != 0
    assert L.lib().maua_last_error().decode() == "maua_farneback_level_size: no such level at this size"


@pytest.mark.parametrize("rows,cols", [(15, 15), (39, 39), (45, 40), (57, 71), (82, 68), (104, 128), (123, 160), (512, 512), (720, 1281)])
def test_level_sizes(rows, cols):
    import maua_amd.flow as F
    n = F.farneback_levels(rows, cols)
    assert n == FR.pyramid_levels(rows, cols) + 1
    for k in range(n):
        assert F.farneback_level_size(rows, cols, k) == FR.level_size(rows, cols, k), k
        h, w = FR.level_size(rows, cols, k)
        assert (h, w) == (int(np.rint(rows * 0.8 ** k)), int(np.rint(cols * 0.8 ** k))) and (k == 0 or min(h, w) >= 32)
    assert F.farneback_level_size(rows, cols, 0) == (rows, cols)


# ------------------------------------------------------------------------------------------------------------------ the reference alone
def test_gray_inputs_reach_the_clamps_and_the_planted_values():
    for rows, cols in GRAY_SIZES:
        a, b, planted = FR.gray_images(rows, cols)
        lum = lambda im: (0.2126 * im[0] + 0.7152 * im[1] + 0.0722 * im[2]) * 255
        for im in (a, b):
            assert float(lum(im).min()) < 0 and float(lum(im).max()) > 255
        g = FR.to_gray_u8(a)
        assert {k for _, k, _ in planted} == {"integer", "below", "zero", "contraction"}
        assert FR.gray_contracted(FR.CONTRACTION_PIXEL) == 105       # the pixel tells a contracted luminance from torch's
        for x, kind, value in planted:
            assert float(g[0, x]) == value, (x, kind)
        assert float(lum(a)[0, 4]) == 255.0                # 255 exactly, not through the clamp
        # rounding to nearest would differ from the truncation on about half of the pixels
        assert float((torch.round(lum(a).clamp(0, 255)) != g).float().mean()) > 0.3


@pytest.mark.parametrize("rows,cols,k", BLUR_CASES)
def test_restated_blur_is_inside_its_bound(rows, cols, k):
    assert k <= FR.pyramid_levels(rows, cols) and (k == 0 or k == FR.pyramid_levels(rows, cols))
    taps = FR.level_taps(k).shape[0]
    assert taps == {0: 3, 5: 5, 6: 7}[k]
    d = FR.restate_level(*stage_pair(rows, cols), k)
    r = FR.check_blur(d, k)
    print(f"restated blur {cols}x{rows} level {k} ({taps} taps): worst error / bound {r:.3f}")
    assert r <= 1


@pytest.mark.parametrize("rows,cols,k", RESIZE_CASES)
def test_restated_resize_is_inside_its_bound(rows, cols, k):
    d = FR.restate_level(*stage_pair(rows, cols), k)
    r = FR.check_resize(d)
    print(f"restated resize {cols}x{rows} level {k}: worst error / bound {r:.3f}")
    assert r <= 1
    if k == 0:
        assert torch.equal(d["level"], d["blur"])


@pytest.mark.parametrize("rows,cols", POLY_SIZES)
def test_restated_expansion_is_inside_its_bound(rows, cols):
    r = FR.check_poly(FR.restate_level(*stage_pair(rows, cols), 0))
    print(f"restated polynomial expansion {cols}x{rows}: worst error / bound {r:.3f}")
    assert r <= 1


@pytest.mark.parametrize("rows,cols", MAT_SIZES)
def test_matrices_inputs_and_restatement(rows, cols):
    flows, planted = FR.matrices_flows(rows, cols)
    d = FR.restate_level(*stage_pair(rows, cols), 0, init=flows)
    r, inside = FR.check_matrices(d)
    for i, y, x, want in planted:
        assert bool(inside[i, y, x]) == want, (i, y, x, want)
    assert {w for *_, w in planted} == {True, False}
    yy, xx = torch.meshgrid([torch.arange(rows), torch.arange(cols)], indexing="ij")
    for i in range(2):
        fx, fy = torch.floor(xx + flows[i, ..., 0]), torch.floor(yy + flows[i, ..., 1])
        sides = dict(left=fx < 0, right=fx >= cols - 1, top=fy < 0, bottom=fy >= rows - 1)
        share = {k: float(v.float().mean()) for k, v in sides.items()}
        out = 1 - float(inside[i].float().mean())
        print(f"matrices inputs {cols}x{rows} direction {i}: outside {out:.3f} {share}")
        assert all(v >= 0.05 for v in share.values()) and 0.25 <= out <= 0.45
        assert float(flows[i].abs().max()) == 10 * cols and bool(torch.isfinite(flows[i]).all())
    print(f"restated matrices {cols}x{rows}: worst error / bound {r:.3f}")
    assert r <= 1


@pytest.mark.parametrize("rows,cols", ITER_SIZES)
def test_restated_iterations_are_inside_their_bounds(rows, cols):
    a, b = stage_pair(rows, cols)
    d1, d2 = FR.restate_level(a, b, 0, iterations=1), FR.restate_level(a, b, 0, iterations=2)
    r1, out1 = FR.check_iteration(d1)
    r2, out2 = FR.check_second_iteration(d1, d2)
    print(f"restated iterations {cols}x{rows}: one {r1:.3f} ({out1:.4f} left out), two {r2:.3f} ({out2:.4f} left out)")
    assert r1 <= 1 and r2 <= 1 and out1 <= 0.005 and out2 <= 0.005


def test_restated_upsample_is_inside_its_bound():
    rows, cols, k = UPSAMPLE
    flow_k = FR.restate_level(*stage_pair(rows, cols), k)["flow"]
    h, w = FR.level_size(rows, cols, k - 1)
    up = FR.fb_resize(flow_k.permute(0, 3, 1, 2), h, w).permute(0, 2, 3, 1) * torch.tensor(1.0 / FR.PYR_SCALE).float()
    r = FR.check_upsample(flow_k, up, h, w)
    print(f"restated flow upsample {cols}x{rows} level {k} -> {k - 1}: worst error / bound {r:.3f}")
    assert r <= 1 and float(flow_k.abs().max()) > 0.5


@pytest.mark.parametrize("kind", CHAIN_INPUTS)
@pytest.mark.parametrize("rows,cols", CHAIN_SIZES)
def test_chain_inputs_are_well_conditioned(rows, cols, kind):
    r = chain_references(kind, rows, cols)
    print(f"farneback restatement {kind} {cols}x{rows}: float32 vs float64 max abs {r['spread']:.3e}")
    assert 0 < r["spread"] <= SPREAD_LIMIT
