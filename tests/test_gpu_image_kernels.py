"""The image-space kernels (csrc/image_ops.hip, csrc/resize.hip, csrc/cutouts.hip, csrc/colormatch.hip) one entry point at a time, straight
through the C ABI, against the twin tests/image_ref.py - the method of tests/test_gpu_latent_kernels.py: 4096 guard elements on both
sides of every buffer (tests/cabi_guard.py), after each call the guards are intact, the result is fully written and holds no NaN from
a guard, the comparison holds and a second call gives the same bits.  An exact family is compared bit for bit, a bounded family
inside the bound that tests/image_ref.py derives next to its reference; every argument check of the launchers is a refusal by name
with the outputs untouched.  tests/test_image_kernels_host.py holds the twin against torch, the restated third-party pieces, the
oracle and the fixtures, and shows that these comparisons reject off-by-one mutants of the twin at the shapes used here.
test_zz_report prints the worst error / bound per family (WORST).

Exact, bit for bit: perlin (raw, bytes through an identity table, table, image), restitch (acc / norm in the reference's tile order),
destitch, resize2d mode 1 (F.pad, all modes, three dtypes; circular padding larger than the input wraps again, as include/maua_hip.h
says), grad_accumulate, min / max of moments, the cutouts' tap tables (through single-pixel images), the colour-match histogram (of
single-pixel images, one per special colour, and of the random image: the normalisation's float32 sum restated in the kernel's order).
Bounded (tests/image_ref.py, next to each reference): image_resize, sharpen, moments' sums (a running bound over the fixed tree),
match_apply, conv1d_reflect and its vjp, bicubic in three dtypes and its vjp, the cutouts and their vjp, the colour-match gradient;
two dot-product identities <vjp(d), x> = <d, fwd(x)> in float64 within the two bounds."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import image_ref as R  # noqa: E402
from cabi_guard import G, Buf, call, inp, ratio, same  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
F = np.float32
TORCH_DT = {"f32": (torch.float32, 0), "bf16": (torch.bfloat16, 1), "f16": (torch.float16, 2)}


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), float(r))
    return r


def ints(v):
    return (C.c_int * len(v))(*[int(u) for u in v])


def floats(v):
    return (C.c_float * len(v))(*[float(u) for u in v])


def refused_with(text, name, *args):
    """refused, and with the entry point's own message (never a bare launch error)"""
    rc = getattr(L.lib(), name)(L.ctx(), *args)
    assert rc != 0, f"{name} accepted {args}"
    with pytest.raises(L.MauaHipError, match=text):
        L.check(rc)
    torch.cuda.synchronize()


def twice(run):
    """run() -> arrays; the second call gives the same bits"""
    a, b = run(), run()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert same(x.view(np.uint8), y.view(np.uint8)), "two calls differ"
    return a


# ---------------------------------------------------------------------------------------------------------------- image_resize
def tables(n_in, n_out, kernel):
    import maua_amd.image as I
    left, w = I.resize_tables(n_in, n_out, kernel)
    return left.numpy(), w.numpy()


def run_image_resize(src, Ho, Wo, ty, tx, prior=None, add=0.0):
    planes, H, W = src.shape
    sb = inp(src)
    tb = [None if t is None else (inp(t[0], torch.int32, guard=0), inp(t[1])) for t in (ty, tx)]
    out = Buf(planes * Ho * Wo) if prior is None else inp(prior)
    a = [(None, None, 0) if t is None else (t[0].ptr, t[1].ptr, t_[1].shape[1]) for t, t_ in zip(tb, (ty, tx))]
    call("maua_image_resize", sb.ptr, planes, H, W, out.ptr, Ho, Wo, *a[0], *a[1], int(prior is not None), add)
    out.check("image_resize", written=prior is None)
    sb.check("image_resize input")
    for t in tb:
        if t is not None:
            t[0].check("left table")
            t[1].check("weight table")
    return out.get().reshape(planes, Ho, Wo)



@pytest.mark.parametrize("H,W,Ho,Wo", R.IMAGE_RESIZE_CASES)
def test_image_resize(H, W, Ho, Wo):
    for kernel in ("cubic", "lanczos3"):
        src = R.normal((5, H, W), H + W)
        ty = tables(H, Ho, kernel) if H != Ho else None
        tx = tables(W, Wo, kernel) if W != Wo else None
        for prior, add in ((None, 0.0), (None, -1.0), (R.normal((5, Ho, Wo), 3), 0.25)):
            want, bound = R.image_resize(src, Ho, Wo, *(ty or (None, None)), *(tx or (None, None)), prior=prior, add=add)
            got = twice(lambda: run_image_resize(src, Ho, Wo, ty, tx, prior, add))
            assert note("image_resize", ratio(got, want, bound)) <= 1, (kernel, prior is not None, add)


def test_image_resize_taps_leaving_the_image_on_both_sides():
    src = R.normal((5, 3, 4), 1)
    ty = (np.array([-2, -1, 0, 1, 2, -4, 3], np.int32), R.normal((7, 5), 2))       # rows -2 .. 2 / 3 .. 7 of 3: some taps outside, some rows all outside
    tx = (np.array([-3, 2, -1], np.int32), R.normal((3, 6), 3))
    want, bound = R.image_resize(src, 7, 3, *ty, *tx)
    assert note("image_resize", ratio(twice(lambda: run_image_resize(src, 7, 3, ty, tx)), want, bound)) <= 1


def test_image_resize_refusals():
    src, out, li, w = inp(np.zeros(5 * 12)), Buf(5 * 20), inp(np.zeros(8), torch.int32, guard=0), inp(np.zeros(64))
    ok = (src.ptr, 5, 3, 4, out.ptr, 4, 5, li.ptr, w.ptr, 4, li.ptr, w.ptr, 4, 0, 0.0)

    def but(**kw):
        names = ("src", "planes", "H", "W", "dst", "Ho", "Wo", "ly", "wy", "ty", "lx", "wx", "tx", "acc", "add")
        return [kw.get(n, v) for n, v in zip(names, ok)]
    call("maua_image_resize", *but(planes=0))
    assert out.untouched()
    for kw in (dict(src=None), dict(dst=None), dict(dst=src.ptr), dict(planes=-1), dict(planes=65536), dict(H=0), dict(H=-3), dict(W=0), dict(W=-4),
               dict(Ho=0), dict(Ho=-4), dict(Wo=0), dict(Wo=-5), dict(wy=None), dict(ty=0), dict(ty=-1), dict(wx=None), dict(tx=0), dict(ly=None),
               dict(lx=None), dict(W=16385)):
        refused_with("maua_image_resize", "maua_image_resize", *but(**kw))
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- destitch / restitch

def weights(n, T, seed):
    """positive blend weights (a zero weight sum is the reference's 0 / 0; maua_amd/image.py's tables are held on the host)"""
    return (R.uniform((n, T), seed, 0.05, 1.0)).astype(F)


@pytest.mark.parametrize("H,W,T,ys,xs", R.GRIDS)
def test_destitch_restitch(H, W, T, ys, xs):
    B = 2
    img = R.normal((B, 3, H, W), H * W)
    n = len(ys) * len(xs)

    def run_de():
        ib, out = inp(img), Buf(n * B * 3 * T * T)
        call("maua_image_destitch", ib.ptr, B, H, W, T, ints(ys), len(ys), ints(xs), len(xs), out.ptr)
        out.check("destitch")
        ib.check("destitch input")
        return out.get().reshape(n * B, 3, T, T)
    assert same(twice(run_de), R.destitch(img, T, ys, xs))
    tiles, wy, wx = R.normal((n, 3, T, T), n + T), weights(len(ys), T, 1), weights(len(xs), T, 2)

    def run_re():
        tb, yb, xb, out = inp(tiles), inp(wy), inp(wx), Buf(3 * H * W)
        call("maua_image_restitch", tb.ptr, T, ints(ys), len(ys), ints(xs), len(xs), yb.ptr, xb.ptr, out.ptr, H, W)
        out.check("restitch")
        for b in (tb, yb, xb):
            b.check("restitch input")
        return out.get().reshape(3, H, W)
    want, _acc, norm = R.restitch32(tiles, T, ys, xs, wy, wx, H, W)
    assert (norm > 0).all()
    assert same(twice(run_re), want)


def test_destitch_restitch_refusals():
    img, out, w = inp(np.zeros(2 * 3 * 11 * 13)), Buf(6 * 2 * 3 * 25), inp(np.ones(15))
    ys, xs = [0, 3, 6], [0, 8]
    call("maua_image_destitch", img.ptr, 0, 11, 13, 5, ints(ys), 3, ints(xs), 2, out.ptr)
    assert out.untouched()
    for a in ((None, 2, 11, 13, 5, ints(ys), 3, ints(xs), 2, out.ptr), (img.ptr, 2, 11, 13, 5, ints(ys), 3, ints(xs), 2, None),
              (img.ptr, -1, 11, 13, 5, ints(ys), 3, ints(xs), 2, out.ptr), (img.ptr, 21846, 11, 13, 5, ints(ys), 3, ints(xs), 2, out.ptr),
              (img.ptr, 2, 0, 13, 5, ints(ys), 3, ints(xs), 2, out.ptr), (img.ptr, 2, 11, -13, 5, ints(ys), 3, ints(xs), 2, out.ptr),
              (img.ptr, 2, 11, 13, 0, ints(ys), 3, ints(xs), 2, out.ptr), (img.ptr, 2, 11, 13, 12, ints(ys), 3, ints(xs), 2, out.ptr),
              (img.ptr, 2, 11, 13, 5, None, 3, ints(xs), 2, out.ptr), (img.ptr, 2, 11, 13, 5, ints(ys), 0, ints(xs), 2, out.ptr),
              (img.ptr, 2, 11, 13, 5, ints(ys), 3, ints(xs), -2, out.ptr), (img.ptr, 2, 11, 13, 5, ints(ys), 65, ints(xs), 2, out.ptr),
              (img.ptr, 2, 11, 13, 5, ints([0, 3, 7]), 3, ints(xs), 2, out.ptr), (img.ptr, 2, 11, 13, 5, ints(ys), 3, ints([-1, 8]), 2, out.ptr)):
        refused_with("maua_image_destitch", "maua_image_destitch", *a)
    tiles = inp(np.zeros(6 * 3 * 25))
    ok = dict(tiles=tiles.ptr, T=5, ys=ys, xs=xs, wy=w.ptr, wx=w.ptr, out=out.ptr, H=11, W=13)

    def re(**kw):
        k = dict(ok, **kw)
        return (k["tiles"], k["T"], None if k["ys"] is None else ints(k["ys"]), len(k["ys"] or []) if "nr" not in k else k["nr"],
                ints(k["xs"]), len(k["xs"]) if "nc" not in k else k["nc"], k["wy"], k["wx"], k["out"], k["H"], k["W"])
    for kw in (dict(tiles=None), dict(wy=None), dict(wx=None), dict(out=None), dict(T=0), dict(T=-5), dict(H=0), dict(W=-13), dict(H=65536),
               dict(nr=0), dict(nc=-1), dict(nr=65), dict(ys=[0, 3, 5]),        # the last row is not flush with the edge
               dict(ys=[1, 3, 6]), dict(xs=[0, 6]),                             # the first not at 0 / a gap between columns 0 and 6 (T = 5)
               dict(ys=[0, 6, 3]), dict(xs=[0, 9])):                            # not ascending / leaves the image
        refused_with("maua_image_restitch", "maua_image_restitch", *re(**kw))
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- sharpen
@pytest.mark.parametrize("H,W", [(1, 1), (2, 5), (3, 3), (3, 257), (17, 19)])
def test_sharpen(H, W):
    B = 2
    img = R.uniform((B * 3, H, W), H + W, -1.5, 1.5)                   # beyond [-1, 1]: the clamp to [0, 1] of (x + 1) / 2 is live
    for strength in (0.0, 0.5, 1.0, 2.5, -0.75):
        def run():
            ib, out = inp(img), Buf(img.size)
            call("maua_image_sharpen", ib.ptr, B, H, W, strength, out.ptr)
            out.check("sharpen")
            ib.check("sharpen input")
            return out.get().reshape(img.shape)
        want, bound = R.sharpen(img, strength)
        assert note("sharpen", ratio(twice(run), want, bound)) <= 1, strength


def test_sharpen_refusals():
    img, out = inp(np.zeros(54)), Buf(54)
    call("maua_image_sharpen", img.ptr, 0, 3, 3, 1.0, out.ptr)
    assert out.untouched()
    for a in ((None, 2, 3, 3, 1.0, out.ptr), (img.ptr, 2, 3, 3, 1.0, None), (img.ptr, 2, 3, 3, 1.0, img.ptr), (img.ptr, -2, 3, 3, 1.0, out.ptr),
              (img.ptr, 2, 0, 3, 1.0, out.ptr), (img.ptr, 2, 3, -3, 1.0, out.ptr), (img.ptr, 21846, 3, 3, 1.0, out.ptr),
              (img.ptr, 2, 65536, 3, 1.0, out.ptr)):
        refused_with("maua_image_sharpen", "maua_image_sharpen", *a)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- moments / match_apply
@pytest.mark.parametrize("HW", [1, 4095, 4096, 4097])
def test_moments(HW):
    frames = 2
    assert L.lib().maua_image_moments_slices(HW) == R.moments_slices(HW)
    for navg in (1, 3):
        img = R.uniform((frames * navg, 3, HW), HW + navg, -1.2, 1.2)
        noise = R.normal((frames, 3, HW), HW)
        for ns in (None, 1e-3):
            S = R.moments_slices(HW)

            def run():
                ib, nb, out = inp(img), inp(noise), Buf(frames * S * 11)
                call("maua_image_moments", ib.ptr, frames, navg, HW, None if ns is None else nb.ptr, ns or 0.0, out.ptr)
                out.check("moments")
                ib.check("moments input")
                nb.check("moments noise")
                return out.get().reshape(frames, S, 11)
            got = twice(run)
            want, bound = R.moments(img, navg, None if ns is None else noise, ns or 0.0)
            assert same(got[..., 9:], want[..., 9:].astype(F)), "min / max are exact"
            assert note("moments", ratio(got[..., :9], want[..., :9], bound[..., :9])) <= 1, (navg, ns)


@pytest.mark.parametrize("HW", [1, 257])
def test_match_apply(HW):
    img, noise, prior = R.normal((3, HW), HW), R.normal((3, HW), HW + 1), R.normal((3, HW), HW + 2)
    m, mu_t, mu_s = R.normal((9,), 4), R.normal((3,), 5), R.normal((3,), 6)
    for ns in (None, 1e-3):
        for acc in (0, 1):
            for clamp in (0, 1):
                def run():
                    ib, nb = inp(img), inp(noise)
                    out = inp(prior) if acc else Buf(3 * HW)
                    call("maua_image_match_apply", ib.ptr, None if ns is None else nb.ptr, ns or 0.0, HW, floats(m), floats(mu_t), floats(mu_s),
                         0.5, acc, clamp, -0.4, 0.6, out.ptr)
                    out.check("match_apply", written=not acc)
                    ib.check("match_apply input")
                    nb.check("match_apply noise")
                    return out.get().reshape(3, HW)
                want, bound = R.match_apply(img, None if ns is None else noise, ns or 0.0, m, mu_t, mu_s, 0.5, prior if acc else None, clamp,
                                            -0.4, 0.6)
                assert note("match_apply", ratio(twice(run), want, bound)) <= 1, (ns, acc, clamp)


def test_moments_and_match_apply_refusals():
    img, out = inp(np.zeros(64)), Buf(64)
    call("maua_image_moments", img.ptr, 0, 1, 4, None, 0.0, out.ptr)
    assert out.untouched()
    for a in ((None, 2, 1, 4, None, 0.0, out.ptr), (img.ptr, 2, 1, 4, None, 0.0, None), (img.ptr, -2, 1, 4, None, 0.0, out.ptr),
              (img.ptr, 2, 0, 4, None, 0.0, out.ptr), (img.ptr, 2, -1, 4, None, 0.0, out.ptr), (img.ptr, 2, 1, 0, None, 0.0, out.ptr),
              (img.ptr, 2, 1, -4, None, 0.0, out.ptr), (img.ptr, 65536, 1, 4, None, 0.0, out.ptr)):
        refused_with("maua_image_moments", "maua_image_moments", *a)
    m, v = floats(np.eye(3).ravel()), floats([0, 0, 0])
    for a in ((None, None, 0.0, 4, m, v, v, 1.0, 0, 0, 0.0, 1.0, out.ptr), (img.ptr, None, 0.0, 4, None, v, v, 1.0, 0, 0, 0.0, 1.0, out.ptr),
              (img.ptr, None, 0.0, 4, m, None, v, 1.0, 0, 0, 0.0, 1.0, out.ptr), (img.ptr, None, 0.0, 4, m, v, None, 1.0, 0, 0, 0.0, 1.0, out.ptr),
              (img.ptr, None, 0.0, 4, m, v, v, 1.0, 0, 0, 0.0, 1.0, None), (img.ptr, None, 0.0, 0, m, v, v, 1.0, 0, 0, 0.0, 1.0, out.ptr),
              (img.ptr, None, 0.0, -4, m, v, v, 1.0, 0, 0, 0.0, 1.0, out.ptr)):
        refused_with("maua_image_match_apply", "maua_image_match_apply", *a)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- perlin
def perlin_grads(width, height, n, ch, seed, flat=False):
    g = []
    for c in range(ch):
        for k in range(n):
            a = R.normal((2, (width << k) + 1, (height << k) + 1), seed + 10 * c + k)
            g.append(np.zeros_like(a) if flat and c == 0 else a)
    return g


def run_perlin(grads, octaves, width, height, grayscale):
    n, ch = len(octaves), (1 if grayscale else 3)
    S = (width << n) * (height << n)
    gb, raw, out = inp(np.concatenate([g.ravel() for g in grads])), Buf(ch * S), Buf(3 * S)
    offs = R.perlin_offsets(grads)
    call("maua_image_perlin", gb.ptr, (C.c_long * len(offs))(*offs), floats(octaves), n, width, height, int(grayscale), raw.ptr, out.ptr)
    raw.check("perlin raw")
    out.check("perlin image")
    gb.check("perlin gradients")
    return raw.get().reshape(ch, width << n, height << n), out.get().reshape(3, width << n, height << n)


def ulps(a, b):
    ia, ib = (np.where(v.view(np.int32) < 0, np.int32(-2 ** 31) - v.view(np.int32), v.view(np.int32)).astype(np.int64) for v in (a, b))
    return np.abs(ia - ib)


@pytest.mark.parametrize("width,height,n", [(1, 1, 1), (2, 3, 3), (3, 2, 4)])
@pytest.mark.parametrize("grayscale", [False, True])
def test_perlin(width, height, n, grayscale):
    ch = 1 if grayscale else 3
    octaves = [1.0, 0.5, 0.3, 0.7][:n]
    for flat in (False, True):
        grads = perlin_grads(width, height, n, ch, 7 * width + n, flat)
        raw, out = twice(lambda: run_perlin(grads, octaves, width, height, grayscale))
        want = R.perlin32(grads, octaves, width, height, grayscale)
        diff = ulps(raw, want["raw"])
        print(f"perlin {width} x {height}, {n} octaves, grey {grayscale}, flat {flat}: {int((diff > 0).sum())} of {diff.size} raw elements differ, "
              f"by up to {int(diff.max())} ulp; {int((out != want['out']).sum())} image elements differ")
        assert same(raw, want["raw"]), "the octave sum, every operation rounded on its own"
        assert same(out, want["out"]), "bytes, autocontrast table and to_tensor"
        if flat:                                           # channel 0 is 0.5 everywhere: hi <= lo, the table is the identity, out * 255 is the byte
            assert (want["lut"][0] == np.arange(256)).all() and same(out[0] * F(255.0), want["q"][0].astype(F)) and want["q"][0, 0, 0] == 127


def test_perlin_refusals():
    g, raw, out = inp(np.zeros(64)), Buf(12), Buf(12)
    offs, octs = (C.c_long * 17)(*([0] * 17)), floats([1.0] * 17)
    for a in ((None, offs, octs, 1, 1, 1, 1, raw.ptr, out.ptr), (g.ptr, None, octs, 1, 1, 1, 1, raw.ptr, out.ptr),
              (g.ptr, offs, None, 1, 1, 1, 1, raw.ptr, out.ptr), (g.ptr, offs, octs, 1, 1, 1, 1, raw.ptr, None),
              (g.ptr, offs, octs, 0, 1, 1, 1, raw.ptr, out.ptr), (g.ptr, offs, octs, -1, 1, 1, 1, raw.ptr, out.ptr),
              (g.ptr, offs, octs, 17, 1, 1, 1, raw.ptr, out.ptr), (g.ptr, offs, octs, 1, 0, 1, 1, raw.ptr, out.ptr),
              (g.ptr, offs, octs, 1, 1, -1, 1, raw.ptr, out.ptr), (g.ptr, offs, octs, 16, 1, 1, 1, raw.ptr, out.ptr)):       # 65536 on a side
        refused_with("maua_image_perlin", "maua_image_perlin", *a)
    assert raw.untouched() and out.untouched()


# ---------------------------------------------------------------------------------------------------------------- grad_accumulate
@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
def test_grad_accumulate(n):
    base, acc0 = R.normal((n,), n), R.normal((n,), n + 1)
    base[0] = np.inf                                          # +-inf is not a NaN: it passes through
    base[-1] = -np.inf if n > 1 else np.inf
    cases = [("clean", base, acc0)]
    for where in sorted({0, n // 2, n - 1}):
        s = base.copy()
        s[where] = np.nan
        cases.append((f"NaN at {where}", s, acc0))
    a = acc0.copy()
    a[n // 2] = np.nan
    cases.append(("acc holds a NaN", base, a))
    for what, sub, acc in cases:
        for first in (0, 1):
            def run():
                sb, ab = inp(sub), inp(acc)
                call("maua_grad_accumulate", sb.ptr, ab.ptr, n, first)
                ab.check("grad_accumulate", nan_ok=True)
                sb.check("grad_accumulate input")
                return ab.get()
            assert same(twice(run), R.grad_accumulate32(sub, acc, first)), (what, first)


def test_grad_accumulate_refusals():
    s, a = inp(np.ones(4)), Buf(4)
    call("maua_grad_accumulate", s.ptr, a.ptr, 0, 1)
    assert a.untouched()
    for args in ((None, a.ptr, 4, 1), (s.ptr, None, 4, 1), (s.ptr, a.ptr, -4, 1)):
        refused_with("maua_grad_accumulate", "maua_grad_accumulate", *args)
    assert a.untouched()


# ---------------------------------------------------------------------------------------------------------------- resize2d, mode 1 (F.pad)
class Half:
    """a bf16 / f16 buffer of n elements on tests/cabi_guard.py's byte buffers (which know 1-, 4- and 8-byte elements): 2 n bytes between
    G more bytes of the same pattern on either side, so that G elements on both sides are watched - 0xFFFF (a NaN in both formats) around
    an input, the sentinel in an output."""

    def __init__(self, n, tdt, data=None):
        self.n, self.tdt = n, tdt
        if data is None:
            self.buf = Buf(2 * n + 2 * G, torch.uint8)
        else:
            body = torch.from_numpy(np.ascontiguousarray(data)).reshape(-1).to(tdt).view(torch.uint8).numpy()
            self.buf = inp(np.concatenate([np.full(G, 255, np.uint8), body, np.full(G, 255, np.uint8)]), torch.uint8, guard=255)
        self.before = self.buf.get().copy()
        self.ptr = C.c_void_p(self.buf.ptr.value + G)

    def check(self, what):
        self.buf.check(what, written=False)
        now = self.buf.get()
        assert same(now[:G], self.before[:G]) and same(now[-G:], self.before[-G:]), f"{what}: a store outside the buffer"
        if self.buf.out:
            assert (now[G:-G].view(np.uint16) != 0x5A5A).all(), f"{what}: elements of the result were never written"
        else:
            assert same(now, self.before), f"{what}: an input was written"

    def get(self):
        v = torch.from_numpy(self.buf.get()[G:-G].copy()).view(self.tdt).float().numpy()
        assert not np.isnan(v).any()
        return v


def run_resize2d(x, oh, ow, mode, pl=0, pt=0, how=R.PAD_CONSTANT, value=0.0, dt="f32"):
    N, Cc, H, W = x.shape
    tdt, code = TORCH_DT[dt]
    xb, out = (inp(x), Buf(N * Cc * oh * ow)) if dt == "f32" else (Half(x.size, tdt, x), Half(N * Cc * oh * ow, tdt))
    call("maua_resize2d", xb.ptr, out.ptr, N, Cc, H, W, oh, ow, mode, pl, pt, how, value, code)
    out.check("resize2d")
    xb.check("resize2d input")
    return out.get().reshape(N, Cc, oh, ow)


@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
def test_resize2d_pad(dt):
    tdt, _ = TORCH_DT[dt]
    for H, W, oh, ow, pl, pt, hows in R.PAD_CASES:
        x = torch.from_numpy(R.normal((2, 3, H, W), H * W + oh)).to(tdt).float().numpy()     # numbers of the dtype
        for how in hows or (R.PAD_CONSTANT, R.PAD_REFLECT, R.PAD_REPLICATE, R.PAD_CIRCULAR):
            value = float(torch.tensor(-0.3).to(tdt))
            got = twice(lambda: run_resize2d(x, oh, ow, 1, pl, pt, how, value, dt))
            assert same(got, R.pad2d(x, oh, ow, pl, pt, how, F(value))), (H, W, oh, ow, pl, pt, how)


# ---------------------------------------------------------------------------------------------------------------- conv1d_reflect


@pytest.mark.parametrize("planes,H,W", R.CONV_SHAPES)
def test_conv1d_reflect_and_vjp(planes, H, W):
    assert (planes * H * W) % 257 == 1
    x, dy = R.normal((planes, H, W), H + W), R.normal((planes, H, W), H * W)
    for axis in (0, 1):
        n = (H, W)[axis]
        for radius in sorted({0, 1, n - 1} & set(range(n))):
            taps = R.normal((2 * radius + 1,), radius + n)
            res = {}
            for name, src in (("maua_conv1d_reflect", x), ("maua_conv1d_reflect_vjp", dy)):
                def run():
                    sb, tb, out = inp(src), inp(taps), Buf(src.size)
                    call(name, sb.ptr, out.ptr, tb.ptr, radius, axis, planes, H, W)
                    out.check(name)
                    sb.check(name + " input")
                    tb.check(name + " taps")
                    return out.get().reshape(src.shape)
                want, bound = R.conv1d_reflect(src, taps, axis, vjp=name.endswith("vjp"))
                got = twice(run)
                assert note(name[5:], ratio(got, want, bound)) <= 1, (axis, radius)
                res[name] = (got.astype(np.float64), bound)
            (fwd, bf), (adj, ba) = res["maua_conv1d_reflect"], res["maua_conv1d_reflect_vjp"]
            lhs, rhs = float((adj * x).sum()), float((dy.astype(np.float64) * fwd).sum())                 # <vjp(d), x> = <d, fwd(x)>
            slack = float((ba * np.abs(x)).sum() + (bf * np.abs(dy)).sum())
            assert abs(lhs - rhs) <= slack, (axis, radius)
            note("conv1d dot identity", abs(lhs - rhs) / max(slack, 1e-300))


def test_resize_refusals():
    x, out, t = inp(np.zeros(64)), Buf(64), inp(np.ones(3))
    for name in ("maua_conv1d_reflect", "maua_conv1d_reflect_vjp"):
        for a in ((x.ptr, out.ptr, t.ptr, 1, 0, 0, 4, 4), (x.ptr, out.ptr, t.ptr, 1, 0, 2, 0, 4), (x.ptr, out.ptr, t.ptr, 1, 0, 2, 4, 0)):
            call(name, *a)                                                   # an empty tensor: nothing is done
        assert out.untouched()
        for a in ((None, out.ptr, t.ptr, 1, 0, 2, 4, 4), (x.ptr, None, t.ptr, 1, 0, 2, 4, 4), (x.ptr, out.ptr, None, 1, 0, 2, 4, 4),
                  (x.ptr, x.ptr, t.ptr, 1, 0, 2, 4, 4), (x.ptr, out.ptr, t.ptr, 1, 0, -2, 4, 4), (x.ptr, out.ptr, t.ptr, 1, 0, -2, -4, 4),
                  (x.ptr, out.ptr, t.ptr, 1, 0, 2, -4, 4), (x.ptr, out.ptr, t.ptr, 1, 0, 2, 4, -4), (x.ptr, out.ptr, t.ptr, -1, 0, 2, 4, 4),
                  (x.ptr, out.ptr, t.ptr, 4, 0, 2, 4, 4), (x.ptr, out.ptr, t.ptr, 4, 1, 2, 5, 4), (x.ptr, out.ptr, t.ptr, 1, 2, 2, 4, 4),
                  (x.ptr, out.ptr, t.ptr, 1, -1, 2, 4, 4)):
            refused_with(name, name, *a)
        assert out.untouched()
    ok = dict(x=x.ptr, y=out.ptr, N=1, C=2, H=3, W=4, oh=2, ow=3, mode=0, pl=0, pt=0, how=3, value=0.0, dt=0)
    for kw in (dict(N=0), dict(C=0), dict(oh=0), dict(ow=0)):
        call("maua_resize2d", *dict(ok, **kw).values())
    assert out.untouched()
    for kw in (dict(x=None), dict(y=None), dict(y=x.ptr), dict(N=-1), dict(C=-2), dict(H=0), dict(H=-3), dict(W=0), dict(W=-4), dict(oh=-2),
               dict(ow=-3), dict(oh=-2, ow=-3), dict(N=-1, C=-2), dict(mode=3), dict(mode=-1), dict(mode=1, how=4), dict(mode=1, how=-1),
               dict(dt=3), dict(dt=-1), dict(mode=1, how=1, oh=7, pt=3), dict(mode=1, how=1, ow=9, pl=4), dict(mode=1, how=1, oh=7, pt=0)):
        refused_with("resize2d", "maua_resize2d", *dict(ok, **kw).values())
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- bicubic and its vjp
@pytest.mark.parametrize("dt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("H,W,oh,ow", R.BICUBIC_SHAPES)
def test_resize2d_bicubic(H, W, oh, ow, dt):
    tdt, _ = TORCH_DT[dt]
    assert (2 * 3 * oh * ow) % 256
    x = torch.from_numpy(R.normal((2, 3, H, W), H * W + ow)).to(tdt).float().numpy()
    for mode in (0, 2):
        want, bound = R.bicubic(x, oh, ow, mode == 2, dt)
        got = twice(lambda: run_resize2d(x, oh, ow, mode, dt=dt))
        assert note(f"bicubic {dt}", ratio(got, want, bound)) <= 1, mode


@pytest.mark.parametrize("H,W,oh,ow", R.BICUBIC_SHAPES + R.BICUBIC_VJP_EXTRA)
def test_resize2d_bicubic_vjp(H, W, oh, ow):
    gy = R.normal((2, 3, oh, ow), H * W + oh)
    for align in (0, 1):
        def run():
            gb, out = inp(gy), Buf(2 * 3 * H * W)
            call("maua_resize2d_bicubic_vjp", gb.ptr, out.ptr, 2, 3, H, W, oh, ow, align)
            out.check("bicubic_vjp")
            gb.check("bicubic_vjp input")
            return out.get().reshape(2, 3, H, W)
        want, bound = R.bicubic_vjp(gy, H, W, bool(align))
        assert note("bicubic_vjp", ratio(twice(run), want, bound)) <= 1, align


def test_resize2d_bicubic_vjp_refusals():
    g, out = inp(np.zeros(64)), Buf(64)
    ok = dict(gy=g.ptr, gx=out.ptr, N=1, C=2, H=3, W=4, oh=2, ow=3, align=0)
    for kw in (dict(N=0), dict(C=0), dict(H=0), dict(W=0)):
        call("maua_resize2d_bicubic_vjp", *dict(ok, **kw).values())
    assert out.untouched()
    for kw in (dict(gy=None), dict(gx=None), dict(gx=g.ptr), dict(N=-1), dict(C=-2), dict(N=-1, C=-2), dict(H=-3), dict(W=-4), dict(H=-3, W=-4),
               dict(oh=0), dict(ow=0), dict(oh=-2), dict(ow=-3), dict(oh=-2, ow=-3)):
        refused_with("maua_resize2d_bicubic_vjp", "maua_resize2d_bicubic_vjp", *dict(ok, **kw).values())
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- cutouts and their vjp
CLIP_MEAN, CLIP_STD = (0.48145466, 0.4578275, 0.40821073), (0.26862954, 0.26130258, 0.27577711)


def rect_array(rects):
    return ints([v for r in rects for v in r])


def run_cutouts(img, rects, cs, mul, add, mean, std):
    B, _, H, W = img.shape
    ib, out = inp(img), Buf(len(rects) * B * 3 * cs * cs)
    call("maua_cutouts", ib.ptr, B, H, W, rect_array(rects), len(rects), cs, mul, add, floats(mean), floats(std), out.ptr)
    out.check("cutouts")
    ib.check("cutouts input")
    return out.get().reshape(len(rects) * B, 3, cs, cs)


def run_cutouts_vjp(d_out, B, H, W, rects, cs, mul, std):
    db, out = inp(d_out), Buf(B * 3 * H * W)
    call("maua_cutouts_vjp", db.ptr, B, H, W, rect_array(rects), len(rects), cs, mul, floats(std), out.ptr)
    out.check("cutouts_vjp")
    db.check("cutouts_vjp input")
    return out.get().reshape(B, 3, H, W)


@pytest.mark.parametrize("cs", [8, 32])
def test_cutouts_and_vjp(cs):
    B = 2
    for H, W in R.CUTOUT_IMAGES[cs]:
        rects = R.cutout_rects(cs, H, W)
        img = R.uniform((B, 3, H, W), H + cs, -1.1, 1.1)
        d_out = R.normal((len(rects) * B, 3, cs, cs), W + cs)
        for mul, add, mean, std in ((0.5, 0.5, CLIP_MEAN, CLIP_STD), (1.0, 0.0, (0, 0, 0), (1, 1, 1))):
            want, bound = R.cutouts(img, rects, cs, mul, add, mean, std)
            got = twice(lambda: run_cutouts(img, rects, cs, mul, add, mean, std))
            assert note("cutouts", ratio(got, want, bound)) <= 1, (H, W, mul)
            gw, gb = R.cutouts_vjp(d_out, B, H, W, rects, cs, mul, std)
            grad = twice(lambda: run_cutouts_vjp(d_out, B, H, W, rects, cs, mul, std))
            assert note("cutouts_vjp", ratio(grad, gw, gb)) <= 1, (H, W, mul)
            # the forward is affine in the image: <vjp(d), img> = <d, fwd(img) - fwd(0)>, in float64 within the two bounds
            zero = run_cutouts(np.zeros_like(img), rects, cs, mul, add, mean, std).astype(np.float64)
            zb = R.cutouts(np.zeros_like(img), rects, cs, mul, add, mean, std)[1]
            lhs = float((grad.astype(np.float64) * img).sum())
            rhs = float((d_out.astype(np.float64) * (got.astype(np.float64) - zero)).sum())
            slack = float((gb * np.abs(img)).sum() + ((bound + zb) * np.abs(d_out)).sum())
            assert abs(lhs - rhs) <= slack
            note("cutouts dot identity", abs(lhs - rhs) / max(slack, 1e-300))


@pytest.mark.parametrize("cs", [8, 32])
def test_cutout_tap_tables_bit_for_bit(cs):
    """single-pixel images: image b holds a 1 at (b, b); with the identity affine the vertical pass leaves the weight wy[y][b - left(y)]
    itself and the output at (y, x) is its product with wx[x][b - left(x)], rounded once - predicted from the twin's float32 tables
    (left, taps and the normalised weights)"""
    H, W = R.CUTOUT_IMAGES[cs][1]
    m = min(H, W, 4 * cs - 1)
    assert m == 4 * cs - 1                                 # every size the launcher allows up to 48, every third beyond, and the last three
    sizes = sorted(set(range(1, min(m, 48) + 1)) | set(range(48, m + 1, 3)) | {m - 2, m - 1, m})
    B = max(sizes)
    img = np.zeros((B, 3, H, W), F)
    img[np.arange(B), :, np.arange(B), np.arange(B)] = 1.0
    rects = [(s, 0, 0) for s in sizes]
    got = twice(lambda: run_cutouts(img, rects, cs, 1.0, 0.0, (0, 0, 0), (1, 1, 1))).reshape(len(sizes), B, 3, cs, cs)
    for n, size in enumerate(sizes):
        left, w = R.cutout_tables32(size, cs)
        Wm = np.zeros((cs, B), F)                          # float32 table entries; columns >= size stay zero (outside the cutout)
        for k in range(w.shape[1]):
            idx = left + k
            ok = (idx >= 0) & (idx < size)
            Wm[np.arange(cs)[ok], idx[ok]] = w[ok, k]
        want = Wm.T[:, :, None] * Wm.T[:, None, :]          # [b, y, x] = fl(w[y][b] * w[x][b])
        assert want.dtype == F
        for c in range(3):
            assert same(got[n, :, c], want), (size, c)
        if size == cs:
            assert same(Wm[:, :cs], np.eye(cs, dtype=F)), "size == cut_size: the identity (weights 0, 0, 1, 0)"


def test_cutouts_refusals():
    H, W, cs, B = 31, 29, 8, 2
    img, out, dimg = inp(np.zeros(B * 3 * H * W)), Buf(2 * B * 3 * cs * cs), Buf(B * 3 * H * W)
    good = [(8, 3, 2), (5, 26, 24)]
    m, s = floats((0, 0, 0)), floats((1, 1, 1))

    def fwd(**kw):
        k = dict(dict(img=img.ptr, B=B, H=H, W=W, rects=rect_array(good), n=2, cs=cs, mul=1.0, add=0.0, mean=m, std=s, out=out.ptr), **kw)
        return tuple(k.values())

    def bwd(**kw):
        k = dict(dict(d=img.ptr, B=B, H=H, W=W, rects=rect_array(good), n=2, cs=cs, mul=1.0, std=s, out=dimg.ptr), **kw)
        return tuple(k.values())
    call("maua_cutouts", *fwd(B=0))
    call("maua_cutouts_vjp", *bwd(B=0))
    assert out.untouched() and dimg.untouched()
    many = ints([1, 0, 0] * 65536)
    bad_rects = ([(0, 3, 2)], [(8, 24, 2)], [(8, 3, 22)], [(8, -1, 2)], [(8, 3, -1)], [(30, 0, 0)], [(8 | (1 << 28), 3, 2)], [(8 | (1 << 31) - 2 ** 32, 3, 2)])
    for name, build, nulls in (("maua_cutouts", fwd, ("img", "rects", "mean", "std", "out")), ("maua_cutouts_vjp", bwd, ("d", "rects", "std", "out"))):
        cases = [{k: None} for k in nulls] + [dict(out=img.ptr), dict(B=-1), dict(H=0), dict(H=-31), dict(W=0), dict(W=-29), dict(n=0), dict(n=-2),
                                             dict(cs=0), dict(cs=-8), dict(n=-2, cs=-8), dict(rects=many, n=65536, B=1), dict(rects=many, n=32768, B=2),
                                             dict(cs=7)]                            # min(H, W) = 29 > 4 * 7 - 1
        if name == "maua_cutouts_vjp":
            cases += [dict(B=21846), dict(H=65536)]                                 # the gradient's own grid limits: 3 B and H
        cases += [dict(rects=rect_array(r + good[1:])) for r in bad_rects]
        for kw in cases:
            refused_with(name, name, *build(**kw))
    assert out.untouched() and dimg.untouched()


# ---------------------------------------------------------------------------------------------------------------- colour match
def run_cm_hist(img, H, W, nbins, sat, nan_ok=False):
    B = img.shape[0]
    ib, out = inp(img), Buf(B * nbins)
    call("maua_colormatch_hist", ib.ptr, B, H, W, nbins, sat, out.ptr)
    out.check("colormatch_hist", nan_ok=nan_ok)
    ib.check("colormatch_hist input")
    return out.get().reshape(B, nbins)


def run_cm_grad(img, H, W, nbins, sat, target, scale, nan_ok=False):
    B = img.shape[0]
    ib, tb, grad, loss = inp(img), inp(target), Buf(img.size), Buf(B)
    call("maua_colormatch_grad", ib.ptr, B, H, W, nbins, sat, tb.ptr, int(target.ndim == 2), scale, grad.ptr, loss.ptr)
    grad.check("colormatch_grad", nan_ok=nan_ok)
    loss.check("colormatch loss", nan_ok=nan_ok)
    ib.check("colormatch_grad input")
    tb.check("colormatch target")
    return grad.get().reshape(img.shape), loss.get()


@pytest.mark.parametrize("nbins", R.CM_NBINS + (R.cm_odd_nbins()[0],))
def test_colormatch_hist_of_single_pixel_images_bit_for_bit(nbins):
    px, tags = R.cm_special_pixels(nbins)
    img = px.reshape(-1, 3, 1)
    for sat in (1, 0):
        fix = R.cm_hist_fix(img, nbins, sat)
        assert ((fix > 0).sum(1) <= 2).all(), "two bins at most: the float32 sum S has no order"
        want = R.cm_final32(fix)[2]
        got = twice(lambda: run_cm_hist(img, 1, 1, nbins, sat, nan_ok=True))
        bad = [(tags[b], [(int(i), got[b, i].tobytes().hex(), want[b, i].tobytes().hex()) for i in np.nonzero(got[b] != want[b])[0]])
               for b in range(len(tags)) if not same(got[b], want[b])]
        assert not bad, (sat, bad)


@pytest.mark.parametrize("nbins", R.CM_NBINS + (R.cm_odd_nbins()[0],))
def test_colormatch_hist_and_grad_of_a_random_image(nbins):
    img = R.cm_random_image()
    B, H, W = 3, 37, 53
    for sat in (1, 0):
        fix = R.cm_hist_fix(img, nbins, sat)
        Hs, _S, Hn32 = R.cm_final32(fix)
        Hn = Hs.astype(np.float64) / Hs.astype(np.float64).sum(1, keepdims=True)
        nS = -(-nbins // 256) + 10                          # S: the per-thread sums, the butterfly and the four waves; one division
        got = twice(lambda: run_cm_hist(img, H, W, nbins, sat))
        assert note("colormatch hist", ratio(got, Hn, (nS + 1) * R.U * Hn)) <= 1, sat
        assert same(got, Hn32), "and bit for bit with S restated in the kernel's order (per-thread sums, the butterfly, the four waves)"
        for target in (R.cm_target(nbins, sat, 1)[0], R.cm_target(nbins, sat, B)):
            want, bound, loss, loss_bound = R.cm_grad(img, nbins, sat, target, 1000.0)
            grad, gl = twice(lambda: run_cm_grad(img, H, W, nbins, sat, target, 1000.0))
            assert note("colormatch grad", ratio(grad, want, bound)) <= 1, (sat, target.ndim)
            assert note("colormatch loss", ratio(gl, loss, loss_bound)) <= 1, (sat, target.ndim)


def test_colormatch_all_grey_with_saturation_weighting_is_nan_and_dropped():
    """every weight is 0, so S = 0 and the histogram is 0 / 0: NaN, as the reference's; the gradient holds NaN (through the hue's share
    of the two channels that are not the first maximum) and maua_grad_accumulate drops it"""
    B, H, W, nbins = 2, 5, 7, 64
    img = np.repeat(R.uniform((B, 1, H * W), 3), 3, 1)
    got = run_cm_hist(img, H, W, nbins, 1, nan_ok=True)
    assert np.isnan(got).all() and same(got, R.cm_final32(R.cm_hist_fix(img, nbins, 1))[2])
    target = R.cm_target(nbins, 1, 1)[0]
    want = R.cm_grad(img, nbins, 1, target, 1.0)[0]
    grad, _ = run_cm_grad(img, H, W, nbins, 1, target, 1.0, nan_ok=True)
    assert same(np.isnan(grad), np.isnan(want)) and np.isnan(grad).any() and (grad[~np.isnan(grad)] == 0).all()
    acc0 = R.normal((grad.size,), 9)
    sb, ab = inp(grad), inp(acc0)
    call("maua_grad_accumulate", sb.ptr, ab.ptr, grad.size, 0)
    ab.check("grad_accumulate")
    assert same(ab.get(), acc0)


def test_colormatch_refusals():
    img, out, t = inp(np.zeros(2 * 3 * 4)), Buf(2 * 64), inp(np.full(64, 1 / 64))
    grad, loss = Buf(24), Buf(2)
    call("maua_colormatch_hist", img.ptr, 0, 2, 2, 64, 1, out.ptr)
    call("maua_colormatch_grad", img.ptr, 0, 2, 2, 64, 1, t.ptr, 0, 1.0, grad.ptr, loss.ptr)
    assert out.untouched() and grad.untouched() and loss.untouched()
    shapes = ((-1, 2, 2, 64), (65536, 2, 2, 64), (2, 0, 2, 64), (2, -2, 2, 64), (2, 2, 0, 64), (2, 2, -2, 64), (2, -2, -2, 64), (2, 2, 2, 1), (2, 2, 2, 0),
              (2, 2, 2, -64), (2, 2, 2, 1025), (2, 4096, 4096, 2), (1, 4096, 4097, 3))        # the last two: more than 2^23 (bins - 1) pixels
    for a in [(None, 2, 2, 2, 64, 1, out.ptr), (img.ptr, 2, 2, 2, 64, 1, None)] + [(img.ptr, *sh, 1, out.ptr) for sh in shapes]:
        refused_with("maua_colormatch_hist", "maua_colormatch_hist", *a)
    for a in [(None, 2, 2, 2, 64, 1, t.ptr, 0, 1.0, grad.ptr, loss.ptr), (img.ptr, 2, 2, 2, 64, 1, None, 0, 1.0, grad.ptr, loss.ptr),
              (img.ptr, 2, 2, 2, 64, 1, t.ptr, 0, 1.0, None, loss.ptr), (img.ptr, 2, 2, 2, 64, 1, t.ptr, 0, 1.0, img.ptr, loss.ptr)] + \
             [(img.ptr, *sh, 1, t.ptr, 0, 1.0, grad.ptr, loss.ptr) for sh in shapes]:
        refused_with("maua_colormatch_grad", "maua_colormatch_grad", *a)
    assert out.untouched() and grad.untouched() and loss.untouched()


def test_zz_report():
    for k, v in sorted(WORST.items()):
        print(f"worst error / bound, {k}: {v:.3g}")
