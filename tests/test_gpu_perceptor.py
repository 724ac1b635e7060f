"""The VGG / LPIPS perceptor kernels of csrc/perceptor.hip - vgg_conv0 and its two adjoint kernels, maxpool2 / maxpool2_vjp, mask_add,
gram_partial / gram_reduce, style_dsum / style_dgram, lpips_head / lpips_norm, rows_sum, features_out, zero_f32 - through the C ABI
(maua_vgg_*) on tiny plans that put each kernel behind at most two convolutions, against the float64 restatement in
tests/perceptor_ref.py.  The method of tests/test_gpu_groupnorm.py and tests/test_gpu_modconv.py: a family whose expected result is
exact and compared bit for bit (np.array_equal on the float32 values read back), guard regions around every tensor the test owns
(NaN around images, targets and lin weights, a sentinel pattern around grad, loss and the features / gram / lpips-features
outputs), a Gaussian family inside a derived element-wise bound with no element left out, and a closing report.
tests/test_perceptor_host.py proves on the CPU what both families rest on.

No tie allowance is needed: ReLU's mask and the pool's argmax are functions of the STORED activations, which maua_vgg_features
returns exactly (pooling entries too), so the reference backward fed the device's activations is the same linear map as the device's;
the forward is pinned layer by layer, each layer's reference fed the device's stored input.

Exact family (perceptor_ref.exact_case).  The image is chosen so that ((img * 0.5 + 0.5) - mean) / std is an integer in [-1, 1] (mean
dyadic, std powers of two: 1.f / std and mul * istd exact); weights in {-1, 0, 1}, biases in {-1, 0}: activations are small integers,
whole pixels zero after ReLU, most pooling windows tied in every position order.  The style head gets T = G - D0 with D0 a sparse
non-symmetric integer matrix with a transposed pair, a diagonal entry and zeros, sum |D0| a power of two and strength = C^2: A0 + 1e-8f
== A0, k = 1, and loss, Sym = dG + dG^T, the head gradient F Sym, every masked sum and adjoint and the image gradient are dyadic
numbers whose float32 partial sums are exact in any order - bit for bit in f32 and, every stored intermediate being representable
(asserted per case on the CPU), in bf16.  Per-sample and shared targets, two taps with unrelated D0, loss returned and loss == NULL.

Gaussian family.  Gaussian image, He-scaled Gaussian weights rounded to their storage type.  Rounding points, read from each kernel
(v = 2^-24, u = the storage unit; perceptor_ref's *_bound functions restate each line):
    vgg_conv0        x' = (img mul + add - mean) istd in float32, 27 products + sums onto the bias, ReLU, the store
    convolutions     the MFMA kernels of modconv.hip / modconv_dma.hip at unit styles: test_gpu_modconv's bound with n = 0
    maxpool2         no arithmetic: compared bit for bit on the device's own input
    gram             float32 products, <= 256 per slice in a running sum, then the slices in order
    lpips_norm       C / 64 squares per lane + 6 shuffle additions, sqrt, + 1e-10f, one division
    style head       D = G - T; Q, A as float32 chunk sums; Sym in about eight operations, stored in the network type (a sign that |D|
                     cannot decide inside its own error is allowed for); the head GEMM (C float32 terms), stored
    lpips head       the norm as above; d, w d^2 and its sums; gv = 2 w d coef; the projection sum; k2; gv / re - f k2, stored
    rows_sum         a thread's run of hw / 1024 values, the wave's shuffles, 16 wave sums, the mul, the +=
    backward         mask_add: one addition and the store where both gradients meet, nothing otherwise; maxpool2_vjp: none; the
                     transposed convolution: the MFMA bound on the incoming error and value; conv0's adjoint: a float32 run of at
                     most 36 Co products, the factor mul * (1.f / std), the product
No term is measured: every one is derived from the code, and there is no margin on top."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import perceptor_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
DTID = {"f32": L.F32, "bf16": L.BF16}
SENT32 = 0x5A5A5A5A
G = 4096                                            # guard elements on either side of every buffer
WORST = {}                                          # family -> worst error / bound seen (test_zz_report prints it)
ROUTES = set()                                      # (kernel route, dtype) the convolutions took, as run_conv's condition reads
SAME_BITS = []                                      # LDS-direct and generic gradients bit-identical? (reported, not asserted)


def _sync():
    torch.cuda.synchronize()


class Buf:
    """a float32 device buffer between guard regions: NaN guards for inputs, a sentinel bit pattern for outputs"""

    def __init__(self, data=None, n=0):
        if data is not None:
            flat = torch.from_numpy(np.ascontiguousarray(data, dtype=np.float64).reshape(-1))
            assert torch.equal(flat.float().double(), flat), "operands must be representable in float32"
            self.full = torch.full((2 * G + flat.numel(),), float("nan"), dtype=torch.float32, device=DEV)
            self.full[G:G + flat.numel()] = flat.float().to(DEV)
            self.n = flat.numel()
        else:
            self.full = torch.empty((2 * G + n,), dtype=torch.float32, device=DEV)
            self.n = n
            self.full.view(torch.int32).fill_(SENT32)
        self.ptr = C.c_void_p(self.full.data_ptr() + G * 4)

    def get(self, what):
        """guards intact, every element written, no NaN: the body as float64 numpy"""
        b = self.full.view(torch.int32).cpu()
        assert (b[:G] == SENT32).all() and (b[G + self.n:] == SENT32).all(), f"{what}: a store outside the buffer"
        assert (b[G:G + self.n] != SENT32).all(), f"{what}: elements of the result were never written"
        body = self.full[G:G + self.n].cpu()
        assert not torch.isnan(body).any(), f"{what}: NaN in the result (a guard region was read)"
        return body.double().numpy()

    def untouched(self):
        return bool((self.full.view(torch.int32) == SENT32).all())


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), float(r))


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.isfinite(err).all()
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0


def conv_route(dt, Ci, Co, h, w, no_dma):
    """run_conv's choice, restated: the LDS-direct kernel for bf16 on 8 x 32 tiles (wide: Co % 128 == 0 on whole tiles; narrow: Co == 64)"""
    if dt == "bf16" and not no_dma and Ci % 64 == 0:
        if Co % 128 == 0 and h % 8 == 0 and w % 32 == 0:
            return "dma wide"
        if Co in (32, 64) and h >= 8 and w >= 32:
            return "dma narrow"
    return "generic"


class Net:
    """one maua_vgg handle on a (plan, params, pre, replicate) network of perceptor_ref"""

    def __init__(self, net, dt, no_dma=False):
        self.plan, self.params, self.pre, self.replicate = net
        self.dt, self.no_dma = dt, no_dma
        mul, add, mean, std = self.pre
        h = C.c_void_p()
        L.check(L.lib().maua_vgg_create(L.ctx(), DTID[dt], (C.c_int * len(self.plan))(*self.plan), len(self.plan), int(self.replicate),
                                        C.c_float(mul), C.c_float(add), (C.c_float * 3)(*mean), (C.c_float * 3)(*std), C.byref(h)))
        self.h = h
        for k, (w, b) in enumerate(self.params):
            for what, a in ((0, w), (1, b)):
                a32 = np.ascontiguousarray(a, dtype=np.float32)
                assert np.array_equal(a32.astype(np.float64), a)
                L.check(L.lib().maua_vgg_load(self.h, k, what, a32.ctypes.data_as(C.c_void_p), C.c_size_t(a32.size)))

    def close(self):
        if self.h is not None:
            L.lib().maua_vgg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def grid(self, op):
        s = sum(1 for c in self.plan[:op + 1] if c == 0)
        return self.H >> s, self.W >> s

    def channels(self, op):
        return next(c for c in reversed(self.plan[:op + 1]) if c)

    def forward(self, img):
        self.B, _, self.H, self.W = img.shape
        self.img = Buf(img)
        L.check(L.lib().maua_vgg_forward(self.h, self.img.ptr, self.B, self.H, self.W))
        _sync()
        cin = 3
        for i, c in enumerate(self.plan):
            if c and i:
                ROUTES.add((conv_route(self.dt, cin, c, *self.grid(i - 1), self.no_dma), self.dt))
            cin = c or cin

    def features(self, op):
        h, w = self.grid(op)
        out = Buf(n=self.B * self.channels(op) * h * w)
        L.check(L.lib().maua_vgg_features(self.h, op, out.ptr))
        _sync()
        return out.get(f"features[{op}]").reshape(self.B, self.channels(op), h, w)

    def acts(self):
        return [self.features(i) for i in range(len(self.plan))]

    def gram(self, op):
        c = self.channels(op)
        out = Buf(n=self.B * c * c)
        L.check(L.lib().maua_vgg_gram(self.h, op, out.ptr))
        _sync()
        return out.get(f"gram[{op}]").reshape(self.B, c, c)

    def lpips_features(self, op):
        """[B][C][h][w] (the library's layout is [B][h w][C])"""
        h, w = self.grid(op)
        c = self.channels(op)
        out = Buf(n=self.B * c * h * w)
        L.check(L.lib().maua_vgg_lpips_features(self.h, op, out.ptr))
        _sync()
        return out.get(f"lpips_features[{op}]").reshape(self.B, h, w, c).transpose(0, 3, 1, 2)

    def _grad(self, fn, img, taps, targets, extra, scalar, want_loss):
        self.B, _, self.H, self.W = img.shape
        self.img = Buf(img)
        tb = [Buf(t) for t in targets]
        grad, loss = Buf(n=img.size), Buf(n=self.B)
        strides = [0 if t.shape[0] == 1 else t[0].size for t in targets]
        n = len(taps)
        L.check(fn(self.h, self.img.ptr, self.B, self.H, self.W, (C.c_int * n)(*taps), n, (C.c_void_p * n)(*[t.ptr.value for t in tb]),
                   (C.c_long * n)(*strides), *extra, C.c_float(scalar), grad.ptr, loss.ptr if want_loss else None))
        _sync()
        assert want_loss or loss.untouched()
        return grad.get("grad").reshape(img.shape), loss.get("loss") if want_loss else None

    def style_grad(self, img, taps, targets, strength, want_loss=True):
        """targets: [C][C] (shared) or [B][C][C] per tap"""
        return self._grad(L.lib().maua_vgg_style_grad, img, taps, [t if t.ndim == 3 else t[None] for t in targets], (), strength, want_loss)

    def lpips_grad(self, img, taps, targets, lins, scale, want_loss=True):
        """targets: unit-normalised [Bt][C][h][w] per tap (Bt = 1: shared); lins: [C] per tap"""
        lb = [Buf(w) for w in lins]
        nhwc = [np.ascontiguousarray(t.transpose(0, 2, 3, 1)) for t in targets]
        return self._grad(L.lib().maua_vgg_lpips_grad, img, taps, nhwc, ((C.c_void_p * len(lb))(*[b.ptr.value for b in lb]),), scale, want_loss)


def regions(got, want, bound=None):
    """the worst corner / edge / interior pixel, for a failure message"""
    out = []
    for name, m in R.region_masks(*want.shape[2:]).items():
        if m.any():
            err = np.abs(got - want)[:, :, m]
            out.append(f"{name}: {int((err > (0 if bound is None else bound[:, :, m])).sum())} of {err.size} off, worst {err.max():.3e}")
    return "; ".join(out)


# ---------------------------------------------------------------------------------------------------------------- exact family
def run_exact(i, dt):
    d = R.exact_case(R.EXACT_CASES[i])
    net = Net(d["net"], dt)
    img, plan = d["img"], d["net"][0]
    net.forward(img)
    for op, want in enumerate(d["acts"]):
        got = net.features(op)
        assert np.array_equal(got, want), f"stored activation {op} ({'pool' if plan[op] == 0 else 'conv'}): {regions(got, want)}"
    for op in d["taps"]:
        assert np.array_equal(net.gram(op), R.gram(d["acts"][op])), f"gram of entry {op}"
    grad, loss = net.style_grad(img, d["taps"], d["targets"], d["strength"])
    assert np.array_equal(loss, d["loss"]), (loss, d["loss"])
    assert np.array_equal(grad, d["grad"]), f"image gradient: {regions(grad, d['grad'])}"
    grad2, _ = net.style_grad(img, d["taps"], d["targets"], d["strength"], want_loss=False)     # loss == NULL, and the handle again
    assert np.array_equal(grad2, grad), "a second call on the same handle differs"
    net.close()
    note(f"exact {dt}", 0.0)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(R.CONV0_CASES)))
def test_exact_conv0(i, dt):
    """vgg_conv0 and vgg_conv0_vjp64 (Co = 64) / vgg_conv0_vjp (Co = 128): both paddings, 1 x 1 to 9 x 17, B = 1 and 3"""
    run_exact(i, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(R.POOL_CASES)))
def test_exact_pool(i, dt):
    """maxpool2 and maxpool2_vjp on tied windows: the first maximum in row-major order takes the gradient"""
    run_exact(len(R.CONV0_CASES) + i, dt)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("i", range(len(R.MASK_CASES)))
def test_exact_mask_add_and_ping_pong(i, dt):
    """mask_add with no gradient from above, with no head gradient, with both; five layers of the ga / gb ping-pong"""
    if len(R.CONV0_CASES) + len(R.POOL_CASES) + i in R.EXACT_F32_ONLY and dt == "bf16":
        pytest.fail("not representable in bf16: the case belongs to the bounded family")
    run_exact(len(R.CONV0_CASES) + len(R.POOL_CASES) + i, dt)


# ---------------------------------------------------------------------------------------------------------------- Gaussian family
def check_forward(net, ref_net, img, dt):
    """every stored activation against its layer's float64 reference on the device's own stored input; returns them"""
    plan, params, pre, replicate = ref_net
    acts = net.acts()
    ci = R.conv_of(plan)
    for i, c in enumerate(plan):
        if c == 0:
            assert np.array_equal(acts[i], R.maxpool2(acts[i - 1])), f"pool entry {i}"
            note(f"maxpool2 {dt} (exact)", 0.0)
        elif i == 0:
            ref = R.conv0(img, pre, *params[0], replicate)
            b = R.conv0_bound(img, pre, *params[0], replicate, ref, dt)
            r = ratio(acts[0], ref, b)
            note(f"vgg_conv0 {dt}", r)
            assert r <= 1, f"conv0: {regions(acts[0], ref, b)}"
        else:
            w, bias = params[ci[i]]
            ref = np.maximum(R.conv3x3(acts[i - 1], w, bias), 0.0)
            r = ratio(acts[i], ref, R.conv_bound(acts[i - 1], w, bias, ref, dt))
            note(f"convolution {dt}", r)
            assert r <= 1, f"conv entry {i}"
    return acts


def style_targets(acts, taps, B, seed):
    """Gaussian targets around the features' own Gram matrices (float32 values), per sample and shared in turn"""
    rng = np.random.default_rng(seed)
    out = []
    for j, e in enumerate(taps):
        Gm = R.gram(acts[e])
        T = Gm * (1 + 0.5 * rng.normal(size=Gm.shape)) + rng.normal(size=Gm.shape) * (np.abs(Gm).mean() + 1e-3)
        out.append((T if (j + seed) % 2 == 0 else T[0]).astype(np.float32).astype(np.float64))
    return out


def lpips_targets(acts, taps, B, seed):
    rng = np.random.default_rng(seed)
    nts, lins = [], []
    for j, e in enumerate(taps):
        _, Cc, h, w = acts[e].shape
        nt = R.lpips_normalize(np.abs(rng.normal(size=(B if (j + seed) % 2 == 0 else 1, Cc, h, w))))
        nts.append(nt.astype(np.float32).astype(np.float64))
        lins.append((rng.random(Cc) / Cc).astype(np.float32).astype(np.float64))
    return nts, lins


def check_style(net, ref_net, img, acts, taps, dt, seed, want_loss=True):
    B = img.shape[0]
    targets = style_targets(acts, taps, B, seed)
    grad, loss = net.style_grad(img, taps, targets, 2.5, want_loss)
    heads, hb, ref_loss, eloss = {}, {}, np.zeros(B), np.zeros(B)
    for e, T in zip(taps, targets):
        _, _, heads[e] = R.style_head(acts[e], T, 2.5)
        l, el, hb[e] = R.style_bounds(acts[e], T, 2.5, dt)
        ref_loss, eloss = ref_loss + l, eloss + el
    want, bound = R.backward_with_bound(ref_net, acts, heads, hb, dt)
    if want_loss:
        r = ratio(loss, ref_loss, eloss + len(taps) * R.V * np.abs(ref_loss))
        note(f"style loss {dt}", r)
        assert r <= 1, (loss, ref_loss, eloss)
    r = ratio(grad, want, bound)
    note(f"style gradient {dt}", r)
    assert r <= 1, f"style gradient: {regions(grad, want, bound)}"
    return grad, bound


def check_lpips(net, ref_net, img, acts, taps, dt, seed):
    B = img.shape[0]
    nts, lins = lpips_targets(acts, taps, B, seed)
    grad, dist = net.lpips_grad(img, taps, nts, lins, 3.0)
    heads, hb, ref_dist, edist = {}, {}, np.zeros(B), np.zeros(B)
    for e, nt, lin in zip(taps, nts, lins):
        _, dd, heads[e] = R.lpips_head(acts[e], nt, lin, 3.0)
        _, ed, hb[e] = R.lpips_bounds(acts[e], nt, lin, 3.0, dt)
        ref_dist, edist = ref_dist + dd, edist + ed
    want, bound = R.backward_with_bound(ref_net, acts, heads, hb, dt)
    assert np.isfinite(want).all() and np.isfinite(grad).all() and np.isfinite(dist).all()
    r = ratio(dist, ref_dist, edist + len(taps) * R.V * np.abs(ref_dist))
    note(f"lpips distance {dt}", r)
    assert r <= 1, (dist, ref_dist, edist)
    r = ratio(grad, want, bound)
    note(f"lpips gradient {dt}", r)
    assert r <= 1, f"lpips gradient: {regions(grad, want, bound)}"
    return grad, bound


def check_heads_forward(net, acts, taps, dt):
    for e in taps:
        r = ratio(net.gram(e), R.gram(acts[e]), R.gram_bound(acts[e]))
        note(f"gram {dt}", r)
        assert r <= 1, f"gram of entry {e}"
        n = R.lpips_normalize(acts[e])
        r = ratio(net.lpips_features(e), n, R.norm_bound(acts[e]) * np.abs(n))
        note(f"lpips_norm {dt}", r)
        assert r <= 1, f"lpips features of entry {e}"


def run_gauss(plan, B, H, W, replicate, taps, dt, seed, no_dma=False):
    ref_net = (list(plan), R.gaussian_params(plan, dt, seed), R.GAUSS_PRE, replicate)
    img = R.gaussian_image(B, H, W, seed)
    net = Net(ref_net, dt, no_dma)
    net.forward(img)
    acts = check_forward(net, ref_net, img, dt)
    check_heads_forward(net, acts, taps, dt)
    out = (check_style(net, ref_net, img, acts, taps, dt, seed, want_loss=seed % 3 != 0), check_lpips(net, ref_net, img, acts, taps, dt, seed))
    net.close()
    return out


GAUSS_CONV0 = [(C0, rep, H, W, (1, 3)[(j + rep) % 2]) for C0 in (64, 128) for rep in (0, 1) for j, (H, W) in enumerate(((1, 1), (1, 7), (3, 5), (9, 17)))]


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("C0,rep,H,W,B", GAUSS_CONV0)
def test_gaussian_conv0(C0, rep, H, W, B, dt):
    run_gauss((C0,), B, H, W, rep, [0], dt, seed=H * 100 + W + C0 + rep)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Cc,B,H,W", [(64, 1, 2, 2), (64, 3, 6, 10), (64, 2, 16, 32), (128, 2, 6, 10), (128, 1, 16, 32)])
def test_gaussian_pool(Cc, B, H, W, dt):
    run_gauss((Cc, 0, Cc), B, H, W, 1, [2], dt, seed=Cc + H)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("plan,taps,B,H,W", [((64, 64), [1], 2, 3, 5), ((64, 64, 0, 64, 64), [1, 4], 2, 4, 6), ((64, 64, 0, 64, 64), [1, 4], 3, 8, 12),
                                             ((128, 128), [0, 1], 1, 2, 2)])
def test_gaussian_mask_add_and_ping_pong(plan, taps, B, H, W, dt):
    run_gauss(plan, B, H, W, 0, taps, dt, seed=len(plan) + H)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
@pytest.mark.parametrize("Cc", [64, 128, 512])
@pytest.mark.parametrize("H,W", [(1, 1), (15, 17), (16, 16), (1, 257), (24, 25)])
def test_gaussian_gram_and_heads(H, W, Cc, dt):
    """hw in {1, 255, 256, 257, 600}: gram_partial's tail slice and S > 1; C = 64 (style_dsum's chunks shorter than a block), 128
    (off-diagonal tiles), 512; pixel counts that are no multiple of 4 for the lpips head"""
    run_gauss((Cc,), 1 if Cc == 512 else 3, H, W, 1, [0], dt, seed=H * W + Cc)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_gaussian_rows_sum_above_1024(dt):
    """rows_sum with more than one value per thread (hw = 1056); every other case has hw < 1024"""
    run_gauss((64,), 2, 33, 32, 0, [0], dt, seed=9)


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_lpips_head_at_zero_feature_vectors(dt):
    """the exact family's integer network has pixels whose features are all zero: distance and gradient equal the closed form (the
    projection term 0 there) inside the Gaussian family's bounds, and are finite"""
    d = R.exact_case(R.CONV0_CASES[7])
    assert (d["acts"][0].max(1) == 0).any()
    net = Net(d["net"], dt)
    net.forward(d["img"])
    acts = net.acts()
    assert np.array_equal(acts[0], d["acts"][0])
    check_heads_forward(net, acts, [0], dt)
    check_lpips(net, d["net"], d["img"], acts, [0], dt, seed=0)
    net.close()


@pytest.mark.parametrize("plan", [(64, 128), (128, 64), (64, 64)])
def test_gaussian_convolution_routes(plan, monkeypatch):
    """bf16 on a 16 x 32 grid: the LDS-direct convolution (wide and narrow tiles, forward and transposed), and again on the generic
    kernel (MAUA_VGG_NO_DMA=1 read when the handle is created): each inside its own bound, the two inside the sum of their bounds"""
    res = []
    for no_dma in (False, True):
        if no_dma:
            monkeypatch.setenv("MAUA_VGG_NO_DMA", "1")
        else:
            monkeypatch.delenv("MAUA_VGG_NO_DMA", raising=False)
        res.append(run_gauss(plan, 2, 16, 32, 1, [1], "bf16", seed=plan[0] + plan[1], no_dma=no_dma))
    assert (conv_route("bf16", plan[0], plan[1], 16, 32, False), "bf16") in ROUTES and conv_route("bf16", plan[0], plan[1], 16, 32, False) != "generic"
    for k, what in enumerate(("style", "lpips")):
        r = ratio(res[0][k][0], res[1][k][0], res[0][k][1] + res[1][k][1])
        note(f"LDS-direct against generic, {what} gradient", r)
        SAME_BITS.append(bool(np.array_equal(res[0][k][0], res[1][k][0])))
        assert r <= 1


# ---------------------------------------------------------------------------------------------------------------- one handle
@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_one_handle_through_several_shapes(dt):
    """One handle walked through shapes that shrink, grow and keep B H W while needing more Gram slices (B = 3 at 16 x 16, then B = 2
    at 16 x 24: 4 slices of 256 pixels where 3 were allocated), through the Gram, style and lpips entry points: every result is bit for
    bit the result of a fresh handle on the same input.  (The second shape was refused with "gram workspace too small" while
    ensure_ws keyed the partials' size on B H W; it now sizes them from what each shape needs.)"""
    plan = (64,)
    ref_net = (list(plan), R.gaussian_params(plan, dt, 5), R.GAUSS_PRE, True)
    one = Net(ref_net, dt)
    for j, (B, H, W) in enumerate([(3, 16, 16), (2, 16, 24), (1, 8, 8), (4, 4, 4), (2, 16, 24), (1, 24, 32), (3, 16, 16)]):
        img = R.gaussian_image(B, H, W, 50 + j)
        fresh = Net(ref_net, dt)
        outs = []
        for net in (one, fresh):
            net.forward(img)
            acts = net.acts()
            gm = net.gram(0)
            T = style_targets(acts, [0], B, j)
            nts, lins = lpips_targets(acts, [0], B, j)
            outs.append((acts[0], gm, *net.style_grad(img, [0], T, 2.5), *net.lpips_grad(img, [0], nts, lins, 3.0), net.gram(0)))
        fresh.close()
        for k, (a, b) in enumerate(zip(*outs)):
            assert np.array_equal(a, b), f"shape {j} {(B, H, W)}: result {k} differs from a fresh handle's"
    one.close()


def test_unit_styles_grow_with_the_batch():
    """float32, plan (64, 64): the second convolution and its gradient run on the generic kernel, which multiplies its input by the
    handle's unit styles [B][512].  One handle at B = 1, 3, 1 (16 x 16): the buffer is filled at the first forward, regrown at the
    second, kept at the third - features and style gradient are bit for bit a fresh handle's each time.  (The shapes above stop at
    conv0, which reads no styles.)"""
    plan = (64, 64)
    ref_net = (list(plan), R.gaussian_params(plan, "f32", 6), R.GAUSS_PRE, False)
    assert conv_route("f32", 64, 64, 16, 16, False) == "generic"
    one = Net(ref_net, "f32")
    for j, B in enumerate((1, 3, 1)):
        img = R.gaussian_image(B, 16, 16, 70 + j)
        fresh = Net(ref_net, "f32")
        outs = []
        for net in (one, fresh):
            net.forward(img)
            acts = net.acts()
            outs.append((acts[1], *net.style_grad(img, [1], style_targets(acts, [1], B, j), 2.5)))
        fresh.close()
        for k, (a, b) in enumerate(zip(*outs)):
            assert np.array_equal(a, b), f"B = {B} (step {j}): result {k} differs from a fresh handle's"
        assert np.abs(outs[0][0]).max() > 0 and np.abs(outs[0][1]).max() > 0
    one.close()


def test_refusals_write_nothing():
    """a pooling entry is no tap; H, W must divide by the pooling; B == 0 returns at once: grad and loss stay untouched"""
    ref_net = ([64, 0, 64], R.gaussian_params((64, 0, 64), "f32", 1), R.GAUSS_PRE, False)
    net = Net(ref_net, "f32")
    img, T = Buf(R.gaussian_image(1, 4, 4, 1)), Buf(np.zeros((64, 64)))
    grad, loss = Buf(n=48), Buf(n=1)
    call = lambda B, H, W, tap: L.lib().maua_vgg_style_grad(net.h, img.ptr, B, H, W, (C.c_int * 1)(tap), 1, (C.c_void_p * 1)(T.ptr.value),   # noqa: E731
                                                            (C.c_long * 1)(0), C.c_float(1.0), grad.ptr, loss.ptr)
    assert call(1, 4, 4, 1) == -1 and "a tap must be a convolution" in L.lib().maua_last_error().decode()
    assert call(1, 3, 4, 0) == -1 and "multiples of 2" in L.lib().maua_last_error().decode()
    assert call(0, 4, 4, 0) == 0
    _sync()
    assert grad.untouched() and loss.untouched()
    net.close()


def test_zz_report():
    """the worst error / bound per family and the convolution routes taken"""
    for k in sorted(WORST):
        print(f"[perceptor] worst error / bound, {k}: {WORST[k]:.3f}")
    print(f"[perceptor] convolution routes taken: {sorted(ROUTES)}; LDS-direct and generic gradients bit-identical in "
          f"{sum(SAME_BITS)} of {len(SAME_BITS)} comparisons")
    assert all(v <= 1 for v in WORST.values())
    if len(WORST) < 12:     # (a single test was selected: the coverage below is a statement about the whole file)
        return
    for t in (("dma wide", "bf16"), ("dma narrow", "bf16"), ("generic", "bf16"), ("generic", "f32")):
        assert t in ROUTES, f"{t} was never taken"
