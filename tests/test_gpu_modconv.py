"""The modulated 3x3 convolutions of the StyleGAN2 synthesis forward, every route of csrc/synth.hip's Route enum forced through
maua_modconv_ex (csrc/modconv_api.hip) on one layer with styles and demodulation coefficients chosen here, against float64 references -
the method of tests/test_gpu_conv.py: an integer family whose expected output is exact and compared with torch.equal, guard regions
around every operand and result, and a Gaussian family within a derived element-wise bound.

Integer family.  x, w small integers; styles s in {+-0.5, +-1, +-2} and coefficients d in {0.5, 1, 2}, different per sample and channel;
integer noise with dyadic strength and per-sample scale; integer bias; epilogues of test_gpu_conv.EPIS that the route admits (alpha 0.25 /
0.5, gain 0.5 / 1 / 2, clamp none / 256).  The [1, 3, 3, 1] FIR with gain 4 has taps {1, 3, 9} / 16 (a phase-folded weight sums up to nine w * tap).  Before torch.equal is trusted the CPU
side asserts (Layer.check_exactness): every prepared weight - plain w, the 6 x 6 phase-folded kernel w * F, the half-folded w * g - is
representable in the storage type; every partial sum is a multiple of 2^-k and stays below 2^(24 - k), so f32 accumulation is exact in any
order; float16 never reaches 65504; and where a route rounds an intermediate, that the rounding really changes values.

Rounding points, read from each kernel (T = rounding to the storage type, identity for float32; v = clamp(act(d S + noise + b) gain)):
    Generic (modconv.hip)         operand T(x s) in the kernel; up = 2: weights T(w * F) folded at load time; y = T(v out_scale)
    Lowres (modconv_lowres.hip)   premod kernel T(x s); the same folded weights; f32 partial sums added in slice order; y = T(v)
    DmaConv1 (modconv_dma.hip)    premod pass T(x s) in front; tile T(v); fused toRGB reads T(v); y = T(T(v) out_scale); dual store:
                                  y = T(v), y_scaled = T(T(v) out_scale) - the value is rounded FIRST, then scaled (what a premod pass
                                  over y would write)
    Hires (modconv_hires.hip)     weights T(T(w or w * F) s d gain) in registers, x unscaled; tile T(v); fused toRGB reads T(v)
    Upwalk (modconv_upwalk.hip)   half-folded weights T(w * g); vertical FIR on the f32 accumulators; y = T(v)
    FusedWalk                     ... the up-layer's T(v) feeds conv1 from LDS, conv1's T(v) feeds toRGB; only the image leaves
    Tconv2 / TconvDma / TconvFir  t = T(conv_transpose(x s, w)) (TconvFir: in LDS), FIR + epilogue on T(t); y = T(v out_scale).
                                  TconvDma / TconvFir read T(x s) from a premod pass, Tconv2 forms it in the kernel
    launch_torgb                  f32 sums of x wmod (bf16: wmod split hi + lo on the matrix cores), + bias, clamp, + FIR(prev)
Finding: with out_scale the LDS-direct kernel stores T(T(v) s) and the generic / FIR epilogues T(v s).  They agree for power-of-two styles
(this family) and differ by one rounding otherwise; both are within the Gaussian family's bound, which counts that rounding.

Gaussian family.  Gaussian x (rounded to T), w / (3 sqrt Ci) (rounded to T), styles 1 + N(0, 1), real demodulation coefficients, the
production epilogue (lrelu 0.2, gain sqrt 2, clamp 256), element-wise against float64 within
    2 u |ref| + (9 Ci 2^-24 + n u) A,   A = gain (|d| sum |x s| |w_eff| + |noise term| + |b|)
with n the route's roundings of operands / intermediates beyond the final store (ROUNDINGS below: T(x s); the weight fold; T(w s d g);
T(t), which reaches the output through FIR taps that sum to one; out_scale on a rounded value).  Under a fused toRGB the image is
bounded by sum |wmod| (feature bound) + (Co 2^-24 + 2^-16) sum |feat wmod| + 2^-23 |rgb|: the features' own errors, the f32 sums, and the
bf16 hi + lo split of wmod (w = hi + lo to 2^-16 relative)."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

from maua_amd import _lib as L
from oracle import ops as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTID = {"f32": L.F32, "bf16": L.BF16, "f16": L.F16}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24}
R = L.ROUTES
ACT = {"linear": 0, "relu": 1, "lrelu": 2}
# test_gpu_conv.EPIS: (act, alpha, gain, clamp)
EPIS = [("linear", 1.0, 1.0, -1.0), ("relu", 0.0, 2.0, -1.0), ("lrelu", 0.25, 0.5, 256.0), ("lrelu", 0.5, 1.0, 256.0),
        ("linear", 1.0, 2.0, 256.0), ("relu", 0.0, 0.5, 256.0)]
PROD = ("lrelu", 0.2, math.sqrt(2.0), 256.0)
LRELU_EPIS, NORELU_EPIS = [2, 3], [0, 2, 3, 4]     # launch_tconv_fir: lrelu only; hires / walk: lrelu or linear
SENT16, SENT32, SENT8 = 0x5A5A, 0x5A5A5A5A, 0x5A
G = 4096                                            # guard elements on either side of every buffer
# roundings beyond the final store, per route (up = 1, up = 2):
#   generic / lowres   T(x s)                       + the phase fold T(w * F) on up-layers
#   dma_conv1          T(x s) (premod pass)         + T(v) before out_scale multiplies it (y = T(T(v) s))
#   hires              T(T(w) s d g) (w exact)      + the phase fold on the up-layer
#   upwalk             T(w * g) half fold           + T(x s)
#   tconv*             T(x s)                       + T(t); the FIR's taps are positive and sum to one per output, so T(t)'s u |t| reaches
#                                                     the output as at most u A.  Their epilogue stores T(v s): no further rounding
ROUNDINGS = {"generic": (1, 2), "lowres": (1, 2), "dma_conv1": (2, None), "hires": (1, 2), "upwalk": (None, 2), "tconv2": (None, 2),
             "tconv_dma": (None, 2), "tconv_fir": (None, 2)}
LAUNCHED = set()                                    # (route, tile) of every launch this file made


def _sync():
    torch.cuda.synchronize()


class Buf:
    """a device buffer between guard regions: NaN guards for inputs, a sentinel bit pattern for outputs"""

    def __init__(self, data=None, n=0, dtype=torch.float32):
        if data is not None:
            flat = data.reshape(-1)
            self.full = torch.full((2 * G + flat.numel(),), float("nan"), dtype=flat.dtype, device=DEV)
            self.full[G:G + flat.numel()] = flat.to(DEV)
            self.n, self.out = flat.numel(), False
        else:
            self.full = torch.empty((2 * G + n,), dtype=dtype, device=DEV)
            self.n, self.out = n, True
            self.reset()
        self.ptr = self.full.data_ptr() + G * self.full.element_size()

    def _bits(self):
        return self.full.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[self.full.element_size()])

    def reset(self):
        self._bits().fill_({1: SENT8, 2: SENT16, 4: SENT32}[self.full.element_size()])

    def get(self, n=None):
        return self.full[G:G + (self.n if n is None else n)].cpu()

    def check(self, n=None, what=""):
        """guards intact, (the first n elements of) the body written without NaN"""
        n = self.n if n is None else n
        s = {1: SENT8, 2: SENT16, 4: SENT32}[self.full.element_size()]
        b = self._bits().cpu()
        assert (b[:G] == s).all() and (b[G + n:] == s).all(), f"{what}: a store outside the written region"
        if self.full.is_floating_point():
            assert not torch.isnan(self.full[G:G + n].float()).any(), f"{what}: NaN in the result (a guard region was read)"


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _lsb(t, kmax=40):
    """smallest k with t * 2^k integer-valued everywhere"""
    for k in range(kmax):
        v = t * 2.0 ** k
        if torch.equal(v, v.round()):
            return k
    raise AssertionError("not dyadic")


class Layer:
    """host float64 operands of one modulated layer, its device buffers, its reference under a route's rounding points"""

    def __init__(self, B, H, W, Ci, Co, up=1, dt="bf16", epi=2, flip=0, bias=True, noise="per", demod=True, x_bcast=False, out_scale=False,
                 dual=False, rgb=None, rgb8=False, skip_f32=False, store=True, family="int", seed=0, R_x=None, R_w=None, wm_shift=0, zero=None,
                 s_vals=(-2.0, -1.0, -0.5, 0.5, 1.0, 2.0), d_vals=(0.5, 1.0, 2.0)):
        g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + H * 131 + W * 17 + Ci * 3 + Co + up)
        self.B, self.H, self.W, self.Ci, self.Co, self.up, self.dt, self.tdt, self.family = B, H, W, Ci, Co, up, dt, TDT[dt], family
        self.flip, self.store, self.dual, self.rgb, self.rgb8, self.skip_f32 = flip, store, dual, rgb, rgb8, skip_f32
        self.act, self.alpha, self.gain, self.clamp = EPIS[epi] if isinstance(epi, int) else epi
        Ho, Wo, tdt = H * up, W * up, self.tdt
        self.Ho, self.Wo = Ho, Wo
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
        pick = lambda vals, *s: torch.tensor(vals, dtype=torch.float64)[torch.randint(0, len(vals), s, generator=g)]
        Bx = 1 if x_bcast else B
        if family == "int":
            # operand ranges from the two exactness conditions (asserted in check_exactness): a phase-folded weight is a sum of up to 3 x 3
            # weights times taps {1, 3, 3} x {1, 3, 3} / 16, at most 49 |w| / 16 (|w| <= 5 keeps 245 < 256 in bf16's 8 bits; the transposed
            # convolutions keep plain weights and pass their own range); f16 keeps everything below 65504
            R_x = R_x or (4 if dt == "f16" or up == 2 else 8)
            R_w = R_w or (3 if dt == "f16" and up == 2 else 4 if dt == "f16" else 5 if up == 2 else 8)
            self.x, self.w = ri(-R_x, R_x, Bx, Ci, H, W), ri(-R_w, R_w, Co, Ci, 3, 3)
            self.s = pick(list(s_vals), B, Ci)
            self.d = pick(list(d_vals), B, Co) if demod else None
            self.b = ri(-64, 64, Co) if bias else None
            self.nz = ri(-8, 8, B if noise == "per" else 1, Ho, Wo) if noise else None
            self.nz_strength, self.nz_scale = [0.5, 1.0, 2.0][seed % 3], pick([0.5, 1.0, 2.0], B) if seed % 2 == 0 else None
            self.osc = pick([-2.0, -1.0, -0.5, 0.5, 1.0, 2.0], B, Co) if out_scale else None
            self.wm = ri(-2, 2, B, 3, Co) * 2.0 ** -wm_shift if rgb else None
            self.rb = ri(-4, 4, 3) * 2.0 ** -wm_shift if rgb else None
            self.prev = ri(-16, 16, B, 3, Ho // 2, Wo // 2) * 2.0 ** -wm_shift if rgb == "prev" else None
        else:
            rn = lambda *s: torch.randn(*s, generator=g).double()
            self.x, self.w = rn(Bx, Ci, H, W).to(tdt).double(), (rn(Co, Ci, 3, 3) / (3.0 * Ci ** 0.5)).to(tdt).double()
            self.s = (1.0 + rn(B, Ci)).float().double()
            wmod = self.w[None] * self.s[:, None, :, None, None]
            self.d = ((wmod * wmod).sum((2, 3, 4)) + 1e-8).rsqrt().float().double() if demod else None
            self.b = rn(Co).float().double() if bias else None
            self.nz = rn(B if noise == "per" else 1, Ho, Wo).float().double() if noise else None
            self.nz_strength, self.nz_scale = 0.75, (0.5 + torch.rand(B, generator=g).double()).float().double()
            self.osc = (1.0 + rn(B, Co)).float().double() if out_scale else None
            self.wm = (rn(B, 3, Co) / Co ** 0.5).float().double() if rgb else None
            self.rb = rn(3).float().double() if rgb else None
            self.prev = rn(B, 3, Ho // 2, Wo // 2).float().double() if rgb == "prev" else None
        if zero is not None:
            zero(self)     # a case that keeps only some weights / inputs non-zero
        f32 = lambda t: None if t is None else Buf(t.float())
        self.xd = Buf(_nhwc(self.x).to(tdt))
        self.wd, self.sd, self.dd, self.bd, self.nzd = f32(self.w), f32(self.s), f32(self.d), f32(self.b), f32(self.nz)
        self.nsd, self.oscd, self.wmd, self.rbd, self.prevd = f32(self.nz_scale), f32(self.osc), f32(self.wm), f32(self.rb), f32(self.prev)
        self.y = Buf(n=B * Ho * Wo * Co, dtype=tdt)
        self.ys = Buf(n=B * Ho * Wo * Co, dtype=tdt) if dual else None
        self.t = Buf(n=B * (2 * H + 1) * (2 * W + 1) * Co, dtype=tdt) if up == 2 else None
        self.rgbd = Buf(n=B * 3 * Ho * Wo) if rgb else None
        self.rgb8d = Buf(n=B * Ho * Wo * 3, dtype=torch.uint8) if rgb8 else None

    def desc(self, with_t=False, **kw):
        p = lambda b: b.ptr if b is not None else None
        H, W, up = self.H, self.W, self.up
        d = L.ModconvDesc(x=self.xd.ptr, x_bstride=0 if self.x.shape[0] == 1 and self.B > 1 else H * W * self.Ci, w=self.wd.ptr, flip=self.flip,
                          s=self.sd.ptr, d=p(self.dd), noise=p(self.nzd),
                          noise_bstride=0 if self.nz is None or (self.nz.shape[0] == 1 and self.B > 1) else self.Ho * self.Wo,
                          noise_strength=self.nz_strength, noise_scale=p(self.nsd), bias=p(self.bd), y=self.y.ptr if self.store else None,
                          B=self.B, H=H, W=W, Ci=self.Ci, Co=self.Co, up=up, act=ACT[self.act], alpha=self.alpha, gain=self.gain,
                          clamp=self.clamp, out_scale=p(self.oscd), y_scaled=p(self.ys), rgb_wmod=p(self.wmd), rgb_bias=p(self.rbd),
                          rgb_prev=p(self.prevd), rgb_out=p(self.rgbd), rgb_clamp=256.0, rgb8_out=p(self.rgb8d), rgb_skip_f32=int(self.skip_f32),
                          t=self.t.ptr if with_t and self.t is not None else None)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    # ---- reference
    def T(self, v):
        return v.to(self.tdt).double()

    def xs(self):
        return self.x.expand(self.B, -1, -1, -1) * self.s[:, :, None, None]

    def tconv(self, xs, w):
        wt = w.flip([2, 3]) if self.flip else w
        return F.conv_transpose2d(xs, wt.transpose(0, 1), stride=2)                # [B][Co][2H + 1][2W + 1]

    @staticmethod
    def fir(t):
        return O.upfirdn2d(t, O.setup_filter((1, 3, 3, 1)).double(), padding=(1, 1, 1, 1), gain=4.0)

    def conv(self, xs, w, round_t=False):
        if self.up == 1:
            return F.conv2d(xs, w, padding=1), None
        t = self.tconv(xs, w)
        if round_t:
            t = self.T(t)
        return self.fir(t), t

    def noise_term(self):
        if self.nz is None:
            return 0.0
        sc = self.nz_scale.view(-1, 1, 1, 1) if self.nz_scale is not None else 1.0
        return (self.nz.expand(self.B, -1, -1)[:, None] * self.nz_strength) * sc

    def epilogue(self, v):
        if self.act == "relu":
            v = v.clamp(min=0)
        elif self.act == "lrelu":
            v = torch.where(v > 0, v, v * self.alpha)
        v = v * self.gain
        return v.clamp(-self.clamp, self.clamp) if self.clamp >= 0 else v

    def pre(self, S):
        v = S * self.d[:, :, None, None] if self.d is not None else S
        v = v + self.noise_term()
        return v + self.b.view(1, -1, 1, 1) if self.b is not None else v

    def image(self, feat):
        """toRGB + skip on the rounded features: planar float64 [B][3][Ho][Wo] and its u8 HWC frame"""
        img = torch.einsum("bchw,bkc->bkhw", feat, self.wm) + self.rb.view(1, 3, 1, 1)
        img = img.clamp(-256.0, 256.0)
        if self.prev is not None:
            img = img + O.upsample2d(self.prev, O.setup_filter((1, 3, 3, 1)).double())
        v = ((img.float() + 1.0) / 2.0).clamp(0.0, 1.0) * 255.0
        return img, v.round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def want(self, route, x_in=None):
        """expected results under the route's rounding points (see the module docstring); everything NCHW float64"""
        xs = self.xs() if x_in is None else x_in * self.s[:, :, None, None]
        S, t = self.conv(xs, self.w, round_t=route in ("tconv2", "tconv_dma", "tconv_fir", "upfir"))
        v = self.epilogue(self.pre(S))
        out = {"t": t, "v": v, "S": S}
        feat = self.T(v)
        if self.osc is None:
            out["y"] = feat
        else:
            o = self.osc[:, :, None, None]
            scaled = self.T(feat * o) if route == "dma_conv1" else self.T(v * o)
            out["y"], out["ys"] = (feat, scaled) if self.dual else (scaled, None)
        if self.rgb:
            out["rgb"], out["rgb8"] = self.image(feat)
        return out

    def check_exactness(self, route, w):
        """the conditions under which torch.equal may be trusted (integer family), asserted on the CPU"""
        assert self.family == "int"
        Tq = self.T
        g1 = torch.tensor([1.0, 3.0, 3.0, 1.0], dtype=torch.float64) / 4
        # (a) every prepared weight is representable: plain, half-folded (w * g along x), phase-folded (the 6 x 6 kernel w * F)
        wh = F.conv2d(w.reshape(-1, 1, 3, 3), g1.view(1, 1, 1, 4), padding=(0, 3))
        w6 = F.conv2d(wh, g1.view(1, 1, 4, 1), padding=(3, 0))
        uses = {"plain": self.up == 1 or route in ("tconv2", "tconv_dma", "tconv_fir"), "half-folded": route == "upwalk",
                "phase-folded": self.up == 2 and route in ("generic", "lowres", "hires")}
        for name, k in (("plain", w), ("half-folded", wh), ("phase-folded", w6)):
            if uses[name]:
                assert torch.equal(Tq(k), k) and torch.equal(Tq(k * 8), k * 8) and torch.equal(Tq(k / 8), k / 8), f"{name} weights not representable"
        # (b) partial sums: multiples of 2^-k below 2^(24 - k); the bound on every partial sum is the sum of absolute terms.  k from the
        # operands as the route multiplies them: x s times the (folded) weights, for the weights-in-registers routes times d and the gain
        xs = self.xs()
        assert torch.equal(Tq(xs), xs), "x s not representable"
        A, tA = Layer.conv(self, xs.abs(), w.abs())
        fold = route in ("hires", "upwalk")
        k = _lsb(xs) + _lsb(w6 if self.up == 2 else w) + ((_lsb(self.d) if self.d is not None else 0) + _lsb(torch.tensor(self.gain)) if fold else 0)
        scale = (float(self.d.max()) if self.d is not None else 1.0) * self.gain if fold else 1.0
        assert float(A.max()) * scale * 2.0 ** k < 2.0 ** 24, f"partial sums of S may be inexact: {float(A.max())} 2^{k}"
        if tA is not None:   # t's own sums, and the un-normalised FIR over it (taps 1, 3, 9)
            assert float(tA.max()) * 16 * 2.0 ** (_lsb(xs) + _lsb(w)) < 2.0 ** 24, "partial sums of t may be inexact"
        ref = self.want(route)
        # the epilogue's own values (d S, the pre-activation, the activated value before the clamp) are representable in f32
        Sd = ref["S"] * self.d[:, :, None, None] if self.d is not None else ref["S"]
        pre, cl = self.pre(ref["S"]), self.clamp
        self.clamp = -1.0
        post = self.epilogue(pre)
        self.clamp = cl
        for q in (Sd, pre, post):
            assert float(q.abs().max()) * 2.0 ** _lsb(q) < 2.0 ** 24, "the epilogue may be inexact"
        lim = 65504.0 if self.tdt == torch.float16 else 3.0e38
        assert float(ref["v"].abs().max()) < lim and (ref["t"] is None or float(ref["t"].abs().max()) < lim), "the reference leaves the storage type's range"
        if self.rgb:
            feat = Tq(ref["v"])
            if self.dt == "bf16":   # the features toRGB reads are really rounded, and some of them are ties
                v = ref["v"]
                half = 2.0 ** (torch.floor(torch.log2(v.abs().clamp(min=2.0 ** -60))) - 8)
                assert (feat != v).float().mean() > 0.01, "the features under toRGB are never rounded"
                assert (((feat - v).abs() == half) & (v != 0)).any(), "no feature under toRGB is a rounding tie"
            k = _lsb(feat) + _lsb(self.wm)
            bound = torch.einsum("bchw,bkc->bkhw", feat.abs(), self.wm.abs()).max() + 4 + 16
            assert float(bound) * 2.0 ** k < 2.0 ** 24, "the toRGB sums may be inexact"
        return ref


def _route_call(p, route, d1=None, **kw):
    tile = C.c_int(-1)
    d = p.desc(**kw)
    rc = L.lib().maua_modconv_route(C.byref(d), C.byref(d1) if d1 is not None else None, DTID[p.dt], R[route], C.byref(tile))
    L.check(rc)
    return tile.value


def launch(p, route, d1=None, force_segs=0, narrow_ok=1, **kw):
    tile = _route_call(p, route, d1, **kw)
    d = p.desc(**kw)
    L.check(L.lib().maua_modconv_ex(L.ctx(), C.byref(d), C.byref(d1) if d1 is not None else None, DTID[p.dt], R[route], force_segs, narrow_ok))
    _sync()
    LAUNCHED.add((route, tile if route in ("generic", "dma_conv1") else 0))
    return tile


def _nchw(buf, B, H, W, Cc):
    return buf.get().reshape(B, H, W, Cc).permute(0, 3, 1, 2)


def _same(got, want, what):
    want = want.to(got.dtype)
    if not torch.equal(got, want):
        bad = (got.double() != want.double()).nonzero()
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} values differ, first at {bad[0].tolist()}: got {got[tuple(bad[0])].item()} "
                             f"want {want[tuple(bad[0])].item()}")


def check_outputs(p, ref, what):
    """every output of the layer against the reference, every guard region intact"""
    B, Ho, Wo, Co = p.B, p.Ho, p.Wo, p.Co
    if p.store:
        p.y.check(what=what + " y")
        _same(_nchw(p.y, B, Ho, Wo, Co), ref["y"], what + " y")
    else:
        p.y.check(n=0, what=what + " y (not stored)")
    if p.ys is not None:
        p.ys.check(what=what + " y_scaled")
        _same(_nchw(p.ys, B, Ho, Wo, Co), ref["ys"], what + " y_scaled")
    if p.rgbd is not None:
        if p.skip_f32:
            p.rgbd.check(n=0, what=what + " rgb (skipped)")
        else:
            p.rgbd.check(what=what + " rgb")
            _same(p.rgbd.get().reshape(B, 3, Ho, Wo), ref["rgb"].float(), what + " rgb")
    if p.rgb8d is not None:
        p.rgb8d.check(what=what + " rgb8")
        _same(p.rgb8d.get().reshape(B, Ho, Wo, 3), ref["rgb8"], what + " rgb8")


def run_exact(p, route, want_tile=None, **kw):
    ref = p.check_exactness(route, p.w)
    tile = launch(p, route, **kw)
    if want_tile is not None:
        assert tile == want_tile, f"tile / slices {tile}, expected {want_tile}"
    check_outputs(p, ref, route)
    return ref


# ---------------------------------------------------------------------------------------------------------------- reference sanity (CPU)
def test_reference_is_the_oracles_modulated_convolution():
    """the reference above (x s, then d) against oracle.ops.modulated_conv2d's grouped form (w s, demodulated) on Gaussian operands"""
    for up, flip in ((1, 0), (2, 0), (2, 1)):
        p = Layer(2, 5, 7, 32, 32, up=up, dt="f32", flip=flip, family="gauss", noise=None, bias=False)
        S, _ = p.conv(p.xs(), p.w)
        mine = S * p.d[:, :, None, None]
        f = O.setup_filter((1, 3, 3, 1)).double()
        ref = O.modulated_conv2d(p.x, p.w, p.s, up=up, padding=1, resample_filter=f, demodulate=True, flip_weight=bool(flip))
        # (d here is rounded to float32, as the kernels receive it: 2^-24 relative, with room for the float64 sums)
        assert (mine - ref).abs().max() < 2.0 ** -22 * ref.abs().max(), (up, flip, float((mine - ref).abs().max()))


# ---------------------------------------------------------------------------------------------------------------- Generic
# (dt, B, H, W, Ci, Co, up, tile rule); image sizes that fit no tile, one / two / an odd number of K chunks, every rule styles reach
GENERIC = [
    ("bf16", 2, 5, 7, 32, 32, 1, 9), ("bf16", 3, 16, 16, 64, 128, 1, 1), ("bf16", 2, 33, 17, 96, 128, 1, 6), ("bf16", 2, 64, 64, 64, 128, 1, 2),
    ("bf16", 1, 64, 65, 96, 128, 1, 3), ("bf16", 2, 64, 64, 32, 64, 1, 7), ("bf16", 2, 12, 20, 160, 64, 1, 8), ("f16", 2, 9, 33, 64, 96, 1, 9),
    ("f32", 2, 13, 11, 32, 128, 1, 1), ("f32", 2, 33, 17, 64, 128, 1, 6), ("f16", 2, 33, 17, 96, 256, 1, 6),
    ("bf16", 2, 16, 16, 64, 32, 2, 4), ("bf16", 3, 8, 8, 64, 64, 2, 5), ("bf16", 2, 5, 7, 96, 32, 2, 6), ("bf16", 1, 64, 64, 64, 32, 2, 2),
    ("bf16", 2, 9, 3, 32, 32, 2, 6), ("f16", 2, 7, 12, 64, 32, 2, 5), ("f32", 2, 6, 9, 32, 32, 2, 5), ("bf16", 2, 1, 1, 32, 32, 2, 6),
    ("bf16", 2, 3, 40, 32, 32, 2, 6), ("f32", 2, 64, 64, 32, 32, 2, 2), ("bf16", 1, 64, 64, 96, 32, 2, 3),
]


@pytest.mark.parametrize("i,dt,B,H,W,Ci,Co,up,rule", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(GENERIC)])
def test_generic_exact(i, dt, B, H, W, Ci, Co, up, rule):
    p = Layer(B, H, W, Ci, Co, up, dt, epi=i % len(EPIS), flip=i % 2, bias=i % 4 != 3, noise=[None, "per", "bcast"][i % 3], demod=i % 5 != 4,
              x_bcast=i % 6 == 1, out_scale=up == 2 and i % 2 == 0, seed=i)
    run_exact(p, "generic", want_tile=rule)


def test_generic_fused_torgb_exact():
    for i, (H, W, rgb) in enumerate([(64, 64, "prev"), (18, 16, "noprev"), (16, 18, "prev")]):
        p = Layer(2, H, W, 64, 128, 1, "bf16", epi=NORELU_EPIS[i % 4], rgb=rgb, seed=i, R_x=4, R_w=4)
        run_exact(p, "generic")


# ---------------------------------------------------------------------------------------------------------------- Lowres
# (dt, B, H, W, Ci, Co, up, K slices): H W <= 64, square, non-square, 1 x N; every slice count these geometries produce
LOWRES = [("bf16", 1, 4, 4, 512, 512, 1, 18), ("bf16", 3, 8, 8, 512, 128, 1, 18), ("bf16", 2, 8, 8, 256, 512, 1, 4), ("bf16", 2, 4, 4, 128, 128, 2, 18),
          ("bf16", 3, 1, 7, 320, 128, 1, 45), ("bf16", 2, 5, 12, 64, 32, 2, 9), ("f32", 2, 8, 8, 64, 128, 1, 18), ("f32", 3, 2, 9, 32, 64, 2, 9),
          ("bf16", 2, 8, 8, 128, 512, 2, 2), ("bf16", 1, 1, 64, 64, 128, 1, 9)]


@pytest.mark.parametrize("i,dt,B,H,W,Ci,Co,up,ks", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(LOWRES)])
def test_lowres_exact(i, dt, B, H, W, Ci, Co, up, ks):
    p = Layer(B, H, W, Ci, Co, up, dt, epi=i % len(EPIS), flip=i % 2, bias=i % 4 != 3, noise=[None, "per", "bcast"][(i + 1) % 3], demod=i % 5 != 4,
              x_bcast=i % 3 == 0, seed=i, R_x=2 if Ci >= 256 else None)
    run_exact(p, "lowres", want_tile=ks)


# ---------------------------------------------------------------------------------------------------------------- DmaConv1
# (dt, B, H, W, Ci, Co, tile, out_scale, dual, rgb)
DMA = [("bf16", 2, 8, 32, 64, 128, 128, False, False, None), ("bf16", 3, 16, 64, 128, 256, 256, True, False, None),
       ("bf16", 2, 8, 64, 192, 384, 128, True, True, None), ("bf16", 2, 24, 32, 64, 512, 256, True, True, None),
       ("bf16", 2, 8, 32, 128, 128, 128, True, False, "prev"), ("bf16", 2, 16, 32, 64, 256, 256, True, False, "noprev"),
       ("f16", 2, 8, 32, 64, 128, 128, True, True, None), ("f16", 2, 16, 32, 128, 256, 256, False, False, "prev"),
       ("bf16", 1, 8, 32, 320, 128, 128, True, True, None)]


@pytest.mark.parametrize("i,dt,B,H,W,Ci,Co,tile,osc,dual,rgb", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(DMA)])
def test_dma_conv1_exact(i, dt, B, H, W, Ci, Co, tile, osc, dual, rgb):
    p = Layer(B, H, W, Ci, Co, 1, dt, epi=LRELU_EPIS[i % 2] if rgb else i % len(EPIS), bias=i % 4 != 3, noise=[None, "per", "bcast"][(i + 2) % 3],
              demod=i % 5 != 4, x_bcast=i == 3, out_scale=osc, dual=dual, rgb=rgb, seed=i, R_x=1 if rgb else 4, R_w=2 if rgb else 4)   # (rgb: not saturated at the clamp)
    run_exact(p, "dma_conv1", want_tile=tile)


def test_dual_store_rounds_before_it_scales():
    """y_scaled = T(T(v) s_next), not T(v s_next): pinned with a style of 3 (not a power of two) on values that need rounding"""
    p = Layer(2, 8, 32, 64, 128, 1, "bf16", epi=0, out_scale=True, dual=True, seed=3)
    p.osc = torch.full_like(p.osc, 3.0)
    p.oscd = Buf(p.osc.float())
    ref = p.check_exactness("dma_conv1", p.w)
    once = p.T(ref["v"] * 3.0)
    assert (once != ref["ys"]).any(), "the operands never tell the two orders apart"
    launch(p, "dma_conv1")
    check_outputs(p, ref, "dual store")


# ---------------------------------------------------------------------------------------------------------------- Hires
# (dt, B, H, W, Ci, Co, up, rgb, rgb8, skip_f32, store)
HIRES = [("bf16", 2, 8, 32, 32, 32, 1, None, False, False, True), ("bf16", 2, 16, 64, 32, 32, 1, "prev", False, False, True),
         ("bf16", 3, 8, 96, 32, 32, 1, "noprev", True, False, True), ("bf16", 2, 24, 32, 32, 32, 1, "prev", True, True, False),
         ("bf16", 2, 4, 32, 64, 64, 1, None, False, False, True), ("bf16", 2, 12, 64, 64, 64, 1, "prev", False, False, False),
         ("f16", 2, 8, 32, 64, 64, 1, "noprev", True, False, True), ("bf16", 2, 4, 32, 64, 32, 2, None, False, False, True),
         ("bf16", 3, 12, 64, 64, 32, 2, None, False, False, True), ("f16", 2, 4, 32, 64, 32, 2, None, False, False, True),
         ("f16", 2, 8, 32, 32, 32, 1, "prev", True, True, False)]


@pytest.mark.parametrize("i,dt,B,H,W,Ci,Co,up,rgb,rgb8,skip,store", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(HIRES)])
def test_hires_exact(i, dt, B, H, W, Ci, Co, up, rgb, rgb8, skip, store):
    p = Layer(B, H, W, Ci, Co, up, dt, epi=NORELU_EPIS[i % 4], flip=i % 2, bias=i % 4 != 3, noise=[None, "per", "bcast"][(i + 1) % 3],
              demod=i % 5 != 4, rgb=rgb, rgb8=rgb8, skip_f32=skip, store=store, seed=i, wm_shift=10 if rgb8 else 0)
    ref = run_exact(p, "hires")
    if rgb8:
        assert ((ref["rgb8"] > 0) & (ref["rgb8"] < 255)).float().mean() > 0.05, "the u8 frame is saturated: nothing is tested"


# ---------------------------------------------------------------------------------------------------------------- Upwalk, FusedWalk
UPWALK = [("bf16", 2, 2, 64), ("bf16", 2, 3, 64), ("bf16", 3, 7, 128), ("f16", 2, 5, 64), ("bf16", 1, 33, 192), ("bf16", 2, 16, 64)]


@pytest.mark.parametrize("i,dt,B,H,W", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(UPWALK)])
def test_upwalk_exact(i, dt, B, H, W):
    p = Layer(B, H, W, 64, 32, 2, dt, epi=NORELU_EPIS[i % 4], flip=i % 2, bias=i % 4 != 3, noise=[None, "per", "bcast"][(i + 1) % 3],
              demod=i % 5 != 4, seed=i)
    run_exact(p, "upwalk")


# (dt, B, H, W, force_segs, narrow_ok): one strip (W <= 63), several (126 output columns each), a last strip of <= 32 columns (W = 70,
# 72, 79), H = 2, odd H.  The launcher takes min(force_segs, max(1, H / 32)) segments: H = 99 and 97 run 3 segments of 33 rows (odd, with
# the narrow last strip walked as two half-height sub-items), H = 64 / 65 two, force_segs beyond rows / 2 is clamped
FUSED = [("bf16", 2, 2, 16, 0, 1), ("bf16", 2, 3, 63, 0, 1), ("bf16", 2, 5, 64, 0, 1), ("bf16", 2, 5, 64, 0, 0), ("bf16", 1, 7, 79, 1, 1),
         ("bf16", 1, 64, 70, 2, 1), ("bf16", 1, 65, 70, 2, 0), ("bf16", 1, 99, 70, 3, 1), ("f16", 2, 4, 72, 0, 1), ("bf16", 1, 97, 79, 9, 1),
         ("bf16", 2, 33, 16, 9, 1)]


@pytest.mark.parametrize("i,dt,B,H,W,segs,narrow", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(FUSED)])
def test_fused_walk_exact(i, dt, B, H, W, segs, narrow):
    """conv0 (up) -> conv1 -> toRGB + skip (-> u8) in one walk: the up-layer's rounded output is conv1's input"""
    u8 = i % 2 == 0
    # conv1's input is the up-layer's rounded output.  x in multiples of 32 keeps the up-layer's S (FIR / 16) a multiple of 2, so that with
    # d in {0.5, 1, 2}, integer noise with dyadic strength and an lrelu slope its output is a multiple of 2^-5 of at most 256: really rounded
    # to bf16, and still coarse enough that conv1's sums (weights in {-1, 0, 1}, d in {1, 2}, gain >= 1) stay exact - asserted below
    def coarse(q):
        q.x = q.x * 32
    up = Layer(B, H, W, 64, 32, 2, dt, epi=LRELU_EPIS[i % 2], flip=i % 2, bias=i % 4 != 3, noise=["per", "bcast", None][i % 3], demod=i % 5 != 4,
               seed=i, store=False, R_x=1, R_w=3, zero=coarse)
    c1 = Layer(B, 2 * H, 2 * W, 32, 32, 1, dt, epi=[3, 0][i % 2], bias=i % 3 != 2, noise=[None, "per", "bcast"][i % 3], demod=i % 4 != 3,
               rgb="prev" if i % 3 else "noprev", rgb8=u8, skip_f32=u8 and i % 4 == 0, store=False, seed=100 + i, wm_shift=12 if u8 else 0, R_w=1,
               d_vals=(1.0, 2.0))
    r0 = up.check_exactness("upwalk", up.w)
    c1.x = r0["y"]                                      # conv1 reads the up-layer's output as it would have been stored
    assert (up.T(r0["v"]) != r0["v"]).float().mean() > (0.01 if dt == "bf16" else 0.0), "the up-layer's output is never rounded"
    r1 = c1.check_exactness("hires", c1.w)
    launch(up, "fused_walk", d1=c1.desc(), force_segs=segs, narrow_ok=narrow)
    up.y.check(n=0, what="fused walk: the up-layer's features")
    check_outputs(c1, r1, "fused walk")


# ---------------------------------------------------------------------------------------------------------------- transposed convolutions
def _only(kind):
    """keep a single non-zero input pixel and weight tap so that ONE position class of t's thin edge is pinned on its own"""
    def zero(p):
        x, w = torch.zeros_like(p.x), torch.zeros_like(p.w)
        H, W = p.H, p.W
        # t[2 i + ky][2 j + kx] += x[i][j] w[ky][kx]: the last row of t (2H) takes ky = 2 of input row H - 1, the last column kx = 2
        iy, ix, ky, kx = {"row": (H - 1, W // 3, 2, 1), "col": (H // 3, W - 1, 1, 2), "corner": (H - 1, W - 1, 2, 2)}[kind]
        if p.flip:
            ky, kx = 2 - ky, 2 - kx
        x[:, :, iy, ix], w[:, :, ky, kx] = p.x[:, :, iy, ix], p.w[:, :, ky, kx]
        p.x, p.w = x, w
    return zero


TCONV = [("tconv2", "bf16", 2, 1, 1, 32, 32), ("tconv2", "bf16", 2, 5, 7, 64, 64), ("tconv2", "f32", 2, 4, 9, 32, 32), ("tconv2", "f16", 2, 16, 33, 32, 64),
         ("tconv2", "bf16", 3, 33, 17, 96, 32), ("tconv_dma", "bf16", 2, 8, 32, 32, 32), ("tconv_dma", "bf16", 3, 16, 64, 96, 64),
         ("tconv_dma", "f16", 2, 8, 32, 64, 32), ("tconv_dma", "bf16", 1, 24, 32, 32, 256), ("tconv_fir", "bf16", 2, 16, 32, 32, 32),
         ("tconv_fir", "bf16", 2, 17, 33, 64, 64), ("tconv_fir", "f16", 2, 16, 32, 32, 32), ("tconv_fir", "bf16", 3, 23, 61, 96, 32),
         ("tconv_fir", "bf16", 1, 30, 90, 32, 256)]


@pytest.mark.parametrize("i,route,dt,B,H,W,Ci,Co", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(TCONV)])
def test_transposed_convolution_routes_exact(i, route, dt, B, H, W, Ci, Co):
    epi = LRELU_EPIS[i % 2] if route == "tconv_fir" else i % len(EPIS)
    p = Layer(B, H, W, Ci, Co, 2, dt, epi=epi, flip=i % 2, bias=i % 4 != 3, noise=[None, "per", "bcast"][(i + 1) % 3], demod=i % 5 != 4,
              x_bcast=i % 6 == 1, out_scale=i % 2 == 0, seed=i, R_x=None if dt == "f16" else 8, R_w=None if dt == "f16" else 8)
    ref = run_exact(p, route, with_t=route != "tconv_fir")
    if dt == "bf16" and Ci >= 64:
        unrounded = p.tconv(p.xs(), p.w)
        assert (unrounded != ref["t"]).float().mean() > 0.01, "t is never rounded: the rounding point is not exercised"
    if route != "tconv_fir":   # t itself: every position, the thin last row and column included
        p.t.check(what=route + " t")
        _same(_nchw(p.t, B, 2 * H + 1, 2 * W + 1, Co), ref["t"], route + " t")


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("kind", ["row", "col", "corner"])
@pytest.mark.parametrize("route", ["tconv_dma", "tconv2", "tconv_fir"])
def test_thin_edge_positions_pinned_individually(route, kind, flip):
    p = Layer(2, 16, 32, 32, 64, 2, "bf16", epi=2, flip=flip, noise="per", out_scale=True, seed=7, R_x=8, R_w=8, zero=_only(kind))
    ref = run_exact(p, route, with_t=route != "tconv_fir")
    edge = {"row": ref["t"][:, :, -1, :-1], "col": ref["t"][:, :, :-1, -1], "corner": ref["t"][:, :, -1, -1]}[kind]
    assert (edge != 0).any() and float(ref["t"].abs().sum()) == float(edge.abs().sum()), "the case does not isolate that edge"
    if route != "tconv_fir":
        _same(_nchw(p.t, 2, 33, 65, 64), ref["t"], route + " t")


UPFIR = [("bf16", 2, 1, 1, 8), ("bf16", 3, 5, 7, 40), ("f32", 2, 3, 9, 4), ("f16", 2, 17, 3, 32), ("bf16", 1, 33, 2, 64)]


@pytest.mark.parametrize("i,dt,B,H,W,Co", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(UPFIR)])
def test_upfir_epilogue_alone_exact(i, dt, B, H, W, Co):
    """the FIR / epilogue pass on a given integer t: odd sizes, broadcast noise, out_scale"""
    p = Layer(B, H, W, 32, Co, 2, dt, epi=i % len(EPIS), bias=i % 4 != 3, noise=[None, "per", "bcast"][(i + 1) % 3], demod=i % 5 != 4,
              out_scale=i % 2 == 0, seed=i)
    g = torch.Generator().manual_seed(i)
    t = torch.randint(-300, 301, (B, Co, 2 * H + 1, 2 * W + 1), generator=g).double()
    t = p.T(t) if dt != "f16" else (t / 4).round()
    S = p.fir(t)
    v = p.epilogue(p.pre(S))
    assert float(S.abs().max()) * 16 < 2.0 ** 24 and float(v.abs().max()) * 2.0 ** _lsb(v) < 2.0 ** 24
    want = p.T(v * p.osc[:, :, None, None]) if p.osc is not None else p.T(v)
    tb = Buf(_nhwc(t).to(p.tdt))
    launch(p, "upfir", x=tb.ptr, w=None, s=None)
    p.y.check(what="upfir y")
    _same(_nchw(p.y, B, 2 * H, 2 * W, Co), want, "upfir y")


# ---------------------------------------------------------------------------------------------------------------- toRGB
TORGB = [("bf16", 2, 2, 2, 32, True), ("bf16", 2, 6, 10, 64, False), ("bf16", 3, 8, 8, 128, True), ("bf16", 2, 4, 6, 256, True), ("bf16", 2, 4, 4, 512, True),
         ("f16", 2, 6, 4, 64, True), ("f32", 2, 5, 7, 32, False), ("f32", 2, 4, 4, 512, True), ("bf16", 1, 3, 5, 96, False)]


@pytest.mark.parametrize("i,dt,B,H,W,Cc,prev", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(TORGB)])
def test_torgb_exact(i, dt, B, H, W, Cc, prev):
    g = torch.Generator().manual_seed(i)
    x = torch.randint(-64, 65, (B, Cc, H, W), generator=g).double()
    wm = torch.randint(-4, 5, (B, 3, Cc), generator=g).double() / 2
    rb = torch.randint(-4, 5, (3,), generator=g).double()
    pv = torch.randint(-16, 17, (B, 3, H // 2, W // 2), generator=g).double() if prev else None
    clamp = 256.0
    img = (torch.einsum("bchw,bkc->bkhw", x, wm) + rb.view(1, 3, 1, 1)).clamp(-clamp, clamp)
    assert (img.abs() == clamp).any() or Cc < 128, "the clamp is never active"
    if prev:
        img = img + O.upsample2d(pv, O.setup_filter((1, 3, 3, 1)).double())
    xb, wb, bb, pb = Buf(_nhwc(x).to(TDT[dt])), Buf(wm.float()), Buf(rb.float()), Buf(pv.float()) if prev else None
    out = Buf(n=B * 3 * H * W)
    L.check(L.lib().maua_torgb_ex(L.ctx(), C.c_void_p(xb.ptr), C.c_void_p(wb.ptr), C.c_void_p(bb.ptr), C.c_void_p(pb.ptr if prev else None),
                                  C.c_void_p(out.ptr), B, H, W, Cc, C.c_float(clamp), DTID[dt]))
    _sync()
    LAUNCHED.add(("torgb", 0))
    out.check(what="torgb")
    _same(out.get().reshape(B, 3, H, W), img.float(), "torgb")


# ---------------------------------------------------------------------------------------------------------------- across routes
def test_every_route_of_one_up_layer_gives_the_same_bits():
    """64 -> 32 channels on 16 x 64: every up-route admits it.  The three transposed-convolution routes share their rounding points and
    must agree to the bit (TconvFir = TconvDma + epilogue follows from both meeting one reference); so must the three folded-weight routes"""
    outs = {}
    for route in ("tconv2", "tconv_dma", "tconv_fir", "generic", "hires", "upwalk"):
        p = Layer(2, 16, 64, 64, 32, 2, "bf16", epi=2, noise="per", seed=11, R_x=8, R_w=5)
        run_exact(p, route)
        outs[route] = p.y.get()
    for a, b in (("tconv_dma", "tconv2"), ("tconv_fir", "tconv2"), ("hires", "generic"), ("upwalk", "generic")):
        assert torch.equal(outs[a].view(torch.int16), outs[b].view(torch.int16)), f"{a} differs from {b}"


def test_every_route_of_one_conv1_layer_gives_the_same_bits():
    outs = {}
    for route in ("generic", "dma_conv1"):   # (8 x 32 pixels: more than the split-K route admits; it meets the generic kernel below)
        p = Layer(2, 8, 32, 64, 128, 1, "bf16", epi=3, noise="bcast", seed=12)
        run_exact(p, route)
        outs[route] = p.y.get()
    assert torch.equal(outs["generic"].view(torch.int16), outs["dma_conv1"].view(torch.int16))
    for route in ("generic", "lowres"):
        p = Layer(2, 8, 8, 64, 128, 1, "bf16", epi=3, noise="bcast", seed=13)
        run_exact(p, route)
        outs[route] = p.y.get()
    assert torch.equal(outs["generic"].view(torch.int16), outs["lowres"].view(torch.int16))
    for route in ("generic", "hires"):
        p = Layer(2, 8, 32, 32, 32, 1, "bf16", epi=2, noise="per", seed=14)
        run_exact(p, route)
        outs[route] = p.y.get()
    assert torch.equal(outs["generic"].view(torch.int16), outs["hires"].view(torch.int16))


# ---------------------------------------------------------------------------------------------------------------- Gaussian family
GAUSS = [("generic", "bf16", 2, 33, 17, 160, 128, 1), ("generic", "f16", 2, 33, 17, 160, 128, 1), ("generic", "f32", 2, 33, 17, 160, 128, 1),
         ("generic", "bf16", 2, 9, 13, 96, 64, 2), ("generic", "f32", 2, 9, 13, 96, 64, 2), ("lowres", "bf16", 3, 8, 8, 256, 128, 1),
         ("lowres", "bf16", 2, 4, 4, 128, 128, 2), ("dma_conv1", "bf16", 2, 16, 64, 192, 256, 1), ("dma_conv1", "f16", 2, 16, 64, 192, 256, 1),
         ("hires", "bf16", 2, 8, 32, 64, 64, 1), ("hires", "bf16", 2, 4, 32, 64, 32, 2), ("upwalk", "bf16", 2, 5, 64, 64, 32, 2),
         ("tconv2", "bf16", 2, 9, 13, 96, 64, 2), ("tconv_dma", "bf16", 2, 16, 32, 96, 64, 2), ("tconv_fir", "bf16", 2, 17, 33, 96, 64, 2),
         ("tconv_fir", "f16", 2, 17, 33, 96, 64, 2)]


def _gauss_ref_tol(p, route, osc):
    """float64 reference of the stored features and their element-wise bound (module docstring)"""
    S, _ = p.conv(p.xs(), p.w)
    v = p.epilogue(p.pre(S))
    ref = v * (p.osc[:, :, None, None] if osc else 1.0)
    A, _ = p.conv(p.xs().abs(), p.w.abs())
    A = (A * p.d[:, :, None, None].abs() + p.noise_term().abs() + p.b.abs().view(1, -1, 1, 1)) * p.gain * (p.osc.abs()[:, :, None, None] if osc else 1.0)
    n, u = ROUNDINGS[route][p.up - 1], U[p.dt]
    return ref, 2 * u * ref.abs() + (9 * p.Ci * 2.0 ** -24 + n * u) * A, n


@pytest.mark.parametrize("route,dt,B,H,W,Ci,Co,up", GAUSS, ids=["-".join(map(str, c)) for c in GAUSS])
def test_route_gaussian_within_float64_bound(route, dt, B, H, W, Ci, Co, up):
    osc = route in ("dma_conv1", "tconv2", "tconv_dma", "tconv_fir") or (route == "generic" and up == 2)
    p = Layer(B, H, W, Ci, Co, up, dt, epi=PROD, noise="per", out_scale=osc, family="gauss", seed=1)
    launch(p, route)
    p.y.check(what=route)
    ref, tol, n = _gauss_ref_tol(p, route, osc)
    err = (_nchw(p.y, B, H * up, W * up, Co).double() - ref).abs()
    print(f"{route} {dt} up {up}: {n} roundings, max error {err.max().item():.3e}, largest error / bound {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), f"max excess {(err - tol).max().item()}"


def _rgb_tol(feat, feat_tol, wm, img, prev, Cc):
    """the image's bound: the features' errors through |wmod|, the f32 sums, the bf16 hi + lo split of wmod, the f32 result and skip"""
    mag = torch.einsum("bchw,bkc->bkhw", feat.abs(), wm.abs())
    skip = O.upsample2d(prev.abs(), O.setup_filter((1, 3, 3, 1)).double()) if prev is not None else 0.0
    return torch.einsum("bchw,bkc->bkhw", feat_tol, wm.abs()) + (Cc * 2.0 ** -24 + 2.0 ** -16) * mag + 2.0 ** -22 * (img.abs() + mag + skip + 4.0)


GAUSS_RGB = [("generic", "bf16", 2, 64, 64, 64, 128, "prev"), ("dma_conv1", "bf16", 2, 16, 64, 192, 256, "prev"), ("dma_conv1", "f16", 2, 8, 32, 64, 128, "noprev"),
             ("hires", "bf16", 2, 8, 32, 64, 64, "prev"), ("hires", "bf16", 2, 16, 32, 32, 32, "noprev"), ("hires", "f16", 2, 8, 32, 32, 32, "prev")]


@pytest.mark.parametrize("route,dt,B,H,W,Ci,Co,rgb", GAUSS_RGB, ids=["-".join(map(str, c)) for c in GAUSS_RGB])
def test_fused_torgb_gaussian_within_float64_bound(route, dt, B, H, W, Ci, Co, rgb):
    """Gaussian wmod (its bf16 lo part is not zero) on the rounded features; the image is compared, the stored features too"""
    p = Layer(B, H, W, Ci, Co, 1, dt, epi=PROD, noise="per", rgb=rgb, family="gauss", seed=2)
    launch(p, route)
    p.y.check(what=route)
    p.rgbd.check(what=route + " rgb")
    ref, tol, _ = _gauss_ref_tol(p, route, False)
    err = (_nchw(p.y, B, H, W, Co).double() - ref).abs()
    assert (err <= tol).all()
    img, _ = p.image(ref)
    tol_img = _rgb_tol(ref, tol, p.wm, img, p.prev, Co)
    e = (p.rgbd.get().reshape(B, 3, H, W).double() - img).abs()
    print(f"{route} {dt} fused toRGB: max error {e.max().item():.3e}, largest error / bound {(e / tol_img).max().item():.3f}")
    assert (e <= tol_img).all(), f"max excess {(e - tol_img).max().item()}"


@pytest.mark.parametrize("dt,Cc,prev", [("bf16", 128, True), ("bf16", 512, True), ("bf16", 96, False), ("f16", 64, True), ("f32", 128, True)])
def test_torgb_gaussian_within_float64_bound(dt, Cc, prev):
    """the separate toRGB launch on exact (already rounded) features and Gaussian wmod: only the sums, the split and the f32 result"""
    g = torch.Generator().manual_seed(Cc)
    B, H, W = 2, 6, 10
    x = torch.randn(B, Cc, H, W, generator=g).to(TDT[dt]).double()
    wm, rb = (torch.randn(B, 3, Cc, generator=g) / Cc ** 0.5).double(), torch.randn(3, generator=g).double()
    pv = torch.randn(B, 3, H // 2, W // 2, generator=g).double() if prev else None
    img = (torch.einsum("bchw,bkc->bkhw", x, wm) + rb.view(1, 3, 1, 1)).clamp(-256.0, 256.0)
    if prev:
        img = img + O.upsample2d(pv, O.setup_filter((1, 3, 3, 1)).double())
    tol = _rgb_tol(x, torch.zeros_like(x), wm, img, pv, Cc)
    xb, wb, bb, pb = Buf(_nhwc(x).to(TDT[dt])), Buf(wm.float()), Buf(rb.float()), Buf(pv.float()) if prev else None
    out = Buf(n=B * 3 * H * W)
    L.check(L.lib().maua_torgb_ex(L.ctx(), C.c_void_p(xb.ptr), C.c_void_p(wb.ptr), C.c_void_p(bb.ptr), C.c_void_p(pb.ptr if prev else None),
                                  C.c_void_p(out.ptr), B, H, W, Cc, C.c_float(256.0), DTID[dt]))
    _sync()
    out.check(what="torgb")
    e = (out.get().reshape(B, 3, H, W).double() - img).abs()
    print(f"torgb {dt} C {Cc}: max error {e.max().item():.3e}, largest error / bound {(e / tol).max().item():.3f}")
    assert (e <= tol).all(), f"max excess {(e - tol).max().item()}"


# ---------------------------------------------------------------------------------------------------------------- the forward's plan
LOW, GEN, DMA1, HIR, UPW, FUS, DONE, TFIR, TDMA, T2 = range(10)
KERNEL, PRODUCER, XM, PREMOD = range(4)


def _net(res=1024, dt="bf16"):
    h = C.c_void_p()
    L.check(L.lib().maua_synth_create(L.ctx(), res, 512, 32768, 512, DTID[dt], 0, C.byref(h)))
    return h


def _plan(h, want_u8):
    n = C.c_int(0)
    conv, rgb, pack = (C.c_int * (7 * 32))(), (C.c_int * 16)(), C.c_int(-1)
    L.check(L.lib().maua_synth_get_plan(h, int(want_u8), conv, 32, rgb, C.byref(pack), C.byref(n)))
    nb = (n.value + 1) // 2
    return [list(conv[7 * i:7 * i + 7]) for i in range(n.value)], list(rgb[:nb]), pack.value


def _bench_plan(dt, want_u8):
    """(route, src, scale_next, dual, rgb, rgb8, skip_store) per conv layer of bench.py's network (1024^2, w_dim 512, channel_base 32768,
    channel_max 512): b4.conv1, then conv0 / conv1 of b8 .. b1024"""
    low = LOW if dt == "bf16" else GEN                    # the split-K GEMM has no float16 form
    u8 = int(want_u8)
    return [[low, KERNEL, 0, 0, 0, 0, 0]] * 4 + [
        [GEN, KERNEL, 0, 0, 0, 0, 0],                     # b16.conv1
        [GEN, KERNEL, 1, 0, 0, 0, 0],                     # b32.conv0: four phase kernels, output scaled for the LDS-direct conv1
        [DMA1, PRODUCER, 1, 1, 0, 0, 0],                  # b32.conv1: 512 channels, toRGB separate -> dual store
        [TDMA, XM, 1, 0, 0, 0, 0],                        # b64.conv0
        [DMA1, PRODUCER, 1, 1, 0, 0, 0],                  # b64.conv1
        [TDMA, XM, 1, 0, 0, 0, 0],                        # b128.conv0
        [DMA1, PRODUCER, 1, 0, 1, 0, 0],                  # b128.conv1: 256 channels, toRGB fused, features stored scaled
        [TDMA, PRODUCER, 1, 0, 0, 0, 0],                  # b256.conv0
        [DMA1, PRODUCER, 1, 0, 1, 0, 0],                  # b256.conv1
        [TFIR, PRODUCER, 0, 0, 0, 0, 0],                  # b512.conv0: 256^2 input, t stays in LDS
        [HIR, KERNEL, 0, 0, 1, 0, 0],                     # b512.conv1
        [FUS, KERNEL, 0, 0, 0, 0, 1],                     # b1024.conv0: the whole last block as one walk
        [DONE, KERNEL, 0, 0, 1, u8, 1]], [0, 0, 0, 0, 0, 1, 1, 1, 1], 0


@pytest.mark.parametrize("want_u8", [False, True])
@pytest.mark.parametrize("dt", ["bf16", "f16"])
def test_benchmark_network_plan(dt, want_u8):
    """the routing of the network bench.py measures: a threshold edit that moves it off its fast kernels is a diff of this table.
    The routes are those of a kernel trace of one forward of this network on the commit before maua_synth_get_plan existed (bf16 and f16,
    f32 and u8 output): three split-K launches per layer for the first four layers (f16: generic kernels), generic <4,1,2,1,9,64> and
    <4,4,2,1,3,128>, four LDS-direct conv1 launches (three 256-channel tiles, one 128), three edge + main + FIR / epilogue triples, one
    tconv_fir, one hires <64,64,1>, one fused walk; five separate toRGB launches (blocks 4 .. 64), no premod pass, no u8 pack launch"""
    h = _net(1024, dt)
    try:
        got = _plan(h, want_u8)
        want = _bench_plan(dt, want_u8)
        assert got[0] == want[0], "\n".join(f"{i}: got {g} want {w}" for i, (g, w) in enumerate(zip(got[0], want[0])) if g != w)
        assert got[1:] == (want[1], want[2]), got[1:]
    finally:
        L.lib().maua_synth_destroy(h)


@pytest.mark.parametrize("res,dt", [(32, "bf16"), (256, "bf16"), (256, "f16"), (128, "f32")])
def test_plan_is_the_same_before_and_after_a_forward(res, dt):
    """maua_synth_get_plan predicts, on a net without a workspace, whether the premod buffer will exist; after a forward it reads it"""
    h = _net(res, dt)
    try:
        before = [_plan(h, u8) for u8 in (False, True)]
        nws = L.lib().maua_synth_num_ws(h)
        ws = torch.zeros(2, nws, 512, device=DEV)
        img = torch.empty(2, 3, res, res, device=DEV)
        L.check(L.lib().maua_synth_forward(h, C.c_void_p(ws.data_ptr()), None, None, 2, C.c_void_p(img.data_ptr())))
        _sync()
        assert [_plan(h, u8) for u8 in (False, True)] == before
        assert any(c[3] for c in before[0][0]) == (res >= 256 and dt != "f32"), "the dual store goes with the premod buffer"
    finally:
        L.lib().maua_synth_destroy(h)


OPTION_SETS = [dict(), dict(use_hires=0), dict(upwalk=0), dict(upwalk=1), dict(tconv_up=0), dict(tconv_up=1 << 20), dict(tconv_dma=0),
               dict(tconv_fir=0), dict(tconv_fir=32), dict(dma_conv=0), dict(dual_store=0), dict(fuse_torgb=0), dict(lowres=0),
               dict(keep_features=1), dict(use_hires=0, fuse_torgb=0, dma_conv=0), dict(resize=9), dict(resize=16), dict(warp=13), dict(warp=17)]


@pytest.mark.parametrize("opts", OPTION_SETS, ids=["-".join(f"{k}{v}" for k, v in o.items()) or "default" for o in OPTION_SETS])
@pytest.mark.parametrize("dt", ["bf16", "f16", "f32"])
def test_plan_invariants(dt, opts):
    lib = L.lib()
    h = _net(1024, dt)
    keep = []
    try:
        for k, v in opts.items():
            if k == "resize":      # a stretch hook behind layer v (1-based): 1.5 x the native grid, even sizes
                hh, ww = C.c_int(), C.c_int()
                L.check(lib.maua_synth_layer_size(h, v - 1, C.byref(hh), C.byref(ww)))
                L.check(lib.maua_synth_set_resize(h, v, 0, hh.value * 3 // 2, ww.value * 3 // 2, 0, 0, 0, 0, 3, C.c_float(0.0), None))
            elif k == "warp":
                m = torch.tensor([[1.0, 0, 0, 0, 1, 0]], device=DEV)
                keep.append(m)
                L.check(lib.maua_synth_set_warp(h, 0, v, C.c_void_p(m.data_ptr())))
            else:
                L.check(lib.maua_synth_set_option(h, k.encode(), v))
        hooked = {opts.get("resize"), opts.get("warp")} - {None}
        nl = lib.maua_synth_num_layers(h)
        for want_u8 in (False, True):
            conv, rgb, pack = _plan(h, want_u8)
            assert len(conv) == nl == 17 and len(rgb) == 9
            for i, (route, src, scale_next, dual, frgb, rgb8, skip) in enumerate(conv):
                if src in (PRODUCER, XM):
                    assert i > 0 and conv[i - 1][2], f"layer {i} reads scaled input that layer {i - 1} does not write"
                    assert (src == XM) == bool(conv[i - 1][3]), f"layer {i}: Xm goes with the producer's dual store"
                if scale_next:
                    assert conv[i + 1][1] in (PRODUCER, XM), f"layer {i} scales its output for a layer that does not expect it"
                assert not dual or scale_next
                assert (route == DONE) == (i > 0 and conv[i - 1][0] == FUS), f"layer {i}: WalkDone only follows FusedWalk"
                if skip:
                    assert not opts.get("keep_features") and (i + 1) not in hooked and (route != FUS or (i + 2) not in hooked), f"layer {i}: features dropped that something reads"
                    assert route in (FUS, DONE) or frgb
                if rgb8:
                    assert frgb and want_u8 and i == nl - 1
                if frgb:
                    assert rgb[(i + 1) // 2] == 1, f"layer {i}: fused toRGB in a block whose toRGB is not Fused"
                if dt == "f32":
                    assert route in (LOW, GEN, T2), f"layer {i}: float32 has no route {route}"
                # the route's own launcher accepts the layer's shape
                hh, ww = C.c_int(), C.c_int()
                L.check(lib.maua_synth_layer_size(h, i, C.byref(hh), C.byref(ww)))
                if route != DONE and i not in hooked and (i + 1) not in hooked and not any(k <= i for k in hooked):
                    res = 4 << ((i + 1) // 2)
                    up = 2 if i % 2 == 1 else 1
                    ci, co = min(32768 // (res // up), 512), min(32768 // res, 512)
                    # ... with the flags of the step itself: out_scale, the dual store, the fused toRGB (+ u8), features not stored
                    rgbkw = dict(rgb_wmod=0x700000, rgb_bias=0x800000, rgb_prev=0xC00000 if i > 0 else None, rgb_out=0x900000, rgb_clamp=256.0)
                    d = L.ModconvDesc(x=0x100000, x_bstride=(res // up) ** 2 * ci, w=0x200000, s=0x300000, d=0x400000, bias=0x500000,
                                      y=None if skip and route == HIR else 0x600000, B=2, H=res // up, W=res // up, Ci=ci, Co=co, up=up, act=2,
                                      alpha=0.2, gain=2 ** 0.5, clamp=256.0, out_scale=0xA00000 if scale_next else None,
                                      y_scaled=0xB00000 if dual else None, rgb8_out=0xD00000 if rgb8 and route == HIR else None,
                                      **(rgbkw if frgb and route != DONE else {}))
                    d1 = L.ModconvDesc(x=0x100000, x_bstride=res * res * co, w=0x200000, s=0x300000, y=0x600000, B=2, H=res, W=res, Ci=co, Co=co,
                                       up=1, act=2, alpha=0.2, gain=2 ** 0.5, clamp=256.0, rgb8_out=0xD00000 if conv[i + 1][5] else None,
                                       rgb_skip_f32=0, **rgbkw) if route == FUS else None
                    rc = lib.maua_modconv_route(C.byref(d), C.byref(d1) if d1 is not None else None, DTID[dt], route, None)
                    assert rc == 0, f"layer {i} planned on route {route}, which refuses it: {lib.maua_last_error().decode()}"
            assert bool(pack) == (want_u8 and not any(c[5] for c in conv)), "the u8 frame is packed once: in an epilogue or by its own launch"
            assert all((r == 1) == any(c[4] for c in conv[max(2 * b - 1, 0):2 * b + 1]) for b, r in enumerate(rgb) if r != 2)
    finally:
        lib.maua_synth_destroy(h)


# ---------------------------------------------------------------------------------------------------------------- coverage
def test_zz_every_route_and_tile_was_launched():
    """runs last in this file: no route (for Generic / DmaConv1: no tile) is covered in name only.  Reads a module-level record of the
    launches, so it needs the whole file run in one process (no -k selection, no test distribution across workers)"""
    want = {(r, 0) for r in ("lowres", "hires", "upwalk", "fused_walk", "tconv_fir", "tconv_dma", "tconv2", "upfir", "torgb")}
    want |= {("generic", t) for t in range(1, 10)} | {("dma_conv1", 128), ("dma_conv1", 256)}
    assert LAUNCHED == want, f"missing {sorted(want - LAUNCHED)}, unexpected {sorted(LAUNCHED - want)}"
