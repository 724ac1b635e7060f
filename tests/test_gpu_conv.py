"""The three kernels behind every plain 3x3 convolution (csrc/modconv.hip generic, csrc/modconv_dma.hip LDS-direct, csrc/modconv_lowres.hip
split-K gather GEMM), each forced through maua_conv3x3_ex and through the UNet's routing, against float64 references at their edges:
image sizes that fit no tile, one / two / an odd number of K chunks, every tile rule, channel-sliced operands, one and two residuals,
the virtual x2 up-sampling, partly read K, overhanging narrow tiles, every K-slice count of the gather GEMM, the piece sums.

Main family: integer operands in [-8, 8] (float16: [-6, 6], so that no value of the reference reaches 65504 - asserted), integer
biases in [-64, 64], epilogues that keep integers dyadic (linear / relu / lrelu 0.25, 0.5; gain 1, 2, 0.5; clamp none / 256; res_gain 1,
0.5, -2).  With Ci <= 2048 every partial sum stays below 2^21, so the f32 accumulation is exact in any tap, chunk and slice order and the
expected output is exact, compared with torch.equal.  |S| often exceeds 256, so bf16's rounding (ties included) really runs.

Rounding points, read from the three epilogues (T = rounding to the storage type, the identity for float32 / split float32):
    v = clamp(act(S + b) * gain)                 in f32 (lrelu / linear fold the gain: act((S + b) * gain), the same value here)
    y = T(v)                                     no residual
    y = T(T(v) + res)                            res joins the value as it would have been stored, then the store rounds again
    y = T(res_gain * T(T(v) + res) + res2)       res2 joins what would have been stored after res
The LDS-direct kernel always computed this (its residuals are added to the rounded epilogue tile); the generic kernel and the gather
epilogue added res to the unrounded f32 value - T(v + res) - until this file found the three apart; they now round first.

Guard regions: x sits between NaN guard rows (a whole tile row of the tallest tile on either side) and, with x_pstride > Ci, NaN
channels; y is filled with a sentinel pattern that must survive in the guard rows and outside [y_coff, y_coff + Co); the result must
hold no NaN.  Samples differ and are adjacent, so a halo read that strays into a neighbour reads valid integers and the exact
comparison catches it.

Second family: Gaussian operands, element-wise against float64 within 2u |ref| + 9 Ci 2^-24 (|x| * |w| + |b|), doubled with a
residual (plus the rounding of the value the residual joins), as tests/test_gpu_gemm.py.  The split-float32 products have no derivable
constant: the exact-f32 kernel's measured error against float64 on the same inputs, times 4 (three rounded partial products
instead of one), is the split kernel's bound - test_split_f32_gaussian records the measured figures."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from maua_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
TDT = {"f32": torch.float32, "split": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
DTID = {"f32": L.F32, "split": L.F32_SPLIT, "bf16": L.BF16, "f16": L.F16}
SENT = {torch.bfloat16: 0x5A5A, torch.float16: 0x5A5A, torch.float32: 0x5A5A5A5A}
IVIEW = {torch.bfloat16: torch.int16, torch.float16: torch.int16, torch.float32: torch.int32}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11, "f32": 2.0 ** -24, "split": 2.0 ** -24}
IRANGE = {"bf16": 8, "f32": 8, "split": 8, "f16": 6}    # integer family: operands in [-IRANGE, IRANGE]
ACT = {"linear": 0, "relu": 1, "lrelu": 2}
GENERIC, DMA, GATHER = 1, 2, 3
# epilogues of the integer family (all exact): (act, alpha, gain, clamp)
EPIS = [("linear", 1.0, 1.0, -1.0), ("relu", 0.0, 2.0, -1.0), ("lrelu", 0.25, 0.5, 256.0), ("lrelu", 0.5, 1.0, 256.0),
        ("linear", 1.0, 2.0, 256.0), ("relu", 0.0, 0.5, 256.0)]
RES_GAINS = [1.0, 0.5, -2.0]


def _bits(t):
    return t.view(IVIEW[t.dtype])


def _sync():
    torch.cuda.synchronize()


def _guard_rows(W):
    """rows of the tallest tile any kernel lays over an image this wide (generic kernel: 256 pixels in rows of 32 / 16 / 8 / 4)"""
    tw = 32 if W > 16 else 16 if W > 8 else 8 if W > 4 else 4
    return 256 // tw


def _rnd(v, tdt):
    return v.to(tdt).double()


class Problem:
    """host float64 operands, device buffers with guard regions, the exact / float64 reference of one convolution"""

    def __init__(self, B, H, W, Ci, Co, dt="bf16", epi=0, bias=True, res=0, xpad=0, ypad=0, ycoff=0, rpad=0, Ci_read=0, x_up2=False,
                 family="int", seed=0, irange=None, brange=64):
        g = torch.Generator().manual_seed(seed * 1000003 + B * 7919 + H * 131 + W * 17 + Ci * 3 + Co)
        tdt = TDT[dt]
        R = IRANGE[dt] if irange is None else irange
        if family == "int":
            draw = lambda *s: torch.randint(-R, R + 1, s, generator=g).double()
            bdraw = lambda n: torch.randint(-brange, brange + 1, (n,), generator=g).double()
        else:
            draw = lambda *s: torch.randn(*s, generator=g).to(tdt).double()
            bdraw = lambda n: torch.randn(n, generator=g).float().double()
        self.B, self.H, self.W, self.Ci, self.Co, self.dt, self.tdt, self.family = B, H, W, Ci, Co, dt, tdt, family
        self.act, self.alpha, self.gain, self.clamp = EPIS[epi] if isinstance(epi, int) else epi
        self.n_res, self.res_gain = res, RES_GAINS[seed % 3] if res == 2 else 1.0
        self.Ci_read, self.x_up2 = Ci_read, x_up2
        hs, ws = (H // 2, W // 2) if x_up2 else (H, W)
        self.x = draw(B, Ci, hs, ws)
        self.w = draw(Co, Ci, 3, 3)
        if family != "int":
            self.w = self.w / (3.0 * Ci ** 0.5)
            self.w = self.w.float().double() if tdt == torch.float32 else _rnd(self.w, tdt)
        # channels that are never fetched (whole 32-channel chunks past Ci_read, at least two are read) hold NaN; every channel past Ci_read has
        # zero weights, so the ones between Ci_read and the chunk boundary are read and multiplied by zero
        self.ci_fetched = Ci if not Ci_read else max(64, (Ci_read + 31) // 32 * 32)
        if Ci_read:
            self.w[:, Ci_read:] = 0
        self.b = bdraw(Co) if bias else None
        self.r = draw(B, Co, H, W) if res >= 1 else None
        self.r2 = draw(B, Co, H, W) if res == 2 else None
        self.xps, self.yps, self.ycoff, self.rps = Ci + xpad, Co + ypad + ycoff, ycoff, Co + rpad
        self.gr = _guard_rows(W)
        self.xd = self._nhwc(self.x, self.xps, hs, ws, self.ci_fetched)
        self.wd = self.w.float().to(DEV).contiguous()
        self.bd = self.b.float().to(DEV) if bias else None
        self.rd = self._nhwc(self.r, self.rps, H, W, Co) if res >= 1 else None
        self.r2d = self._nhwc(self.r2, self.rps, H, W, Co) if res == 2 else None
        self.y = self.new_y()
        self.psum = None

    def _nhwc(self, t, ps, h, w, c_valid):
        """device NHWC copy of host NCHW t between NaN guard rows, ps channels per pixel, NaN past c_valid"""
        gpx = self.gr * w
        buf = torch.full((2 * gpx + self.B * h * w, ps), float("nan"), dtype=self.tdt, device=DEV)
        v = t.permute(0, 2, 3, 1).reshape(self.B * h * w, t.shape[1])[:, :c_valid]
        buf[gpx:gpx + self.B * h * w, :c_valid] = v.to(self.tdt).to(DEV)
        return buf

    def new_y(self):
        y = torch.empty((2 * self.gr * self.W + self.B * self.H * self.W, self.yps), dtype=self.tdt, device=DEV)
        _bits(y).fill_(SENT[self.tdt])
        return y

    def _ptr(self, buf, w):
        return buf.data_ptr() + self.gr * w * buf.shape[1] * buf.element_size()

    def desc(self, y=None, B=None, b0=0, **kw):
        """the descriptor of samples [b0, b0 + B)"""
        y = self.y if y is None else y
        H, W = self.H, self.W
        hs, ws = (H // 2, W // 2) if self.x_up2 else (H, W)
        es = y.element_size()
        d = L.ConvDesc(x=self._ptr(self.xd, ws) + b0 * hs * ws * self.xps * es, x_pstride=self.xps, x_bstride=hs * ws * self.xps,
                       w=self.wd.data_ptr(), bias=self.bd.data_ptr() if self.bd is not None else None,
                       y=self._ptr(y, W) + b0 * H * W * self.yps * es, y_pstride=self.yps, y_coff=self.ycoff, y_bstride=H * W * self.yps,
                       res=self._ptr(self.rd, W) + b0 * H * W * self.rps * es if self.rd is not None else None, res_pstride=self.rps,
                       res_bstride=H * W * self.rps,
                       res2=self._ptr(self.r2d, W) + b0 * H * W * self.rps * es if self.r2d is not None else None,
                       res2_pstride=self.rps, res2_bstride=H * W * self.rps, res_gain=self.res_gain,
                       B=self.B if B is None else B, H=H, W=W, Ci=self.Ci, Co=self.Co, act=ACT[self.act], alpha=self.alpha,
                       gain=self.gain, clamp=self.clamp, Ci_read=self.Ci_read, x_up2=int(self.x_up2), variant=0,
                       psum=self.psum.data_ptr() if self.psum is not None else None)
        if self.xps == self.Ci and not kw.get("keep_strides"):
            d.x_pstride = 0    # dense operands go in the way the UNet passes them
        kw.pop("keep_strides", None)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    # ---- references
    def x_seen(self):
        x = self.x.clone()
        if self.Ci_read:
            x[:, self.Ci_read:] = 0
        return F.interpolate(x, scale_factor=2, mode="nearest") if self.x_up2 else x

    def pre(self):
        """S + b in float64"""
        s = F.conv2d(self.x_seen(), self.w, padding=1)
        return s + self.b.view(1, -1, 1, 1) if self.b is not None else s

    def epilogue(self, v):
        if self.act == "relu":
            v = v.clamp(min=0)
        elif self.act == "lrelu":
            v = torch.where(v > 0, v, v * self.alpha)
        v = v * self.gain
        return v.clamp(-self.clamp, self.clamp) if self.clamp >= 0 else v

    def want(self):
        """exact expected output (integer family), NCHW in the storage type; asserts that nothing on the way leaves the type's range"""
        T = lambda t: _rnd(t, self.tdt)
        lim = 65504.0 if self.tdt == torch.float16 else 3.0e38
        stages = [self.epilogue(self.pre())]
        if self.r is not None:
            stages.append(T(stages[-1]) + self.r)
        if self.r2 is not None:
            stages.append(self.res_gain * T(stages[-1]) + self.r2)
        assert max(float(s.abs().max()) for s in stages) < lim, "the reference leaves the storage type's range: shrink the operands"
        return stages[-1].to(self.tdt)

    def got(self, y=None):
        y = self.y if y is None else y
        gpx = self.gr * self.W
        v = y[gpx:gpx + self.B * self.H * self.W, self.ycoff:self.ycoff + self.Co]
        return v.reshape(self.B, self.H, self.W, self.Co).permute(0, 3, 1, 2).cpu()

    def check_guards(self, y=None, B=None):
        y = self.y if y is None else y
        n = (self.B if B is None else B) * self.H * self.W
        gpx = self.gr * self.W
        assert not torch.isnan(y[gpx:gpx + n, self.ycoff:self.ycoff + self.Co].float()).any(), \
            "NaN in the result: a kernel read a guard row, a channel outside its slice or an unread channel"
        bits = _bits(y).cpu()
        s = SENT[self.tdt]
        assert (bits[:gpx] == s).all() and (bits[gpx + n:] == s).all(), "a store outside the samples (guard rows)"
        assert (bits[:, :self.ycoff] == s).all() and (bits[:, self.ycoff + self.Co:] == s).all(), "a store outside the channel slice"

    def check_exact(self, y=None, want=None):
        got, want = self.got(y), self.want() if want is None else want
        if not torch.equal(got, want):
            bad = (got.double() != want.double()).nonzero()
            raise AssertionError(f"{len(bad)} of {got.numel()} outputs differ, first at [b, co, y, x] = {bad[0].tolist()}: "
                                 f"got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}")

    def gauss_err_tol(self, y=None):
        """Gaussian family: (error, bound) element-wise against float64"""
        sb = self.epilogue(self.pre())
        ref = sb + self.r if self.r is not None else sb
        mag = F.conv2d(self.x_seen().abs(), self.w.abs(), padding=1) + (self.b.abs().view(1, -1, 1, 1) if self.b is not None else 0)
        u = U[self.dt]
        tol = 2 * u * ref.abs() + 9 * self.Ci * 2.0 ** -24 * mag
        if self.r is not None:
            tol = 2 * tol + (2 * u * sb.abs() if self.tdt != torch.float32 else 0)
        return (self.got(y).double() - ref).abs(), tol


def launch(p, kernel, **kw):
    return L.lib().maua_conv3x3_ex(L.ctx(), C.byref(p.desc(**kw)), DTID[p.dt], kernel)


def run(p, kernel, **kw):
    L.check(launch(p, kernel, **kw))
    _sync()


def route(p, opt, **kw):
    """(kernel, variant, ksplit) maua_conv3x3_route reports: opt 0 / 1 / 2 the UNet's routing, 100 + k the forced kernel k"""
    v, ks = C.c_int(-1), C.c_int(-1)
    k = L.lib().maua_conv3x3_route(C.byref(p.desc(**kw)), DTID[p.dt], opt, C.byref(v), C.byref(ks))
    L.check(min(k, 0))
    return k, v.value, ks.value


def refusal(p, kernel, **kw):
    """the text a forced kernel refuses with ("" if it launched), and that nothing was written"""
    rc = launch(p, kernel, **kw)
    msg = "" if rc == 0 else L.lib().maua_last_error().decode()
    _sync()
    assert (_bits(p.y).cpu() == SENT[p.tdt]).all(), "a refused call launched"
    return msg


def run_exact(p, kernel, want_variant=None, want_ksplit=None, **kw):
    k, v, ks = route(p, 100 + kernel, **kw)
    assert k == kernel
    if want_variant is not None:
        assert v == want_variant, f"tile {v}, expected {want_variant}"
    if want_ksplit is not None:
        assert ks == want_ksplit, f"{ks} K slices, expected {want_ksplit}"
    _bits(p.y).fill_(SENT[p.tdt])
    run(p, kernel, **kw)
    p.check_guards()
    p.check_exact()
    return v


# ---------------------------------------------------------------------------------------------------------------- the generic kernel
# launch_modconv3x3's tile rules as maua_conv3x3_route numbers them.  With up == 1 rule 1 (H W <= 256, Co % 128 == 0) shadows rules 4 and 5,
# so a plain convolution reaches 1, 2, 3, 6, 7, 8, 9 - six instantiations (1 and 9 share one), all but the 128 x 128 / 128-byte one of rule 5 -
# and float32 / split float32 never reach rule 3 (Ci % 32 == 0 is a whole 128-byte chunk there).
GENERIC_RULES = {"bf16": {1, 2, 3, 6, 7, 8, 9}, "f16": {1, 2, 3, 6, 7, 8, 9}, "f32": {1, 2, 6, 7, 8, 9}, "split": {1, 2, 6, 7, 8, 9}}
SIZES = [(5, 7), (33, 17), (12, 20), (1, 1), (1, 40), (16, 16), (64, 64)]
G_CI, G_CO = [32, 64, 96, 160], [32, 64, 96, 128, 256]
SLICES = [dict(), dict(xpad=32, ypad=64, ycoff=32, rpad=32), dict(xpad=64, ypad=32, rpad=64)]


def _generic_rule(dt, H, W, Ci, Co):
    """the rule the source takes, restated (and confirmed per case through maua_conv3x3_route)"""
    k128 = Ci % (64 if dt in ("bf16", "f16") else 32) == 0
    hw = H * W
    if hw <= 256 and Co % 128 == 0:
        return 1
    if Co % 128 == 0 and hw >= 4096:
        return 2 if k128 else 3
    if Co % 128 == 0:
        return 6
    if Co % 64 == 0:
        return 7 if hw >= 4096 else 8
    return 9


def _generic_cases():
    out, seen = [], {dt: set() for dt in TDT}
    for di, dt in enumerate(TDT):
        shapes = [(SIZES[i % 7], G_CI[i % 4], G_CO[i % 5]) for i in range(di * 9, di * 9 + 26)]
        # every rule at least once per type, at the sizes that reach it
        shapes += [((64, 64), 64, 128), ((64, 64), 96, 128), ((64, 64), 32, 64), ((64, 40), 160, 192), ((33, 17), 96, 256),
                   ((12, 20), 64, 64), ((16, 16), 64, 128), ((5, 7), 32, 256), ((64, 65), 32, 96)]
        for i, ((H, W), Ci, Co) in enumerate(shapes):
            rule = _generic_rule(dt, H, W, Ci, Co)
            seen[dt].add(rule)
            out.append(pytest.param(dt, 2 + (i % 3 == 0), H, W, Ci, Co, rule, i % len(EPIS), i % 3, i % 3,
                                    id=f"{dt}-{H}x{W}-Ci{Ci}-Co{Co}-rule{rule}-e{i % len(EPIS)}r{i % 3}s{i % 3}"))
    return out, seen


GENERIC_CASES, GENERIC_SEEN = _generic_cases()


def test_generic_cases_cover_every_reachable_tile():
    assert GENERIC_SEEN == GENERIC_RULES


@pytest.mark.parametrize("dt,B,H,W,Ci,Co,rule,epi,res,sl", GENERIC_CASES)
def test_generic_kernel_exact(dt, B, H, W, Ci, Co, rule, epi, res, sl):
    p = Problem(B, H, W, Ci, Co, dt, epi, bias=epi != 3, res=res, seed=epi, **SLICES[sl])
    run_exact(p, GENERIC, want_variant=rule)


def test_generic_kernel_refusals():
    p = Problem(2, 8, 32, 64, 32, "bf16")
    assert refusal(p, GENERIC, x_up2=1).startswith("modconv3x3: no x_up2")
    assert refusal(p, GENERIC, Ci_read=32).startswith("modconv3x3: no x_up2")
    p.psum = torch.zeros(2 * 4 * 16, device=DEV)
    assert refusal(p, GENERIC).startswith("modconv3x3: no x_up2")
    p.psum = None
    assert refusal(p, GENERIC, Ci=48).startswith("modconv3x3: Ci must be a multiple of 32")
    assert refusal(p, GENERIC, Co=48).startswith("modconv3x3: Co must be a multiple of 32")
    assert refusal(p, 4).startswith("maua_conv3x3: kernel must be")
    q = Problem(2, 8, 32, 64, 32, "bf16", res=2)
    assert refusal(q, GENERIC, res=None).startswith("maua_conv3x3: res2 goes with res")


# ---------------------------------------------------------------------------------------------------------------- the LDS-direct kernel
# tiles as maua_conv3x3_route reports them: output channels per workgroup (+ 1 odd-chunk form, + 2 piece sums).  bf16 has all seven
# instantiations, f16 the two wide ones without piece sums.
DMA_TILES = {"bf16": {256, 258, 128, 130, 64, 32, 33}, "f16": {256, 128}}
W_CI, W_H, W_W = [64, 128, 192, 320], [8, 16, 24], [32, 64, 96]
W_CO = [(128, 0, 128), (256, 0, 256), (256, 128, 128), (384, 0, 128), (512, 0, 256)]     # (Co, variant argument, tile)


def _wide_cases():
    out, seen = [], {"bf16": set(), "f16": set()}
    for di, dt in enumerate(("bf16", "f16")):
        for i in range(di * 5, di * 5 + 12):
            Co, var, tile = W_CO[i % 5]
            psum = dt == "bf16" and i % 2 == 0
            seen[dt] |= {tile, tile + 2} if psum else {tile}
            out.append(pytest.param(dt, 2, W_H[i % 3], W_W[(i // 2) % 3], W_CI[i % 4], Co, var, tile, i % len(EPIS), (i // 2) % 3, i % 3, psum,
                                    id=f"{dt}-{W_H[i % 3]}x{W_W[(i // 2) % 3]}-Ci{W_CI[i % 4]}-Co{Co}-v{var}-e{i % len(EPIS)}r{(i // 2) % 3}"
                                       f"s{i % 3}p{int(psum)}"))
    return out, seen


WIDE_CASES, WIDE_SEEN = _wide_cases()
N_SIZES = [(8, 32), (9, 33), (34, 50), (40, 70)]       # no overhang, both sides by one, both sides, more than one tile each way
N_SHAPES = [(64, 32, 32), (128, 32, 32), (64, 64, 64), (128, 64, 64), (96, 32, 33), (160, 32, 33), (224, 32, 33)]   # (Ci, Co, tile)


def _narrow_cases():
    out, seen = [], set()
    for i in range(28):
        (H, W), (Ci, Co, tile) = N_SIZES[i % 4], N_SHAPES[i % 7]
        up2 = i % 5 == 1 and H % 2 == 0 and W % 2 == 0
        ci_read = Ci - 40 if i % 3 == 2 and Ci >= 96 else 0
        seen.add(tile)
        out.append(pytest.param(H, W, Ci, Co, tile, i % len(EPIS), (i // 2) % 3, i % 3, up2, ci_read,
                                id=f"{H}x{W}-Ci{Ci}-Co{Co}-e{i % len(EPIS)}r{(i // 2) % 3}s{i % 3}u{int(up2)}k{ci_read}"))
    return out, seen


NARROW_CASES, NARROW_SEEN = _narrow_cases()


def test_dma_cases_cover_every_tile():
    assert WIDE_SEEN["bf16"] | NARROW_SEEN == DMA_TILES["bf16"] and WIDE_SEEN["f16"] == DMA_TILES["f16"]


def _psum_check(p, y):
    """ConvArgs.psum: [sample][8 x 32-pixel tile][Co / 8][16] - 8 sums, then 8 sums of squares, of the STORED values of the piece's channels
    over the tile's pixels.  Against float64 sums of the values read back, within the f32 summation bound n 2^-24 sum |terms|."""
    B, H, W, Co = p.B, p.H, p.W, p.Co
    st = p.got(y).double()                                                        # [B][Co][H][W], what was stored
    t = st.reshape(B, Co // 8, 8, H // 8, 8, W // 32, 32).permute(0, 3, 5, 1, 2, 4, 6).reshape(B, (H // 8) * (W // 32), Co // 8, 8, 256)
    want = torch.cat([t.sum(-1), (t * t).sum(-1)], dim=-1)                       # [B][tile][Co / 8][16]
    bound = 256 * 2.0 ** -24 * torch.cat([t.abs().sum(-1), (t * t).sum(-1)], dim=-1)
    got = p.psum.cpu().double().reshape(want.shape)
    err = (got - want).abs()
    assert (err <= bound).all(), f"piece sums off by up to {(err - bound).max().item()} beyond the f32 summation bound"


@pytest.mark.parametrize("dt,B,H,W,Ci,Co,var,tile,epi,res,sl,psum", WIDE_CASES)
def test_dma_wide_tiles_exact(dt, B, H, W, Ci, Co, var, tile, epi, res, sl, psum):
    p = Problem(B, H, W, Ci, Co, dt, epi, bias=epi != 3, res=res, seed=epi, **SLICES[sl])
    run_exact(p, DMA, want_variant=tile, variant=var)
    if psum:   # the piece-sum instantiation stores the same bits, and sums what it stored
        plain = p.y
        p.y = p.new_y()
        p.psum = torch.full((B * (H // 8) * (W // 32) * (Co // 8) * 16,), float("nan"), device=DEV)
        run_exact(p, DMA, want_variant=tile + 2, variant=var)
        assert torch.equal(_bits(p.y), _bits(plain)), "piece sums on / off store different bits"
        _psum_check(p, p.y)


@pytest.mark.parametrize("res", [0, 1, 2])
def test_dma_piece_sums_on_small_operands(res):
    """operands in [-1, 1] keep the squares small: every entry against the float64 sums of the matching pixels and channels"""
    for Co, var in ((256, 0), (256, 128), (384, 0)):
        p = Problem(2, 16, 64, 128, Co, "bf16", 2, res=res, seed=res, irange=1, brange=4)
        p.psum = torch.full((2 * 2 * 2 * (Co // 8) * 16,), float("nan"), device=DEV)
        run_exact(p, DMA, variant=var)
        _psum_check(p, p.y)


@pytest.mark.parametrize("H,W,Ci,Co,tile,epi,res,sl,up2,ci_read", NARROW_CASES)
def test_dma_narrow_tiles_exact(H, W, Ci, Co, tile, epi, res, sl, up2, ci_read):
    p = Problem(2, H, W, Ci, Co, "bf16", epi, bias=epi != 3, res=res, seed=epi, Ci_read=ci_read, x_up2=up2, **SLICES[sl])
    run_exact(p, DMA, want_variant=tile)


def test_dma_kernel_refusals():
    h = Problem(2, 8, 32, 64, 128, "f16")
    assert refusal(h, DMA, x_up2=1).startswith("modconv_dma (f16): unsupported")
    h.psum = torch.zeros(2 * 16 * 16, device=DEV)
    assert refusal(h, DMA).startswith("modconv_dma (f16): unsupported")
    n = Problem(2, 9, 33, 64, 32, "bf16")
    n.psum = torch.zeros(2 * 4 * 4 * 16, device=DEV)
    assert refusal(n, DMA).startswith("modconv_dma: the narrow tiles carry no")
    n.psum = None
    assert refusal(n, DMA, x_up2=1).startswith("modconv_dma: x_up2 needs even output sizes")
    assert refusal(Problem(2, 8, 32, 96, 64, "bf16"), DMA).startswith("modconv_dma: unsupported shape")    # 64 channels, odd chunk count
    assert refusal(Problem(2, 8, 32, 64, 96, "bf16"), DMA).startswith("modconv_dma: unsupported shape")
    assert refusal(Problem(2, 9, 33, 64, 128, "bf16"), DMA).startswith("modconv_dma: unsupported shape")   # wide tiles do not overhang
    assert refusal(Problem(2, 7, 32, 64, 32, "bf16"), DMA).startswith("modconv_dma: unsupported shape")
    assert refusal(Problem(2, 8, 32, 64, 128, "f32"), DMA).startswith("modconv_dma: unsupported dtype")
    # (the launcher also refuses a noise operand on overhanging tiles; the descriptor of a plain convolution carries none)


# ---------------------------------------------------------------------------------------------------------------- the gather GEMM
# (dt, B, H, W, Ci, Co, K slices).  lowres_geom: 9 Ci / (128 bytes) stages; the smallest divisor >= 256 / (64 x 128 tiles per sample), then
# the fewest slices that still give 2048 workgroups.  1 (2048 tiles), 2 (1536 tiles), every stage its own slice (the largest), and between.
GATHER_CASES = [
    ("bf16", 16, 32, 32, 64, 1024, 1), ("bf16", 16, 32, 24, 128, 1024, 2), ("bf16", 1, 8, 8, 1024, 128, 144), ("f32", 1, 8, 8, 512, 128, 144),
    ("bf16", 5, 5, 7, 64, 128, 9), ("f32", 5, 5, 7, 64, 256, 18), ("bf16", 2, 16, 16, 256, 256, 36), ("f32", 2, 16, 16, 128, 256, 36),
    ("bf16", 1, 32, 32, 64, 128, 9), ("f32", 2, 32, 24, 32, 128, 9), ("bf16", 5, 32, 24, 192, 256, 27), ("f32", 16, 8, 8, 64, 1024, 18),
    ("bf16", 2, 8, 8, 320, 128, 45),
]


@pytest.mark.parametrize("i,dt,B,H,W,Ci,Co,ksplit", [pytest.param(i, *c, id="-".join(map(str, c))) for i, c in enumerate(GATHER_CASES)])
def test_gather_kernel_exact(i, dt, B, H, W, Ci, Co, ksplit):
    p = Problem(B, H, W, Ci, Co, dt, i % len(EPIS), bias=i % 4 != 3, res=i % 2, seed=i, **[dict(), dict(ypad=64, ycoff=32, rpad=32)][i % 2])
    run_exact(p, GATHER, want_variant=0, want_ksplit=ksplit)


def test_gather_cases_take_one_two_and_the_most_slices():
    ks = {c[-1] for c in GATHER_CASES}
    assert {1, 2} <= ks and 9 * 1024 // 64 in ks


def test_gather_kernel_refusals():
    p = Problem(2, 8, 8, 64, 128, "bf16", res=2, xpad=64)
    assert refusal(p, GATHER).startswith("conv_gather: unsupported shape / arguments")            # channel-sliced input
    q = Problem(2, 8, 8, 64, 128, "bf16", res=2)
    assert refusal(q, GATHER).startswith("conv_gather: unsupported shape / arguments")            # a second residual
    q = Problem(2, 8, 8, 64, 128, "bf16")
    assert refusal(q, GATHER, x_bstride=8 * 8 * 64 + 64).startswith("conv_gather: the input must be dense")
    assert refusal(q, GATHER, x_up2=1).startswith("conv_gather: unsupported shape / arguments")
    assert refusal(q, GATHER, Ci_read=32).startswith("conv_gather: unsupported shape / arguments")
    assert refusal(Problem(2, 33, 32, 64, 128, "bf16"), GATHER).startswith("conv_gather: unsupported shape / arguments")   # > 1024 pixels
    assert refusal(Problem(2, 8, 8, 64, 64, "bf16"), GATHER).startswith("conv_gather: unsupported shape / arguments")
    assert refusal(Problem(2, 8, 8, 32, 128, "bf16"), GATHER).startswith("conv_gather: unsupported shape / arguments")
    assert refusal(Problem(2, 8, 8, 64, 128, "f16"), GATHER).startswith("conv_gather: unsupported shape / arguments")


# ---------------------------------------------------------------------------------------------------------------- across kernels
@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("Co", [128, 256])
def test_every_kernel_gives_the_same_bits(res, Co):
    """a shape all three take (16 x 32 pixels, 128 input channels): if two kernels rounded at different points the UNet's output would
    depend on its batch size through the routing"""
    p = Problem(2, 16, 32, 128, Co, "bf16", 0, res=res, seed=res)
    want = p.want()
    outs = {}
    for k in (GENERIC, DMA, GATHER):
        y = p.new_y()
        run(p, k, y=y)
        p.check_guards(y)
        outs[k] = p.got(y)
    for k in (DMA, GATHER):
        assert torch.equal(outs[k], outs[GENERIC]), f"kernel {k} differs from the generic kernel"
    assert torch.equal(outs[GENERIC], want)
    f = Problem(2, 16, 32, 128, Co, "f32", 0, res=res, seed=res)
    y1, y3 = f.new_y(), f.new_y()
    run(f, GENERIC, y=y1)
    run(f, GATHER, y=y3)
    assert torch.equal(f.got(y1), f.got(y3)) and torch.equal(f.got(y1), f.want())


@pytest.mark.parametrize("dt,H,W,Ci,Co", [("bf16", 8, 8, 1024, 1024), ("bf16", 16, 16, 512, 512), ("bf16", 32, 32, 512, 512),
                                          ("f32", 16, 16, 256, 512)])
def test_a_sample_alone_equals_the_sample_in_a_batch_of_16(dt, H, W, Ci, Co):
    """the UNet's routing and the gather kernel's slice count depend on the batch; on the integer family (exact in any slice order) a
    sample's bits must not.  (On Gaussian input the gather kernel is equal across batch sizes to rounding only: 60 dB, stated where
    its slice rule is.)"""
    p = Problem(16, H, W, Ci, Co, dt, 0, res=1)
    r16, r1 = route(p, 0), route(p, 0, B=1)
    assert r16 != r1, "the batch should change the kernel or its K slices here"
    run(p, 0)
    p.check_guards()
    for b0 in (0, 7, 15):
        y = p.new_y()
        run(p, 0, y=y, B=1, b0=b0)
        gpx, n = p.gr * W, H * W
        assert torch.equal(_bits(y)[gpx + b0 * n:gpx + (b0 + 1) * n], _bits(p.y)[gpx + b0 * n:gpx + (b0 + 1) * n]), f"sample {b0}"
        assert (_bits(y)[:gpx + b0 * n].cpu() == SENT[p.tdt]).all() and (_bits(y)[gpx + (b0 + 1) * n:].cpu() == SENT[p.tdt]).all()


def _unet_convs(cfg):
    """(size, Ci, Co), padded to 32 channels, of every 3x3 convolution of a UNet (oracle.diffusion.unet_structure's walk)"""
    from oracle import diffusion as OD
    s, p32, out = OD.unet_structure(cfg), lambda c: (c + 31) // 32 * 32, []
    res = cfg["image_size"]
    out.append((res, p32(cfg["in_channels"]), p32(s["input"][0][0][2])))
    for layers in s["input"][1:] + [s["middle"]] + s["output"]:
        for l in layers:
            if l[0] == "res":
                res = res // 2 if l[3] == "down" else res * 2 if l[3] == "up" else res
                out += [(res, p32(l[1]), p32(l[2])), (res, p32(l[2]), p32(l[2]))]
    out.append((res, p32(s["final_ch"]), p32(cfg["out_channels"])))
    return sorted(set(out))


def _route_shape(B, H, W, Ci, Co, dt="bf16", opt=0):
    d = L.ConvDesc(x=0x10000, w=0x20000, y=0x30000, B=B, H=H, W=W, Ci=Ci, Co=Co, gain=1.0, clamp=-1.0, x_bstride=H * W * Ci)
    v, ks = C.c_int(-1), C.c_int(-1)
    k = L.lib().maua_conv3x3_route(C.byref(d), DTID[dt], opt, C.byref(v), C.byref(ks))
    L.check(min(k, 0))
    return k, v.value


def test_production_routing_runs_the_kernel_the_route_names():
    """kernel 0 on the cheapest shape of every (kernel, tile) class the default 256^2 UNet reaches at batch 1, 4 and 32: the same bits as the
    forced kernel maua_conv3x3_route names (integer operands drawn on the device; these shapes are too large for a host reference)"""
    from oracle import diffusion as OD
    classes = {}
    for B in (1, 4, 32):
        for (s, Ci, Co) in _unet_convs(OD.unet_config()):
            cls = _route_shape(B, s, s, Ci, Co)
            cost = B * s * s * Ci * Co
            if cls not in classes or cost < classes[cls][0]:
                classes[cls] = (cost, B, s, Ci, Co)
    assert set(classes) == {(1, 3), (2, 32), (2, 128), (2, 256), (3, 0)}, sorted(classes)
    g = torch.Generator(device=DEV).manual_seed(5)
    for (kernel, variant), (_, B, s, Ci, Co) in sorted(classes.items()):
        x = torch.randint(-8, 9, (B, s, s, Ci), generator=g, device=DEV).to(torch.bfloat16)
        r = torch.randint(-8, 9, (B, s, s, Co), generator=g, device=DEV).to(torch.bfloat16)
        w = torch.randint(-8, 9, (Co, Ci, 3, 3), generator=g, device=DEV).float()
        b = torch.randint(-64, 65, (Co,), generator=g, device=DEV).float()
        ys = []
        for k in (0, kernel):
            y = torch.empty((B, s, s, Co), dtype=torch.bfloat16, device=DEV)
            _bits(y).fill_(SENT[torch.bfloat16])
            d = L.ConvDesc(x=x.data_ptr(), x_bstride=s * s * Ci, w=w.data_ptr(), bias=b.data_ptr(), y=y.data_ptr(), res=r.data_ptr(),
                           res_pstride=Co, res_bstride=s * s * Co, B=B, H=s, W=s, Ci=Ci, Co=Co, act=0, alpha=1.0, gain=1.0, clamp=-1.0,
                           variant=128 if variant == 128 else 0)
            L.check(L.lib().maua_conv3x3_ex(L.ctx(), C.byref(d), L.BF16, k))
            _sync()
            ys.append(y)
        assert not torch.isnan(ys[0].float()).any()
        assert torch.equal(_bits(ys[0]), _bits(ys[1])), f"kernel 0 differs from forced kernel {kernel} (tile {variant}) at {(B, s, Ci, Co)}"


# ---------------------------------------------------------------------------------------------------------------- Gaussian family
GAUSS = [(GENERIC, "bf16", 2, 33, 17, 160, 128), (GENERIC, "f16", 2, 33, 17, 160, 128), (GENERIC, "f32", 2, 33, 17, 160, 128),
         (DMA, "bf16", 2, 16, 64, 192, 256), (DMA, "f16", 2, 16, 64, 192, 256), (DMA, "bf16", 2, 34, 50, 160, 32),
         (GATHER, "bf16", 5, 32, 24, 192, 256), (GATHER, "f32", 5, 32, 24, 192, 256)]


@pytest.mark.parametrize("res", [0, 1])
@pytest.mark.parametrize("kernel,dt,B,H,W,Ci,Co", GAUSS, ids=[f"k{c[0]}-{c[1]}-{c[3]}x{c[4]}" for c in GAUSS])
def test_kernel_gaussian_within_float64_bound(kernel, dt, B, H, W, Ci, Co, res):
    p = Problem(B, H, W, Ci, Co, dt, 0, res=res, family="gauss", seed=1, ypad=32, rpad=32)
    run(p, kernel)
    p.check_guards()
    err, tol = p.gauss_err_tol()
    print(f"kernel {kernel} {dt} res {res}: max error {err.max().item():.3e}, largest error / bound {(err / tol).max().item():.3f}")
    assert (err <= tol).all(), f"max excess {(err - tol).max().item()}"


@pytest.mark.parametrize("res", [0, 1])
def test_split_f32_gaussian(res):
    """MAUA_F32_SPLIT (float32 tensors, products as three bf16 split products) on Gaussian input: within 4x the error the exact-f32 kernel
    makes against float64 on the same inputs.  Measured on an MI355X (33 x 17 pixels, 160 -> 128 channels, max |error| over the tensor):
    exact-f32 6.108e-06, split 1.922e-05 (ratio 3.15) without a residual; 6.108e-06 and 1.916e-05 (3.14) with one."""
    e = {}
    for dt in ("f32", "split"):
        p = Problem(2, 33, 17, 160, 128, dt, 0, res=res, family="gauss", seed=1, ypad=32, rpad=32)
        run(p, GENERIC)
        p.check_guards()
        err, _ = p.gauss_err_tol()
        e[dt] = err.max().item()
    print(f"res {res}: exact-f32 max error {e['f32']:.3e}, split-f32 max error {e['split']:.3e}, ratio {e['split'] / e['f32']:.2f}")
    assert e["split"] <= 4 * e["f32"], e
