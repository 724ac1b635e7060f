"""The fused GroupNorm kernels (csrc/groupnorm.hip: gn_partial / gn_finalize / gn_apply, gn_partial_group / gn_finalize_group /
gn_finalize_psum / gn_apply_group; csrc/groupnorm_vjp.hip: gn_vjp_partial / gn_vjp_finalize / gn_vjp_apply), launched through
maua_group_norm_ex / maua_group_norm_vjp_ex (csrc/groupnorm_api.hip) - the launchers the diffusion UNet runs - with both sources of
the virtual concatenation, the resampling modes and the raw second output, the scale-shift row stride, the convolution's piece sums,
the kernel route and the gradient's statistics operand chosen here, against float64 references.  The method of
tests/test_gpu_attention.py: a family whose expected result is exact and compared with torch.equal, guard regions around every
buffer (NaN around inputs and in the padding of the scale-shift rows, a sentinel pattern around outputs: y, xr, stats_out, dx0, dx1),
and a Gaussian family inside a derived element-wise bound.  The CPU side is tests/groupnorm_ref.py; tests/test_groupnorm_host.py
proves what the exact family rests on.  maua_group_norm_plan / _vjp_plan say which route, chunking and statistics source a case took.

Exact family.  Group (b, g) holds m + d k: m, d powers of two (|m| / d up to 128), k integers in +- pairs - every float64 partial sum
is exact in any order, the mean is m, and rstd = (float)(1 / sqrt(var + (double)1e-5f)) is the same float32 whether the variance's
`q / cnt - mean * mean` is rounded twice or contracted (proven per input; every fifth group is constant: variance exactly 0).
stats_out is compared exactly on both routes, from the piece sums (float32 tile sums of these inputs are exact) and in the mixed
case.  With silu = 0, gamma = +-2^j and 1 + scale a power of two, ca = rstd gamma and mean ca are exact, and fma(x, ca, cb),
fma(u, 1 + scale, shift) have float64-exact arguments: numpy reproduces y bit for bit, the 2x2 average in the kernels' tap order.
xr is an exact float32 sum of four values, rounded once at the store.
Exact gradient: constant groups (xh = fma(m, rstd, -m rstd) = 0, so the second mean is exactly 0) and integer dy / dres / add whose
group mean is a dyadic number: dx = rstd (dxh - m1) + R^T dres + add, one float32 rounding each, then the store's.

Gaussian family.  Operands rounded to the storage type, float64 reference on the rounded operands: unit Gaussians; spread 1 around a
group mean of up to 60; spread 0.5 around per-channel means of 30 N(0, 1); gamma / beta / scale-shift that spread the pre-activations
over [-20, 20] and beyond.  Bounds, element-wise (v = 2^-24, u = the storage unit, r = the relative error of rstd, xh = (x - mean) rstd):
    statistics  float64 sums: 2^-40 relative.  bf16 group route: 8 values meet in float32 first, ds <= 7 v sum|x|, dq <= 8 v sum x^2;
                piece sums: 256-term float32 tile sums, ds <= 256 v sum|x|, dq <= 256 v sum x^2.  dmean = ds / cnt + v |mean|,
                dvar = dq / cnt + 2 |mean| ds / cnt - the float32 error times 1 + (mean / std)^2 once divided by var -,
                t = dvar / (var + eps), r = t / (2 (1 - t)) + v
    forward     E1 = |xh gamma| (r + 2 v) + dmean rstd |gamma| + 2 v |mean| rstd |gamma| + v (|beta| + |u|)
                     (the third term is the cancellation of x ca against cb = beta - mean ca, both of size |mean| rstd |gamma|)
                E2 = E1 |1 + s| + v |u (1 + s)| + v |u2|;   E3 = 1.1 E2 + |a| (eps_exp e / (1 + e) + 4 v), e = exp(-u2)
                2x2 average: mean(E3) + 3 v mean|a|;  y: E + u (|y| + E);  xr: 3 v mean|x| + u |xr|
    gradient    Exh = v (|mean| rstd + |xh|) (the same cancellation: xh = fma(x, rstd, -mean rstd));  Epre = Exh |gs| + 2 v |xh gs| +
                2 v |bs| + v |pre|;  dsg = sg ((1 - sg) eps_exp + 4 v);  ED = 0.5 Epre + (1 + |pre|) dsg + 4 v (|D| + sg |pre| (1 - sg));
                Edxh = |da gs| ED + |D gs| Eda + 5 v |dxh|;  Em1 = mean(Edxh) + run v mean|dxh| + v |m1|;  Em2 = mean(Edxh |xh| + |dxh|
                Exh) + (run + 1) v mean|dxh xh| + v |m2|;  E = rstd (Edxh + Em1 + Exh |m2| + |xh| Em2 + 3 v (|dxh| + |m1| + |xh m2|)) +
                v |out| + 3 v R^T|dres| (mode 2) + 2 v (|out| + R^T|dres| + |add|);  dx: E + u (|dx| + E)
                (run = ceil(ppc / RY), a thread's float32 run of the partial sums, from the plan query)
eps_exp is the one term not derived from the code: in bf16 SiLU and its derivative use the hardware exp and reciprocal.  float32 exp
on the CPU is measured against float64 over the case's own arguments and 4 x that is allowed (the project's convention); in f32 the
kernels call expf (<= 1 ulp) and divide exactly rounded: eps_exp = 2^-22.  No other margin.  Every group-kernel case is run again with
force_route = 1 and the two results must agree inside the sum of their bounds."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import groupnorm_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
TDT = R.TDT
DTID = {"f32": L.F32, "bf16": L.BF16}
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
G = 4096                                            # guard elements on either side of every buffer
WORST = {}                                          # family -> worst error / bound seen (test_zz_report prints it)
EXP_DEV = {}                                        # family -> largest measured float32 exp deviation
TAKEN = set()                                       # (what, value) the plan queries reported


def _sync():
    torch.cuda.synchronize()


class Buf:
    """rows of `width` elements `ld` apart, starting `lead` elements into their row, between guard regions.  Inputs (data given):
    NaN in the guards and in the rows' padding.  Outputs: a sentinel bit pattern everywhere; check() wants the guards intact and
    every element of the body written."""

    def __init__(self, rows, width, ld=None, dtype=torch.float32, data=None, lead=0):
        ld = width if ld is None else ld
        self.rows, self.width, self.ld, self.lead = rows, width, ld, lead
        self.full = torch.empty((2 * G + rows * ld,), dtype=dtype, device=DEV)
        if data is None:
            self._bits().fill_(SENT16 if self.full.element_size() == 2 else SENT32)
        else:
            body = torch.full((rows, ld), float("nan"), dtype=dtype)
            body[:, lead:lead + width] = torch.as_tensor(data).reshape(rows, width).to(dtype)
            self.full.fill_(float("nan"))
            self.full[G:G + rows * ld] = body.reshape(-1).to(DEV)
        self.ptr = self.full.data_ptr() + (G + lead) * self.full.element_size()

    def _bits(self):
        return self.full.view(torch.int16 if self.full.element_size() == 2 else torch.int32)

    def get(self):
        return self.full[G:G + self.rows * self.ld].reshape(self.rows, self.ld)[:, self.lead:self.lead + self.width].cpu()

    def check(self, what):
        s = SENT16 if self.full.element_size() == 2 else SENT32
        b = self._bits()
        assert bool((b[:G] == s).all()) and bool((b[G + self.rows * self.ld:] == s).all()), f"{what}: a store outside the buffer"
        assert bool((b[G:G + self.rows * self.ld] != s).all()), f"{what}: elements of the result were never written"
        assert not bool(torch.isnan(self.full[G:G + self.rows * self.ld].float()).any()), f"{what}: NaN in the result (a guard was read)"


def dense(a, dt):
    """a float64 array -> an input buffer of the storage type (the values must be representable)"""
    t = torch.from_numpy(np.ascontiguousarray(a))
    st = t.to(TDT[dt])
    assert torch.equal(st.double(), t), "operands must be representable in the storage type"
    return Buf(1, t.numel(), dtype=TDT[dt], data=st)


def ss_buf(ss, kind, B, Cc):
    """(buffer or None, ss_ld, shared)"""
    if kind == "none" or ss is None:
        return None, 0, False
    if kind == "shared":
        return Buf(1, 2 * Cc, data=torch.from_numpy(ss[:1].copy())), 0, True
    if kind == "wide":
        return Buf(B, 2 * Cc, ld=2 * Cc + 64, data=torch.from_numpy(ss), lead=32), 2 * Cc + 64, False
    return Buf(B, 2 * Cc, data=torch.from_numpy(ss)), 2 * Cc, False


def note(family, ratio):
    WORST[family] = max(WORST.get(family, 0.0), float(ratio))


def ratio(got, ref, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    assert np.isfinite(err).all()
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0


class Forward:
    """one GroupNorm forward on uploaded inputs; run(force) launches it and returns (y, xr, stats, plan) with every guard checked"""

    def __init__(self, x, C0, dt, gamma, beta, ss, ss_kind, silu, mode, want_xr, ps=(None, None)):
        self.B, self.H, self.W, self.C = x.shape
        self.C0, self.C1, self.dt, self.silu, self.mode, self.want_xr = C0, self.C - C0, dt, silu, mode, want_xr
        self.x0 = dense(x[..., :C0], dt)
        self.x1 = dense(x[..., C0:], dt) if self.C1 else None
        self.gamma, self.beta = Buf(1, self.C, data=torch.from_numpy(gamma)), Buf(1, self.C, data=torch.from_numpy(beta))
        self.ss, self.ss_ld, self.shared = ss_buf(ss, ss_kind, self.B, self.C)
        self.ps = [None if p is None else Buf(1, p.size, data=torch.from_numpy(p)) for p in ps]
        self.rows = [0 if p is None else p.shape[1] for p in ps]
        self.Ho, self.Wo = R.out_size(self.H, self.W, mode)

    def run(self, force=0):
        n = self.B * self.Ho * self.Wo * self.C
        y = Buf(1, n, dtype=TDT[self.dt])
        xr = Buf(1, n, dtype=TDT[self.dt]) if self.want_xr else None
        st = Buf(1, self.B * 64)
        d = L.GnDesc(x0=self.x0.ptr, C0=self.C0, x1=self.x1.ptr if self.x1 else None, C1=self.C1, B=self.B, H=self.H, W=self.W,
                     gamma=self.gamma.ptr, beta=self.beta.ptr, ss=self.ss.ptr if self.ss else None, ss_ld=self.ss_ld, silu=self.silu,
                     mode=self.mode, y=y.ptr, xr=xr.ptr if xr else None, ps0=self.ps[0].ptr if self.ps[0] else None, rows0=self.rows[0],
                     ps1=self.ps[1].ptr if self.ps[1] else None, rows1=self.rows[1], stats_out=st.ptr, force_route=force,
                     dtype=DTID[self.dt])
        o = [C.c_int(-1) for _ in range(5)]
        L.check(L.lib().maua_group_norm_plan(C.byref(d), *[C.byref(t) for t in o]))
        plan = tuple(t.value for t in o)
        L.check(L.lib().maua_group_norm_ex(L.ctx(), C.byref(d)))
        _sync()
        y.check("y")
        st.check("stats_out")
        if xr:
            xr.check("xr")
        shp = (self.B, self.Ho, self.Wo, self.C)
        stats = st.get().reshape(self.B, 32, 2).numpy()
        TAKEN.update({("route", plan[0], self.dt), ("source", plan[4]), ("fwd RY", plan[1]), ("fwd threads", plan[1] * self.C // R.EPC[self.dt])})
        if plan[3] == 128:
            TAKEN.add(("fwd chunks", 128, (self.H * self.W) % plan[2] != 0))
        return y.get().reshape(shp), xr.get().reshape(shp) if xr else None, stats[..., 0], stats[..., 1], plan


def make_ss(B, Cc, seed, kind, exact, per_group=False):
    with_ss = kind != "none"
    if exact:
        return R.exact_params(B, Cc, seed, with_ss, per_group)
    return R.gaussian_params(B, Cc, seed, with_ss)


# ---------------------------------------------------------------------------------------------------------------- exact forward
def check_exact_forward(fw, x, m32, r32, gamma, beta, ss, expect_route=None, expect_source=None):
    want, ok = R.emulate_apply(x, m32, r32, gamma, beta, ss, fw.shared, fw.mode)
    assert ok, "an fma of the emulation whose float64 argument is not exact"
    want = R.to_storage(want, fw.dt)
    want_xr = R.to_storage(R.resample_raw(x, fw.mode), fw.dt) if fw.want_xr else None
    plans = []
    for force in (0, 1):
        y, xr, mean, rstd, plan = fw.run(force)
        plans.append(plan)
        assert plan[0] == 1 or force == 0
        assert np.array_equal(mean, m32), f"mean differs (plan {plan})"
        assert np.array_equal(rstd, r32), f"rstd differs (plan {plan})"
        assert torch.equal(y, want), f"y differs from the emulation (plan {plan})"
        if fw.want_xr:
            assert torch.equal(xr, want_xr), f"xr differs (plan {plan})"
        if plan[0] == 1:
            break
    if expect_route is not None:
        assert plans[0][0] == expect_route, plans[0]
    if expect_source is not None:
        assert plans[0][4] == expect_source, plans[0]
    return plans[0]


@pytest.mark.parametrize("i", range(len(R.EXACT_CASES)))
def test_exact_forward(i):
    B, H, W, C0, C1, dt, mode, ss_kind, want_xr = R.EXACT_CASES[i]
    Cc = C0 + C1
    x = R.exact_input(B, H, W, Cc, seed=i)
    m32, r32, _ = R.exact_stats(x)
    gamma, beta, ss = make_ss(B, Cc, i, ss_kind, True)
    fw = Forward(x, C0, dt, gamma, beta, ss, ss_kind, 0, mode, want_xr)
    cpg = Cc // 32
    fast = cpg % R.EPC[dt] == 0 and B * fw.Ho <= 65535
    plan = check_exact_forward(fw, x, m32, r32, gamma, beta, ss, expect_route=0 if fast else 1, expect_source=0)
    # the edges this case is here for, as the launcher reports them
    edge = {9: (0, 5), 10: (0, 2), 12: (0, 1), 13: (0, 1, 4, 1, 0), 14: (0, 1, 4, 1, 0), 19: (0, 2, 9, 10, 0), 20: (0, 16, 65, 128, 0),
            25: (1, 16, 171, 128, 0), 26: (1, 16, 256, 128, 0), 0: (1, 64, 1, 1, 0)}.get(i)
    if edge:
        assert plan[:len(edge)] == edge, plan


@pytest.mark.parametrize("i", range(len(R.PSUM_CASES)))
def test_exact_piece_sums(i):
    """statistics from the convolution's piece sums: computed on the CPU from the stored values in the convolution's layout"""
    B, H, W, C0, C1, has0, has1 = R.PSUM_CASES[i]
    Cc = C0 + C1
    x = R.exact_input(B, H, W, Cc, seed=H + C0)
    m32, r32, _ = R.exact_stats(x)
    gamma, beta, ss = make_ss(B, Cc, i, "2C", True)
    ps = (R.psum_layout(x[..., :C0]) if has0 else None, R.psum_layout(x[..., C0:]) if has1 and C1 else None)
    assert all(p is None or p.shape[1] == (H // 8) * (W // 32) for p in ps)
    fw = Forward(x, C0, "bf16", gamma, beta, ss, "2C", 0, (0, 0, 2)[i % 3], 0, ps)
    fast = (Cc // 32) % 8 == 0
    every = has0 and (has1 or not C1)
    check_exact_forward(fw, x, m32, r32, gamma, beta, ss, expect_route=0 if fast else 1, expect_source=1 if fast and every else 0)
    if fast and every:
        # the sums are what is read: with one tile's sums doubled the mean must move (and the tensor itself is not consulted)
        bad = ps[0].copy()
        bad[:, 0, :, :8] += 64.0
        fw2 = Forward(x, C0, "bf16", gamma, beta, ss, "2C", 0, 0, 0, (bad, ps[1]))
        _, _, mean, _, plan = fw2.run(0)
        assert plan[4] == 1 and not np.array_equal(mean[:, 0], m32[:, 0])


# ---------------------------------------------------------------------------------------------------------------- Gaussian forward
def check_gauss_forward(i, case, ps_from=None):
    B, H, W, C0, C1, dt, mode, ss_kind, silu, regime = case
    Cc = C0 + C1
    x = R.gaussian_input(B, H, W, Cc, regime, seed=100 + i, dt=dt)
    gamma, beta, ss = make_ss(B, Cc, 100 + i, ss_kind, False)
    ps = (None, None)
    if ps_from:
        ps = (R.psum_layout(x[..., :C0]), R.psum_layout(x[..., C0:]) if C1 else None)
    fw = Forward(x, C0, dt, gamma, beta, ss, ss_kind, silu, mode, 1, ps)
    eps = None if dt == "bf16" else 2.0 ** -22
    got, refs, plans = [], [], []
    for force in (0, 1):
        y, xr, mean, rstd, plan = fw.run(force)
        plans.append(plan)
        group_sums = plan[0] == 0 and dt == "bf16" and plan[4] == 0
        ref = R.forward_reference(x, gamma, beta, ss, fw.shared, silu, mode, dt, group_sums, psum_err=256.0 if plan[4] == 1 else 0.0, exp_eps=eps)
        fam = f"forward {dt}" + (" piece sums" if plan[4] == 1 else "") + (" per-channel" if plan[0] == 1 else " group")
        note(fam, ratio(y.double().numpy(), ref["y"], ref["by"]))
        note(f"xr {dt}", ratio(xr.double().numpy(), ref["xr"], ref["bxr"]))
        note(f"mean{' piece sums' if plan[4] == 1 else ''}", ratio(mean, ref["mean"], ref["bmean"]))
        note(f"rstd{' piece sums' if plan[4] == 1 else ''}", ratio(rstd, ref["rstd"], ref["brstd"]))
        if silu and dt == "bf16":
            EXP_DEV["forward"] = max(EXP_DEV.get("forward", 0.0), ref["dev"])
        assert ratio(mean, ref["mean"], ref["bmean"]) <= 1 and ratio(rstd, ref["rstd"], ref["brstd"]) <= 1, plan
        assert ratio(y.double().numpy(), ref["y"], ref["by"]) <= 1, (plan, fam)
        assert ratio(xr.double().numpy(), ref["xr"], ref["bxr"]) <= 1, plan
        got.append(y.double().numpy())
        refs.append(ref)
        if plan[0] == 1:
            break
    if len(got) == 2:       # the two routes against each other, inside the sum of their bounds
        r2 = ratio(got[0], got[1], refs[0]["by"] + refs[1]["by"])
        note("route 0 against route 1", r2)
        assert r2 <= 1
    return plans[0]


@pytest.mark.parametrize("i", range(len(R.GAUSS_CASES)))
def test_gaussian_forward(i):
    check_gauss_forward(i, R.GAUSS_CASES[i])


@pytest.mark.parametrize("i,case", enumerate([(2, 8, 32, 256, 0, "bf16", 0, "2C", 1, 1), (2, 16, 64, 256, 512, "bf16", 0, "none", 1, 1),
                                              (1, 16, 64, 256, 0, "bf16", 1, "2C", 1, 2)]))
def test_gaussian_forward_piece_sums(i, case):
    """the piece-sum source with float32 tile sums: the bound carries their error times (mean / std)^2"""
    plan = check_gauss_forward(50 + i, case, ps_from=True)
    assert plan[0] == 0 and plan[4] == 1


def test_preactivations_reach_the_tails():
    B, H, W, C0, C1, dt, mode, ss_kind, silu, regime = R.GAUSS_CASES[4]
    x = R.gaussian_input(B, H, W, C0 + C1, regime, seed=104, dt=dt)
    gamma, beta, ss = make_ss(B, C0 + C1, 104, ss_kind, False)
    ref = R.forward_reference(x, gamma, beta, ss, False, 0, 0, dt, True)
    assert ref["y"].min() < -20 and ref["y"].max() > 20
    assert (np.abs(ref["mean"]) * ref["rstd"]).max() > 30


# ---------------------------------------------------------------------------------------------------------------- gradient
class Gradient:
    def __init__(self, x, C0, dt, stats, gamma, beta, ss, ss_kind, silu, mode, dy, dres, add):
        self.B, self.H, self.W, self.C = x.shape
        self.C0, self.C1, self.dt, self.silu, self.mode = C0, self.C - C0, dt, silu, mode
        self.x0 = dense(x[..., :C0], dt)
        self.x1 = dense(x[..., C0:], dt) if self.C1 else None
        self.stats = Buf(1, self.B * 64, data=torch.from_numpy(np.stack(stats, -1).astype(np.float32)))
        self.gamma, self.beta = Buf(1, self.C, data=torch.from_numpy(gamma)), Buf(1, self.C, data=torch.from_numpy(beta))
        self.ss, self.ss_ld, self.shared = ss_buf(ss, ss_kind, self.B, self.C)
        self.dy = dense(dy, dt)
        self.dres = dense(dres, dt) if dres is not None else None
        self.add0 = dense(add[0], dt) if add[0] is not None else None
        self.add1 = dense(add[1], dt) if add[1] is not None else None

    def run(self):
        px = self.B * self.H * self.W
        dx0 = Buf(1, px * self.C0, dtype=TDT[self.dt])
        dx1 = Buf(1, px * self.C1, dtype=TDT[self.dt]) if self.C1 else None
        p = lambda b: b.ptr if b else None   # noqa: E731
        d = L.GnVjpDesc(x0=self.x0.ptr, C0=self.C0, x1=p(self.x1), C1=self.C1, stats=self.stats.ptr, gamma=self.gamma.ptr,
                        beta=self.beta.ptr, ss=p(self.ss), ss_ld=self.ss_ld, silu=self.silu, mode=self.mode, dy=self.dy.ptr,
                        dres=p(self.dres), add0=p(self.add0), add1=p(self.add1), dx0=dx0.ptr, dx1=p(dx1), B=self.B, H=self.H, W=self.W,
                        dtype=DTID[self.dt])
        o = [C.c_int(-1) for _ in range(4)]
        L.check(L.lib().maua_group_norm_vjp_plan(C.byref(d), *[C.byref(t) for t in o]))
        plan = tuple(t.value for t in o)
        L.check(L.lib().maua_group_norm_vjp_ex(L.ctx(), C.byref(d)))
        _sync()
        dx0.check("dx0")
        out = dx0.get().reshape(self.B, self.H, self.W, self.C0)
        if dx1:
            dx1.check("dx1")
            out = torch.cat((out, dx1.get().reshape(self.B, self.H, self.W, self.C1)), 3)
        TAKEN.update({("vjp RY", plan[0]), ("vjp threads", plan[0] * self.C // R.EPC[self.dt]), ("vjp ranges", plan[3])})
        return out, plan


def split_add(add, C0, C1, a0, a1):
    return (add[..., :C0] if a0 else None, add[..., C0:] if a1 and C1 else None)


def joined_add(add, C0, C1, a0, a1):
    """the `add` the reference sees: zero where a source has none"""
    if not (a0 or (a1 and C1)):
        return None
    t = add.copy()
    if not a0:
        t[..., :C0] = 0
    if not (a1 and C1):
        t[..., C0:] = 0
    return t


@pytest.mark.parametrize("i", range(len(R.GRAD_CASES)))
def test_exact_gradient(i):
    B, H, W, C0, C1, dt, mode, ss_kind, has_dres, a0, a1 = R.GRAD_CASES[i]
    Cc, seed = C0 + C1, 200 + i
    x = R.exact_grad_input(B, H, W, Cc, seed)
    m32, r32, var = R.exact_stats(x)
    assert (var == 0).all()
    Ho, Wo = R.out_size(H, W, mode)
    dy, _ = R.exact_grad_dy(B, Ho, Wo, Cc, seed)
    dres = R.exact_grad_dy(B, Ho, Wo, Cc, seed + 1)[0] if has_dres else None
    add = R.exact_grad_dy(B, H, W, Cc, seed + 2)[0]
    gamma, beta, ss = make_ss(B, Cc, seed, ss_kind, True, per_group=True)
    gr = Gradient(x, C0, dt, (m32, r32), gamma, beta, ss, ss_kind, 0, mode, dy, dres, split_add(add, C0, C1, a0, a1))
    got, plan = gr.run()
    want, m1, exact = R.emulate_grad_const(dy, r32, gamma, ss, gr.shared, mode, H, W, dres, joined_add(add, C0, C1, a0, a1),
                                           run=-(-plan[1] // plan[0]))
    assert exact, "a group mean of dxh that is not exact"
    assert torch.equal(got, R.to_storage(want, dt)), f"dx differs from the emulation (plan {plan})"
    edge = {4: (1, 4, 1, 1), 5: (1, 4, 1, 1), 12: (8, 65, 128, 1), 13: (8, 171, 128, 2), 3: (32, 1, 1, 1), 11: (1,)}.get(i)
    if edge:
        assert plan[:len(edge)] == edge, plan


# every case but the huge one with SiLU, every third without
@pytest.mark.parametrize("i,silu", [(i, 1) for i in range(len(R.GRAD_CASES) - 1)] + [(i, 0) for i in range(0, len(R.GRAD_CASES) - 1, 3)])
def test_gaussian_gradient(i, silu):
    B, H, W, C0, C1, dt, mode, ss_kind, has_dres, a0, a1 = R.GRAD_CASES[i]
    Cc, seed = C0 + C1, 300 + i
    rng = np.random.default_rng(seed)
    x = R.gaussian_input(B, H, W, Cc, (1, 0, 2)[i % 3], seed, dt=dt)
    ref = R.forward_reference(x, np.ones(Cc, np.float32), np.zeros(Cc, np.float32), None, False, 0, 0, dt, False)
    m32, r32 = ref["mean"].astype(np.float32), ref["rstd"].astype(np.float32)
    Ho, Wo = R.out_size(H, W, mode)
    rnd = lambda *s: R.to_storage(rng.normal(size=s), dt).double().numpy()   # noqa: E731
    dy, add = rnd(B, Ho, Wo, Cc), rnd(B, H, W, Cc)
    dres = rnd(B, Ho, Wo, Cc) if has_dres else None
    gamma, beta, ss = make_ss(B, Cc, seed, ss_kind, False)
    gr = Gradient(x, C0, dt, (m32, r32), gamma, beta, ss, ss_kind, silu, mode, dy, dres, split_add(add, C0, C1, a0, a1))
    got, plan = gr.run()
    run = -(-plan[1] // plan[0])
    want, bound, dev = R.grad_reference(x, m32, r32, gamma, beta, ss, gr.shared, silu, mode, dy, dres, joined_add(add, C0, C1, a0, a1), dt, run,
                                        exp_eps=None if dt == "bf16" else 2.0 ** -22)
    if silu and dt == "bf16":
        EXP_DEV["gradient"] = max(EXP_DEV.get("gradient", 0.0), dev)
    r_ = ratio(got.double().numpy(), want, bound)
    note(f"gradient {dt}", r_)
    assert r_ <= 1, plan


def test_refusals_launch_nothing():
    """what the checks refuse (tests/test_groupnorm_host.py pins every text) is refused by the launching entry points too, and B == 0
    returns at once: the sentinel-filled results stay untouched"""
    x = R.exact_input(1, 2, 4, 256, seed=1)
    gamma, beta, _ = R.exact_params(1, 256, 1, False)
    fw = Forward(x, 128, "bf16", gamma, beta, None, "none", 0, 0, 1)
    y, xr, st = Buf(1, x.size, dtype=torch.bfloat16), Buf(1, x.size, dtype=torch.bfloat16), Buf(1, 64)
    ps = Buf(1, 4096, data=torch.zeros(4096))
    base = dict(x0=fw.x0.ptr, C0=128, x1=fw.x1.ptr, C1=128, B=1, H=2, W=4, gamma=fw.gamma.ptr, beta=fw.beta.ptr, ss=None, ss_ld=0, silu=0,
                mode=0, y=y.ptr, xr=xr.ptr, ps0=None, rows0=0, ps1=None, rows1=0, stats_out=st.ptr, force_route=0, dtype=L.BF16)
    for kw, text in ((dict(mode=3), "group_norm: bad resample mode"), (dict(mode=1, H=1, W=8), "group_norm: bad resample mode"),
                     (dict(x1=None), "group_norm: x1 is NULL with C1 > 0"),
                     (dict(ps0=ps.ptr, rows0=1), "group_norm: piece sums need H % 8 == 0, W % 32 == 0, C % 128 == 0 of their source and rows == "
                                                 "(H / 8) * (W / 32)"),
                     (dict(ps0=ps.ptr, rows0=1, dtype=L.F32), "group_norm: piece sums are bf16 only"),
                     (dict(C0=100, C1=156), "group_norm: C % 32 == 0, at most 1024 16-byte pieces per pixel"),
                     (dict(y=y.ptr + 2), "group_norm: pointers and ss_ld must be whole 16-byte pieces"),
                     (dict(force_route=2), "group_norm: force_route is 0 (as routed) or 1 (per-channel kernels)"),
                     (dict(dtype=L.F16), "group_norm: unsupported dtype")):
        assert L.lib().maua_group_norm_ex(L.ctx(), C.byref(L.GnDesc(**{**base, **kw}))) == -1
        assert L.lib().maua_last_error().decode() == text
    assert L.lib().maua_group_norm_ex(L.ctx(), C.byref(L.GnDesc(**{**base, "B": 0}))) == 0
    _sync()
    for b in (y, xr, st):
        assert bool((b._bits() == (SENT16 if b.full.element_size() == 2 else SENT32)).all())
    dx0, dx1 = Buf(1, 1024, dtype=torch.bfloat16), Buf(1, 1024, dtype=torch.bfloat16)
    stats = Buf(1, 64, data=torch.ones(64))
    vb = dict(x0=fw.x0.ptr, C0=128, x1=fw.x1.ptr, C1=128, stats=stats.ptr, gamma=fw.gamma.ptr, beta=fw.beta.ptr, ss=None, ss_ld=0, silu=0,
              mode=0, dy=fw.x0.ptr, dres=None, add0=None, add1=None, dx0=dx0.ptr, dx1=dx1.ptr, B=1, H=2, W=4, dtype=L.BF16)
    for kw, text in ((dict(mode=1, H=1, W=8), "group_norm_vjp: bad resample mode"), (dict(stats=None), "group_norm_vjp: NULL argument"),
                     (dict(dx1=None), "group_norm_vjp: C % 32 == 0, at most 1024 16-byte pieces per pixel"),
                     (dict(dx0=dx0.ptr + 2), "group_norm_vjp: pointers and ss_ld must be whole 16-byte pieces"),
                     (dict(H=65536), "group_norm_vjp: grid too large")):
        assert L.lib().maua_group_norm_vjp_ex(L.ctx(), C.byref(L.GnVjpDesc(**{**vb, **kw}))) == -1
        assert L.lib().maua_last_error().decode() == text
    assert L.lib().maua_group_norm_vjp_ex(L.ctx(), C.byref(L.GnVjpDesc(**{**vb, "B": 0}))) == 0
    _sync()
    for b in (dx0, dx1):
        assert bool((b._bits() == SENT16).all())


def test_zz_report():
    """the worst error / bound per family, the measured exp deviation, and that every route, source and chunk edge was taken"""
    for k in sorted(WORST):
        print(f"[groupnorm] worst error / bound, {k}: {WORST[k]:.3f}")
    for k in sorted(EXP_DEV):
        print(f"[groupnorm] float32 exp against float64 over the {k} cases' arguments: {EXP_DEV[k]:.3e} relative (4 x allowed)")
    assert all(v <= 1 for v in WORST.values())
    if len(WORST) < 8:      # (a single test was selected: the coverage below is a statement about the whole file)
        return
    for t in (("route", 0, "f32"), ("route", 0, "bf16"), ("route", 1, "f32"), ("route", 1, "bf16"), ("source", 0), ("source", 1),
              ("fwd RY", 1), ("fwd RY", 5), ("fwd threads", 480), ("fwd threads", 384), ("fwd threads", 1024), ("fwd chunks", 128, True),
              ("vjp RY", 1), ("vjp threads", 1024), ("vjp threads", 192), ("vjp ranges", 2)):
        assert t in TAKEN, f"{t} was never taken"
