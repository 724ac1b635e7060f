"""CPU side of the GroupNorm parity tests (tests/test_groupnorm_host.py proves it, tests/test_gpu_groupnorm.py uses it): the input
generators of the exact family, the float64 references, the float32 emulation of the kernels' steps, the convolution's piece-sum
layout, and the element-wise bounds of the Gaussian family.  numpy / torch on the CPU only; nothing here touches the library.

Notation: v = 2^-24 (a float32 rounding), u = the storage type's (2^-8 bf16, 2^-24 f32), cnt = H W C / 32 values per group."""
import math
from fractions import Fraction

import numpy as np
import torch

V = 2.0 ** -24
U = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
EPC = {"bf16": 8, "f32": 4}
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
EPS = float(np.float32(1e-5))                       # the kernels' (double)1e-5f
F32, F64 = np.float32, np.float64


def out_size(H, W, mode):
    return (H // 2, W // 2) if mode == 1 else ((H * 2, W * 2) if mode == 2 else (H, W))


def to_storage(a, dt):
    """float array -> torch tensor of the storage type, round to nearest even (what the kernels' stores do)"""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=F32)).to(TDT[dt])


def representable(a, dt):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=F64))
    return bool(torch.equal(t.to(TDT[dt]).double(), t))


# ------------------------------------------------------------------------------------------------------------ exact rounding
def round_f32(fr):
    """a Fraction rounded to the nearest float32 (ties to even), as a Fraction - no double rounding"""
    if fr == 0:
        return Fraction(0)
    e = math.floor(math.log2(abs(fr))) - 23
    while abs(fr) >= Fraction(2) ** (e + 24):
        e += 1
    while abs(fr) < Fraction(2) ** (e + 23):
        e -= 1
    assert e >= -149 + 23 - 23 and e + 23 <= 127, "outside float32's normal range"
    return Fraction(round(fr / Fraction(2) ** e)) * Fraction(2) ** e      # round(Fraction) is half-to-even


def fma32(a, b, c):
    """float32 fma(a, b, c) through float64: a * b is exact there (48 bits); the sum must be exact too (TwoSum), so the one rounding
    to float32 is the fma's.  Returns (result, the sum was exact everywhere)."""
    p = a.astype(F64) * b.astype(F64)
    c = np.broadcast_to(c.astype(F64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    return s.astype(F32), not bool(err.any())


# ------------------------------------------------------------------------------------------------------------ statistics
def group_sums(x):
    """x float64 [B][H][W][C] -> per (sample, group) sum and sum of squares in float64, and cnt"""
    B, H, W, C = x.shape
    g = x.reshape(B, H * W, 32, C // 32)
    return g.sum((1, 3)), (g * g).sum((1, 3)), H * W * (C // 32)


def stats_from_sums(s, q, cnt, contracted=False):
    """the finalize kernels' last thread: mean = s / cnt, var = q / cnt - mean * mean clamped at 0, rstd = 1 / sqrt(var + eps), both
    stored as float32.  contracted: the subtraction as ONE fma(-mean, mean, q / cnt), evaluated exactly and rounded once."""
    mean = s / F64(cnt)
    qq = q / F64(cnt)
    if contracted:
        var = np.array([float(Fraction(float(a)) - Fraction(float(m)) ** 2) for a, m in zip(qq.ravel(), mean.ravel())]).reshape(mean.shape)
    else:
        var = qq - mean * mean
    var = np.maximum(var, 0.0)
    return mean.astype(F32), (1.0 / np.sqrt(var + F64(EPS))).astype(F32), mean, var


def exact_stats(x):
    """float32 (mean, rstd) and the float64 variance of an exact-family input, with the proofs the family rests on: the float64 sums
    are exact (recomputed in integers), the mean is exact, and rstd is the same float32 whether `q / cnt - mean * mean` is rounded
    twice or contracted into one fma"""
    s, q, cnt = group_sums(x)
    xi = np.round(x * 4).astype(np.int64)
    assert (xi == x * 4).all()
    B, H, W, C = x.shape
    gi = xi.reshape(B, H * W, 32, C // 32)
    assert (gi.sum((1, 3)) == s * 4).all() and ((gi * gi).sum((1, 3)) == q * 16).all() and float(q.max()) * 16 < 2.0 ** 53
    m32, r32, mean, var = stats_from_sums(s, q, cnt)
    m32c, r32c, _, _ = stats_from_sums(s, q, cnt, contracted=True)
    assert (mean * cnt == s).all() and (m32.astype(F64) == mean).all(), "the mean is not exact"
    assert np.array_equal(r32, r32c) and np.array_equal(m32, m32c), "rstd depends on contracting q / cnt - mean * mean"
    return m32, r32, var


def psum_layout(x, dtype=F32):
    """the piece sums a wide-tile LDS-direct convolution leaves for its output x [B][H][W][C] (H % 8 == 0, W % 32 == 0, C % 8 == 0):
    [B][(H / 8) (W / 32)][C / 8][16] - per 8 x 32-pixel tile and 8-channel piece the 8 sums, then the 8 sums of squares; summed in
    `dtype` (float32: as the convolution's epilogue holds them)"""
    B, H, W, C = x.shape
    t = x.reshape(B, H // 8, 8, W // 32, 32, C // 8, 8).transpose(0, 1, 3, 5, 2, 4, 6).reshape(B, (H // 8) * (W // 32), C // 8, 256, 8)
    t = t.astype(dtype)
    return np.concatenate((t.sum(3, dtype=dtype), (t * t).sum(3, dtype=dtype)), -1).astype(F32)


def stats_from_psum(ps_list, cnt):
    """float64 group sums of the float32 piece sums of the concatenated sources -> (s, q) [B][32]"""
    s = np.concatenate([p[..., :8].astype(F64).sum(1).reshape(p.shape[0], -1) for p in ps_list], 1)      # [B][C]
    q = np.concatenate([p[..., 8:].astype(F64).sum(1).reshape(p.shape[0], -1) for p in ps_list], 1)
    B, C = s.shape
    return s.reshape(B, 32, C // 32).sum(2), q.reshape(B, 32, C // 32).sum(2)


# ------------------------------------------------------------------------------------------------------------ exact family
MEANS = (0.0, 1.0, -2.0, 64.0, 4.0, -128.0, 0.5, -8.0, 32.0, 0.0, -64.0)     # powers of two: mean * anything is one rounding at most
SPREAD = {0.0: 1.0, 1.0: 0.5, -2.0: 1.0, 64.0: 0.5, 4.0: 2.0, -128.0: 1.0, 0.5: 0.25, -8.0: 0.5, 32.0: 1.0, -64.0: 0.5}


def exact_input(B, H, W, C, seed):
    """x float64 [B][H][W][C]: group (b, g) holds m + d k, m and d powers of two (|m| / d up to 128: a large mean and a tiny spread),
    k integers in [-3, 3] in +- pairs (an odd cnt adds one 0), shuffled: the group's sum is cnt m exactly, so its mean is m; every
    fifth group is constant (variance exactly 0).  All values are representable in bf16."""
    rng = np.random.default_rng(seed)
    cpg, n = C // 32, H * W * (C // 32)
    x = np.empty((B, H * W, 32, cpg))
    for b in range(B):
        for g in range(32):
            m = MEANS[(b * 7 + g + seed) % len(MEANS)]
            half = rng.integers(1, 4, n // 2)
            k = np.concatenate((half, -half, np.zeros(n % 2, dtype=half.dtype)))
            if (b + g) % 5 == 2:
                k[:] = 0
            x[b, :, g, :] = (m + SPREAD[m] * rng.permutation(k)).reshape(H * W, cpg)
    x = x.reshape(B, H, W, C)
    assert representable(x, "bf16")
    return x


def exact_params(B, C, seed, with_ss, per_group=False):
    """gamma = +-2^j, beta and shift small dyadic numbers, 1 + scale a power of two (so every product of the apply pass is exact);
    per_group: gamma and scale constant inside a group (the exact gradient: a group's sum of dxh is then its sum of dy times them)"""
    rng = np.random.default_rng(seed + 1000)
    n, rep = (32, C // 32) if per_group else (C, 1)
    gamma = np.repeat(rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(-1, 3, n), rep).astype(F32)
    beta = (rng.integers(-8, 9, C) / 2.0).astype(F32)
    ss = None
    if with_ss:
        scale = np.repeat(rng.choice([0.0, 1.0, -0.5, 3.0, -2.0], (B, n)), rep, 1)
        ss = np.concatenate((scale, rng.integers(-8, 9, (B, C)) / 4.0), 1).astype(F32)
    return gamma, beta, ss


def resample_raw(x, mode):
    """R(x) with the kernels' float32 steps (the 2x2 average: taps (0,0), (0,1), (1,0), (1,1) added in that order, then * 0.25)"""
    B, H, W, C = x.shape
    if mode == 1:
        Ho, Wo = H // 2, W // 2
        t = x[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).astype(F32)
        return (((t[:, :, 0, :, 0] + t[:, :, 0, :, 1]) + t[:, :, 1, :, 0]) + t[:, :, 1, :, 1]) * F32(0.25)
    if mode == 2:
        return np.repeat(np.repeat(x, 2, 1), 2, 2).astype(F32)
    return x.astype(F32)


def emulate_apply(x, mean32, rstd32, gamma, beta, ss, ss_shared, mode, contracted=False):
    """the apply kernels' float32 steps with silu = 0, on x float64 [B][H][W][C] (values float32 holds exactly):
    ca = rstd * gamma;  cb = beta - mean * ca (contracted: one fma);  u = fma(x, ca, cb);  u = fma(u, 1 + scale, shift);  R(u).
    Returns (float32 result before the store rounding, every fma's float64 argument was exact)."""
    B, H, W, C = x.shape
    grp = np.arange(C) // (C // 32)
    mean, rstd = mean32[:, grp], rstd32[:, grp]                                    # [B][C] float32
    ca = rstd * gamma[None]
    exact = True
    if contracted:
        cb, ok = fma32(-mean, ca, beta[None])
        exact = exact and ok
    else:
        cb = beta[None] - mean * ca
    uu, ok = fma32(x.astype(F32), ca[:, None, None, :], cb[:, None, None, :])
    exact = exact and ok
    if ss is not None:
        row = np.broadcast_to(ss[:1], (B, 2 * C)) if ss_shared else ss
        sc = F32(1.0) + row[:, :C]
        uu, ok = fma32(uu, sc[:, None, None, :], row[:, None, None, C:])
        exact = exact and ok
    return resample_raw(uu, mode), exact


def apply_rational(xv, mean32, rstd32, gamma, beta, scale, shift):
    """one element of the apply pass in exact rational arithmetic, rounded to float32 where the kernel rounds"""
    ca = round_f32(Fraction(float(rstd32)) * Fraction(float(gamma)))
    cb = round_f32(Fraction(float(beta)) - round_f32(Fraction(float(mean32)) * ca))
    uu = round_f32(Fraction(float(xv)) * ca + cb)
    if scale is not None:
        sc = round_f32(1 + Fraction(float(scale)))
        uu = round_f32(uu * sc + Fraction(float(shift)))
    return uu


# ---- exact gradient: constant groups (xh = 0, so the second mean is exactly 0) and integer gradients whose group mean is dyadic
def exact_grad_input(B, H, W, C, seed):
    """x constant per (sample, group): variance exactly 0, rstd = (float)(1 / sqrt(eps)), xh = fma(m, rstd, -m rstd) = 0"""
    cpg = C // 32
    m = np.array([[MEANS[(b * 5 + g + seed) % len(MEANS)] for g in range(32)] for b in range(B)])
    return np.broadcast_to(np.repeat(m, cpg, 1)[:, None, None, :], (B, H, W, C)).copy()


def exact_grad_dy(B, Ho, Wo, C, seed):
    """integer dy [B][Ho][Wo][C]: per group an offset (a power of two) plus +- pairs, so every group sum is (Ho Wo C / 32) * offset"""
    rng = np.random.default_rng(seed + 2000)
    cpg, n = C // 32, Ho * Wo * (C // 32)
    dy = np.empty((B, Ho * Wo, 32, cpg))
    off = np.empty((B, 32))
    for b in range(B):
        for g in range(32):
            off[b, g] = (0.0, 4.0, -8.0, 16.0)[(b + g + seed) % 4]
            half = rng.integers(1, 6, n // 2)
            k = np.concatenate((half, -half, np.zeros(n % 2, dtype=half.dtype)))
            dy[b, :, g, :] = (off[b, g] + rng.permutation(k)).reshape(Ho * Wo, cpg)
    return dy.reshape(B, Ho, Wo, C), off


def adjoint(g, H, W, mode):
    """R^T g in the kernels' float32 steps: mode 1 g[p / 2] * 0.25; mode 2 the four copies added in order (0,0), (0,1), (1,0), (1,1)"""
    g = g.astype(F32)
    if mode == 1:
        return np.repeat(np.repeat(g, 2, 1), 2, 2) * F32(0.25)
    if mode == 2:
        B, Ho, Wo, C = g.shape
        t = g.reshape(B, H, 2, W, 2, C)
        return ((t[:, :, 0, :, 0] + t[:, :, 0, :, 1]) + t[:, :, 1, :, 0]) + t[:, :, 1, :, 1]
    return g


def emulate_grad_const(dy, rstd32, gamma, ss, ss_shared, mode, H, W, dres, add, run=64):
    """the gradient kernels' float32 steps for constant groups and silu = 0: dxh = R^T dy * (gamma (1 + scale)) (exact), m1 = the
    group mean of dxh (exact sums; the quotient must be exact too), xh = 0 and m2 = 0, out = rstd * (dxh - m1) [+ R^T dres] [+ add],
    one float32 rounding each.  Returns (out float32, m1 float32 [B][32], the means and the running sums were exact): a thread adds at
    most `run` = ceil(ppc / RY) values of dxh in float32 - multiples of 2^-6 whose sum must stay below 2^18 - before float64 takes over."""
    B, C = dy.shape[0], dy.shape[3]
    cpg = C // 32
    grp = np.arange(C) // cpg
    gs = np.broadcast_to(gamma[None], (B, C)).astype(F32)
    if ss is not None:
        row = np.broadcast_to(ss[:1], (B, 2 * C)) if ss_shared else ss
        gs = gs * (F32(1.0) + row[:, :C])
    dxh = adjoint(dy, H, W, mode) * gs[:, None, None, :]
    d64 = dxh.astype(F64).reshape(B, H * W, 32, cpg)
    tot, cnt = d64.sum((1, 3)), H * W * cpg
    m1 = tot / cnt
    exact = bool((m1 * cnt == tot).all()) and bool((m1.astype(F32).astype(F64) == m1).all())
    exact = exact and bool((d64 * 64 == np.round(d64 * 64)).all()) and float(np.abs(d64).max()) * run < 2.0 ** 18
    out = rstd32[:, grp][:, None, None, :] * (dxh - m1.astype(F32)[:, grp][:, None, None, :])
    if dres is not None:
        out = out + adjoint(dres, H, W, mode)
    if add is not None:
        out = out + add.astype(F32)
    return out.astype(F32), m1.astype(F32), exact


# ------------------------------------------------------------------------------------------------------------ float64 references
def silu64(a):
    return a / (1.0 + np.exp(-a))


def resample64(a, mode):
    B, H, W, C = a.shape
    if mode == 1:
        Ho, Wo = H // 2, W // 2
        return a[:, :2 * Ho, :2 * Wo].reshape(B, Ho, 2, Wo, 2, C).mean((2, 4))
    if mode == 2:
        return np.repeat(np.repeat(a, 2, 1), 2, 2)
    return a


def adjoint64(g, H, W, mode):
    if mode == 1:
        return np.repeat(np.repeat(g, 2, 1), 2, 2) * 0.25
    if mode == 2:
        B, Ho, Wo, C = g.shape
        return g.reshape(B, H, 2, W, 2, C).sum((2, 4))
    return g


def exp_deviation(args):
    """the largest relative deviation of float32 exp (of the float32 argument) from float64 exp over `args` (those >= -80)"""
    a = np.asarray(args, dtype=F64).ravel()
    a = a[(a >= -80) & (a <= 80)]
    if a.size == 0:
        return 0.0
    e64 = np.exp(a)
    return float(np.max(np.abs(np.exp(a.astype(F32)).astype(F64) - e64) / e64))


def forward_reference(x, gamma, beta, ss, ss_shared, silu, mode, dt, bf16_group_sums, psum_err=0.0, exp_eps=None):
    """x float64 [B][H][W][C] (rounded to the storage type) -> (y, xr, mean, rstd, bound_y, bound_xr, bound_mean, bound_rstd, dev),
    everything float64.  The bounds follow the kernels' rounding points (module docstring of tests/test_gpu_groupnorm.py):
      statistics   float64 sums (2^-40 relative covers them).  bf16 group route (bf16_group_sums): 8 values are summed in float32 first,
                   ds <= 7 v S1, dq <= 8 v S2 (S1 = sum |x|, S2 = sum x^2 of the group); piece sums (psum_err = 256): ds <= 256 v S1,
                   dq <= 256 v S2.  dmean = ds / cnt + v |mean| (stored float32); dvar = dq / cnt + 2 |mean| ds / cnt; with t = dvar /
                   (var + eps) the relative error of rstd is r = t / (2 (1 - t)) + v
      apply        ca = rstd gamma (v), cb = beta - mean ca (2 v, of size |mean| rstd |gamma|: the cancellation term), u = fma (v):
                   E1 = |xh gamma| (r + 2 v) + dmean rstd |gamma| + 2 v |mean| rstd |gamma| + v (|beta| + |u|)
                   scale-shift: sc = 1 + s (v), u2 = fma (v):  E2 = E1 |sc| + v |u sc| + v |u2|
                   SiLU a = u / (1 + e), e = exp(-u):  E3 = 1.1 E2 + |a| (eps_exp e / (1 + e) + 4 v)   (|silu'| <= 1.1)
                   2x2 average: three float32 additions, E = mean(E3) + 3 v mean|a|;  store: u (|y| + E)
      xr           3 v mean|x| (mode 1) + u |xr|"""
    B, H, W, C = x.shape
    cpg = C // 32
    grp = np.arange(C) // cpg
    s, q, cnt = group_sums(x)
    mean, var = s / cnt, np.maximum(q / cnt - (s / cnt) ** 2, 0.0)
    xg = x.reshape(B, H * W, 32, cpg)
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))                      # (the two-pass form: the reference has no cancellation)
    rstd = 1.0 / np.sqrt(var + EPS)
    S1, S2 = np.abs(xg).sum((1, 3)), (xg * xg).sum((1, 3))
    k1 = max(7.0 if bf16_group_sums else 0.0, psum_err)
    k2 = max(8.0 if bf16_group_sums else 0.0, psum_err)
    ds, dq = (k1 * V + 2.0 ** -40) * S1, (k2 * V + 2.0 ** -40) * S2
    dmean = ds / cnt + V * np.abs(mean)
    dvar = dq / cnt + 2 * np.abs(mean) * ds / cnt
    t = np.minimum(dvar / (var + EPS), 0.9)
    r = t / (2 * (1 - t)) + V                                                    # ((1 - t)^-1/2 - 1 <= t / (2 (1 - t)))
    mc, rc, dmc, rrc = (t[:, grp][:, None, None, :] for t in (mean, rstd, dmean, r))
    g_, b_ = gamma.astype(F64)[None, None, None, :], beta.astype(F64)[None, None, None, :]
    xh = (x - mc) * rc
    uu = xh * g_ + b_
    E = np.abs(xh * g_) * (rrc + 2 * V) + dmc * rc * np.abs(g_) + 2 * V * np.abs(mc) * rc * np.abs(g_) + V * (np.abs(b_) + np.abs(uu))
    if ss is not None:
        row = (np.broadcast_to(ss[:1], (B, 2 * C)) if ss_shared else ss).astype(F64)
        sc, sh = 1.0 + row[:, None, None, :C], row[:, None, None, C:]
        u2 = uu * sc + sh
        E = E * np.abs(sc) + V * np.abs(uu * sc) + V * np.abs(u2)
        uu = u2
    dev = 0.0
    if silu:
        dev = exp_deviation(-uu)
        eps_exp = 4 * dev if exp_eps is None else exp_eps
        e = np.exp(-np.clip(uu, -700, 700))
        a = uu / (1.0 + e)
        E = 1.1 * E + np.abs(a) * (eps_exp * e / (1 + e) + 4 * V)
        uu = a
    y = resample64(uu, mode)
    Ey = resample64(E, mode) + (3 * V * resample64(np.abs(uu), mode) if mode == 1 else 0.0)
    by = Ey + U[dt] * (np.abs(y) + Ey)
    xr = resample64(x, mode)
    bxr = (3 * V * resample64(np.abs(x), mode) if mode == 1 else 0.0) + U[dt] * np.abs(xr) * (1 + 4 * V)
    return dict(y=y, xr=xr, mean=mean, rstd=rstd, by=by, bxr=bxr, bmean=dmean, brstd=r * rstd, dev=dev)


def grad_reference(x, mean32, rstd32, gamma, beta, ss, ss_shared, silu, mode, dy, dres, add, dt, run, exp_eps=None):
    """the input gradient in float64 with the float32 statistics it is handed as operands, and its element-wise bound.
    x, dy, dres, add float64 (rounded to the storage type); run = ceil(ppc / RY), a thread's float32 run of the partial sums.
      gs = gamma (1 + scale) (2 v), bs = fma (2 v);  xh = fma(x, rstd, -mean rstd):  Exh = v (|mean| rstd + |xh|) - the cancellation
      term;  pre = fma(xh, gs, bs):  Epre = Exh |gs| + 2 v |xh gs| + 2 v |bs| + v |pre|
      sg = 1 / (1 + e):  dsg = sg ((1 - sg) eps_exp + 4 v);   D = sg fma(pre, 1 - sg, 1)  (|dD / dpre| <= 0.5, |dD / dsg| <= 1 + |pre|):
      ED = 0.5 Epre + (1 + |pre|) dsg + 4 v (|D| + sg |pre| (1 - sg))
      da = R^T dy (mode 2: three float32 additions, 3 v sum|dy|);  dxh = da D gs:  Edxh = |da gs| ED + |D gs| Eda + 5 v |dxh|
      m1, m2: float32 runs of `run` terms, then float64, stored float32:
      Em1 = mean(Edxh) + run v mean|dxh| + v |m1|;   Em2 = mean(Edxh |xh| + |dxh| Exh) + (run + 1) v mean|dxh xh| + v |m2|
      out = rstd (dxh - m1 - xh m2):  E = rstd (Edxh + Em1 + Exh |m2| + |xh| Em2 + 3 v (|dxh| + |m1| + |xh m2|)) + v |out|
      + R^T dres (mode 2: 3 v sum|dres|) + add, two float32 additions (2 v of the sizes), store u |dx|"""
    B, H, W, C = x.shape
    cpg = C // 32
    grp = np.arange(C) // cpg
    mc, rc = (t.astype(F64)[:, grp][:, None, None, :] for t in (mean32, rstd32))
    g_ = np.broadcast_to(gamma.astype(F64)[None, None, None, :], (B, 1, 1, C))
    bs = np.broadcast_to(beta.astype(F64)[None, None, None, :], (B, 1, 1, C))
    if ss is not None:
        row = (np.broadcast_to(ss[:1], (B, 2 * C)) if ss_shared else ss).astype(F64)
        g_ = g_ * (1.0 + row[:, None, None, :C])
        bs = bs * (1.0 + row[:, None, None, :C]) + row[:, None, None, C:]
    xh = (x - mc) * rc
    Exh = V * (np.abs(mc) * rc + np.abs(xh))
    da = adjoint64(dy, H, W, mode)
    Eda = 3 * V * adjoint64(np.abs(dy), H, W, mode) if mode == 2 else 0.0
    dev = 0.0
    if silu:
        pre = xh * g_ + bs
        Epre = Exh * np.abs(g_) + 2 * V * np.abs(xh * g_) + 2 * V * np.abs(bs) + V * np.abs(pre)
        dev = exp_deviation(-pre)
        eps_exp = 4 * dev if exp_eps is None else exp_eps
        sg = 1.0 / (1.0 + np.exp(-np.clip(pre, -700, 700)))
        D = sg * (1.0 + pre * (1.0 - sg))
        dsg = sg * ((1 - sg) * eps_exp + 4 * V)
        ED = 0.5 * Epre + (1 + np.abs(pre)) * dsg + 4 * V * (np.abs(D) + sg * np.abs(pre) * (1 - sg))
    else:
        D, ED = 1.0, 0.0
    dxh = da * D * g_
    Edxh = np.abs(da * g_) * ED + np.abs(D * g_) * Eda + 5 * V * np.abs(dxh)

    def gmean(a):
        return np.broadcast_to(a, x.shape).reshape(B, H * W, 32, cpg).mean((1, 3))[:, grp][:, None, None, :]

    m1, m2 = gmean(dxh), gmean(dxh * xh)
    Em1 = gmean(Edxh) + run * V * gmean(np.abs(dxh)) + V * np.abs(m1)
    Em2 = gmean(Edxh * np.abs(xh) + np.abs(dxh) * Exh) + (run + 1) * V * gmean(np.abs(dxh * xh)) + V * np.abs(m2)
    out = rc * (dxh - m1 - xh * m2)
    E = rc * (Edxh + Em1 + Exh * np.abs(m2) + np.abs(xh) * Em2 + 3 * V * (np.abs(dxh) + np.abs(m1) + np.abs(xh * m2))) + V * np.abs(out)
    mag = np.abs(out)
    if dres is not None:
        out = out + adjoint64(dres, H, W, mode)
        mag = mag + adjoint64(np.abs(dres), H, W, mode)
        E = E + (3 * V * adjoint64(np.abs(dres), H, W, mode) if mode == 2 else 0.0)
    if add is not None:
        out = out + add
        mag = mag + np.abs(add)
    E = E + 2 * V * mag
    return out, E + U[dt] * (np.abs(out) + E), dev


# ------------------------------------------------------------------------------------------------------------ the case tables
# (tests/test_gpu_groupnorm.py runs them, tests/test_groupnorm_host.py proves the exact ones; a case's index is its seed)
# B, H, W, C0, C1, dtype, mode, ss ("none", "2C": ss_ld = 2 C, "shared": ss_ld = 0, "wide": ss_ld = 2 C + 64, the slice 32 floats in), xr
EXACT_CASES = [
    (2, 1, 1, 32, 0, "f32", 0, "none", 0),           # HW = 1, cnt = 1: every group constant; per-channel route, 64 rows without a pixel
    (2, 1, 1, 32, 0, "bf16", 2, "2C", 1),
    (1, 1, 7, 96, 0, "bf16", 0, "shared", 0),        # a piece spans two groups
    (1, 1, 7, 96, 0, "f32", 2, "wide", 1),
    (2, 3, 8, 128, 0, "f32", 0, "2C", 0),            # group kernels in f32 ...
    (2, 3, 8, 128, 0, "bf16", 0, "none", 0),         # ... per-channel in bf16
    (2, 5, 9, 256, 0, "bf16", 0, "wide", 0),         # W = 9: the 8-pixel walk's clamped loads and its break
    (2, 5, 9, 100, 156, "f32", 0, "2C", 0),          # a group across the source boundary
    (2, 2, 12, 200, 312, "bf16", 0, "shared", 0),
    (1, 2, 12, 768, 0, "bf16", 0, "none", 0),        # 96 pieces x 5 rows = 480 threads
    (1, 2, 12, 768, 0, "f32", 2, "2C", 1),           # 192 x 2 = 384
    (2, 6, 10, 2048, 0, "bf16", 1, "2C", 1),         # Wo = 5
    (2, 6, 10, 2048, 0, "f32", 0, "none", 0),        # RY = 1
    (1, 2, 2, 4096, 0, "f32", 1, "none", 1),         # 1024 pieces; mode 1 at 2 x 2
    (1, 2, 2, 8192, 0, "bf16", 0, "2C", 0),
    (2, 5, 7, 256, 0, "bf16", 1, "shared", 1),       # mode 1 at odd sizes: floors like avg_pool2d, statistics over every pixel
    (2, 5, 7, 256, 0, "f32", 1, "none", 1),
    (1, 3, 5, 768, 0, "bf16", 2, "wide", 1),         # mode 2, Wo = 10
    (1, 3, 5, 256, 512, "f32", 2, "none", 1),
    (1, 9, 10, 2048, 0, "bf16", 0, "none", 0),       # fewer chunks than HW / (4 RY)
    (2, 91, 91, 256, 0, "bf16", 0, "2C", 0),         # 128 chunks, the last one ragged
    (2, 3, 8, 128, 128, "bf16", 0, "none", 0),
    (2, 6, 10, 96, 0, "f32", 1, "2C", 1),
    (2, 5, 9, 32, 0, "bf16", 2, "none", 1),
    (2, 2, 12, 256, 512, "bf16", 1, "2C", 1),
    (3, 21846, 1, 256, 0, "bf16", 0, "none", 0),     # B * Ho = 65538: a fast shape on the per-channel kernels
    (1, 32768, 1, 256, 0, "bf16", 2, "none", 0),     # fast by B * H, per-channel by B * Ho
]
# B, H, W, C0, C1, sums of source 0, sums of source 1 (exact family, bf16, seed = H + C0)
PSUM_CASES = [(2, 8, 32, 256, 0, 1, 0), (2, 16, 64, 256, 0, 1, 0), (2, 16, 64, 256, 512, 1, 1), (2, 8, 32, 256, 256, 1, 1),
              (2, 8, 32, 128, 0, 1, 0), (2, 16, 64, 128, 256, 1, 1),       # legal, per-channel kernels: the own pass
              (2, 16, 64, 256, 512, 1, 0), (2, 8, 32, 256, 512, 0, 1)]      # one source without sums: the own pass
# B, H, W, C0, C1, dtype, mode, ss, silu, regime (gaussian_input)
GAUSS_CASES = [
    (2, 5, 9, 32, 0, "f32", 0, "2C", 1, 0),
    (2, 6, 10, 96, 0, "bf16", 1, "none", 1, 2),
    (2, 3, 8, 128, 0, "f32", 2, "wide", 1, 1),
    (2, 3, 8, 128, 0, "bf16", 0, "shared", 1, 1),
    (2, 5, 9, 256, 0, "bf16", 0, "2C", 1, 1),
    (2, 5, 9, 100, 156, "f32", 0, "none", 1, 2),
    (2, 2, 12, 200, 312, "bf16", 2, "2C", 1, 0),
    (1, 6, 10, 768, 0, "bf16", 1, "wide", 1, 1),
    (1, 6, 10, 768, 0, "f32", 0, "shared", 0, 2),
    (1, 3, 8, 2048, 0, "bf16", 0, "none", 1, 1),
    (1, 5, 7, 2048, 0, "f32", 1, "2C", 1, 0),
    (1, 2, 2, 4096, 0, "f32", 0, "none", 1, 1),
    (1, 2, 2, 8192, 0, "bf16", 2, "2C", 1, 2),
    (1, 91, 91, 256, 0, "bf16", 0, "2C", 1, 1),
    (2, 1, 7, 256, 512, "bf16", 0, "none", 1, 1),
    (2, 1, 1, 256, 0, "f32", 2, "none", 1, 0),
]
# B, H, W, C0, C1, dtype, mode, ss, dres, add0, add1
GRAD_CASES = [
    (2, 5, 9, 256, 0, "bf16", 0, "2C", 1, 1, 0),
    (2, 6, 10, 96, 0, "f32", 1, "none", 1, 0, 0),
    (1, 3, 5, 768, 0, "bf16", 2, "wide", 1, 1, 0),
    (2, 1, 1, 32, 0, "f32", 0, "none", 0, 0, 0),
    (1, 2, 2, 8192, 0, "bf16", 1, "2C", 1, 0, 0),    # 1024-thread workgroups, 64 KiB of dynamic LDS
    (1, 2, 2, 4096, 0, "f32", 0, "none", 0, 1, 0),
    (2, 2, 12, 2048, 0, "bf16", 0, "shared", 0, 0, 0),
    (2, 5, 9, 100, 156, "f32", 0, "2C", 0, 1, 0),
    (2, 2, 12, 200, 312, "bf16", 2, "none", 1, 0, 1),
    (2, 3, 8, 128, 128, "bf16", 0, "none", 0, 1, 1),
    (1, 1, 7, 256, 512, "f32", 0, "wide", 1, 1, 1),
    (1, 2, 12, 768, 0, "f32", 0, "2C", 0, 0, 0),
    (1, 91, 91, 256, 0, "bf16", 0, "none", 1, 0, 0),
    (3, 21846, 1, 256, 0, "bf16", 0, "none", 0, 0, 0),   # two sample ranges of the last kernel
]


def gaussian_input(B, H, W, C, regime, seed, dt="bf16"):
    """regime 0: unit Gaussians; 1: spread 1 around a per-(sample, group) mean of up to 60; 2: spread 0.5 around per-channel means
    30 N(0, 1) (the regime of tests/test_gpu_diffusion.py).  Rounded to the storage type, float64."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(B, H, W, C))
    if regime == 1:
        x = x + np.repeat(rng.uniform(-60, 60, (B, 32)), C // 32, 1)[:, None, None, :]
    elif regime == 2:
        x = 0.5 * x + 30 * rng.normal(size=(1, 1, 1, C))
    return to_storage(x, dt).double().numpy()


def gaussian_params(B, C, seed, with_ss):
    """gamma, beta, scale-shift (float32) that spread the pre-activations over [-20, 20] and beyond: SiLU's tails are hit"""
    rng = np.random.default_rng(seed + 3000)
    sign = rng.choice([-1.0, 1.0], C)
    if with_ss:
        gamma, beta = sign * rng.uniform(0.5, 1.5, C), rng.uniform(-1, 1, C)
        ss = np.concatenate((rng.uniform(-7, 5, (B, C)), rng.uniform(-2, 2, (B, C))), 1).astype(F32)
    else:
        gamma, beta, ss = sign * rng.uniform(2, 7, C), rng.uniform(-2, 2, C), None
    return gamma.astype(F32), beta.astype(F32), ss
