"""The twin of the small kernels that hold the guided-diffusion path together: the sampler steps (csrc/sampler.hip), the two f32
kernels of the timestep path (csrc/unet.hip) and the secondary model's glue (csrc/secondary.hip).  A plain module, imported by name by
tests/test_diffusion_kernels_host.py and tests/test_gpu_diffusion_kernels.py; it holds no test and no fixture.

For every operation: a float64 evaluation and, where the order is the contract, a float32 restatement in numpy - every operation on
float32 arrays, so every product, sum and quotient rounds once - in the order of gaussian_diffusion.py as oracle/diffusion.py restates
it.  The restatements of the order-pinned sampler steps take contract=True / False: True fuses exactly what the build fused before
contraction was switched off in those kernels (read off its assembly: a b - c d became fma(a, b, -(c d)), e - k g became fma(-k, g, e),
the multistep sum became fma(w_i, e_i, sum), s + k5 noise became fma(k5, noise, s); pred k3 + k4 eps and the final mask blend were
left as two products and a sum).  fma here is the float64 product and sum rounded to float32 once; the double rounding that can
differ from a true fma in about one element in 2^29 does not matter to what the flag is for (telling the two builds apart).

Bounds come from the float64 result and the stated rounding model only: v = 2^-24 (unit roundoff) times the magnitudes times the
number of roundings on the path.  Library functions on the device: no accuracy table ships with the toolchain, so the allowance is a
stated number of float32 units in the last place of the float64 result - EXP_ULPS = 3 for expf, TRIG_ULPS = 4 for sinf and cosf (the
OpenCL C table the device library is built to) - on top of what the argument's own error contributes.  A float32 result below the
smallest normal number (TINY = 2^-126) may be flushed, and expf of an argument above 88.7 is infinite where the float64 value is
finite: every bound that crosses such a value carries TINY as an absolute term.

The inputs of every GPU case are built here (seeded), so the host file judges mutants on exactly those."""
import math

import numpy as np

V = 2.0 ** -24
TINY = 2.0 ** -126
EXP_ULPS = 3
TRIG_ULPS = 4
F32, BF16 = 0, 1                       # maua_dtype
EPC = {F32: 4, BF16: 8}                # elements per 16-byte piece


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def f64(a):
    return np.asarray(a, dtype=np.float64)


def normal(shape, seed):
    return f32(np.random.default_rng(seed).standard_normal(shape))


def ulp32(y):
    """one float32 unit in the last place at |y| (float64 in, float64 out; at least the smallest subnormal)"""
    return f64(np.spacing(np.abs(f64(y)).astype(np.float32)))


def fma(a, b, c):
    return (f64(a) * f64(b) + f64(c)).astype(np.float32)


def judge(got, expect):
    """The one comparison both test files make.  expect = ("exact", want32): bit for bit up to the sign of zero, NaN equals NaN ->
    0.0 or inf; ("bound", ref64, bound): the worst error / bound (a non-finite error -> inf).  Accepted means <= 1."""
    got = np.asarray(got)
    if expect[0] == "exact":
        want = np.asarray(expect[1])
        return 0.0 if got.shape == want.shape and np.array_equal(got, want, equal_nan=True) else math.inf
    _, ref, bound = expect
    err = np.abs(f64(got) - ref)
    if got.shape != np.shape(ref) or not np.isfinite(err).all():
        return math.inf
    return float(np.max(np.where(err > 0, err / np.maximum(bound, 1e-300), 0.0))) if err.size else 0.0


# ------------------------------------------------------------------------------------------------------------- bf16
def bf16_round(a):
    """float32 -> the float32 value of its bfloat16 (one round to nearest even; finite values and NaN)"""
    a = f32(a)
    bits = a.view(np.uint32).astype(np.uint64)
    r = ((bits + 0x7FFF + ((bits >> 16) & 1)) >> 16).astype(np.uint32) << 16
    out = r.astype(np.uint32).view(np.float32).reshape(a.shape)
    return np.where(np.isnan(a), np.float32(np.nan), out).astype(np.float32)


def store(a, dtype):
    """what a kernel's store leaves of the float32 value a: itself, or one RNE to bf16"""
    return bf16_round(a) if dtype == BF16 else f32(a)


def store_bound(ref, dtype):
    """the error a store adds to a value near ref: none in f32 (the value is the float32 number), half a bf16 unit in bf16"""
    return np.abs(f64(ref)) * 2.0 ** -8 + TINY if dtype == BF16 else 0.0 * np.abs(f64(ref))


# ------------------------------------------------------------------------------------------------------------- schedule
class Schedule:
    """The float64 tables of the respaced process (linear betas over `steps` timesteps, every stride-th kept): what
    gaussian_diffusion.py / respace.py build, restated independently of oracle/diffusion.py and maua_amd/diffusion.py."""

    def __init__(self, steps=1000, n=100):
        base = np.linspace(1000 / steps * 0.0001, 1000 / steps * 0.02, steps, dtype=np.float64)
        stride = next(i for i in range(1, steps) if len(range(0, steps, i)) == n)
        ac_full, last, betas = np.cumprod(1.0 - base), 1.0, []
        for i in range(0, steps, stride):
            betas.append(1 - ac_full[i] / last)
            last = ac_full[i]
        self.betas = b = np.array(betas)
        self.ac = np.cumprod(1.0 - b)
        self.ac_prev = np.append(1.0, self.ac[:-1])
        self.sqrt_ac, self.sqrt_1mac = np.sqrt(self.ac), np.sqrt(1.0 - self.ac)
        self.recip, self.recipm1 = np.sqrt(1.0 / self.ac), np.sqrt(1.0 / self.ac - 1)
        pv = b * (1.0 - self.ac_prev) / (1.0 - self.ac)
        self.post_logvar = np.log(np.append(pv[1], pv[1:]))
        self.coef1 = b * np.sqrt(self.ac_prev) / (1.0 - self.ac)
        self.coef2 = (1.0 - self.ac_prev) * np.sqrt(1.0 - b) / (1.0 - self.ac)
        self.log_betas = np.log(b)


SCH = Schedule()
T_OF_SAMPLE = (17, 0, 99, 5, 60)        # sample 1 sits at t = 0 (mask 0) beside samples at t > 0; every row differs


def ddim_coef(t, eta=0.0, sch=SCH):
    """maua_ddim_step's / maua_plms_eps's [len(t)][8] rows as ddim_sample evaluates them: float32 values taken from the float64
    tables, then float32 arithmetic (each operation rounded once)."""
    t = np.asarray(t)
    ab, abp, one, e = f32(sch.ac[t]), f32(sch.ac_prev[t]), np.float32(1), np.float32(eta)
    sigma = e * np.sqrt((one - abp) / (one - ab)) * np.sqrt(one - ab / abp)
    cf = np.zeros((len(t), 8), np.float32)
    cf[:, 0], cf[:, 1] = f32(sch.recip[t]), f32(sch.recipm1[t])
    cf[:, 2], cf[:, 3] = np.sqrt(one - ab), np.sqrt(abp)
    cf[:, 4] = np.sqrt(one - abp - sigma * sigma)
    cf[:, 5] = sigma * f32(t != 0)
    return cf


def p_coef(t, sch=SCH):
    t = np.asarray(t)
    cf = np.zeros((len(t), 8), np.float32)
    for i, tab in enumerate((sch.recip, sch.recipm1, sch.coef1, sch.coef2, sch.post_logvar, sch.log_betas)):
        cf[:, i] = f32(tab[t])
    cf[:, 6] = f32(t != 0)
    return cf


def plms_coef(t, sch=SCH):
    t = np.asarray(t)
    abp, one = f32(sch.ac_prev[t]), np.float32(1)
    cf = np.zeros((len(t), 8), np.float32)
    cf[:, 0], cf[:, 1], cf[:, 2], cf[:, 3], cf[:, 4] = f32(sch.recip[t]), f32(sch.recipm1[t]), np.sqrt(abp), np.sqrt(one - abp), f32(t != 0)
    return cf


def q_coef(t, sch=SCH):
    t = np.asarray(t)
    return f32(np.stack([sch.sqrt_ac[t], sch.sqrt_1mac[t]], 1))


# ------------------------------------------------------------------------------------------------------------- sampler cases
SAMPLER_SHAPES = ((3, 3, 85), (1, 3, 1), (2, 1, 64), (5, 3, 100))     # (B, C, HW): 765 = a partial last block, rows of 255 = sample
PLMS_WEIGHTS = (((1.0,), 1.0), ((1.0, 1.0), 2.0), ((3.0, -1.0), 2.0), ((23.0, -16.0, 5.0), 12.0), ((55.0, -59.0, 37.0, -9.0), 24.0))


def cms(C):
    return (C, 2 * C, 2 * C + 1)


def sampler_case(B, C, HW, Cm, nan_rest=True, seed=0):
    """x, model_out [B][Cm][HW] (channels C.. NaN when nan_rest: ddim and plms never read them), grad, noise, pred, four epsilons"""
    s = 1000 * B + 100 * C + HW + 7 * Cm + seed
    mo = normal((B, Cm, HW), s + 1)
    if nan_rest:
        mo[:, C:] = np.nan
    return dict(B=B, C=C, HW=HW, Cm=Cm, x=normal((B, C, HW), s), mo=mo, grad=normal((B, C, HW), s + 2) * np.float32(3),
                noise=normal((B, C, HW), s + 3), pred=normal((B, C, HW), s + 4), t=np.array(T_OF_SAMPLE[:B]) if B > 1 else np.array([50]),
                eps=[normal((B, C, HW), s + 5 + i) for i in range(4)])


def _index(B, C, HW, Cm, mut):
    """each element's sample index, its offset in the sample and its model-output index, as the kernels compute them (flat);
    mut: 'idx+1' / 'idx-1' = the sample index from idx / (chw + 1) / (chw - 1), 'stride_C' = the model output strided by C"""
    chw = C * HW
    idx = np.arange(B * chw)
    b = np.minimum(idx // (chw + {"idx+1": 1, "idx-1": -1}.get(mut, 0)), B - 1)
    rem = idx - b * chw
    mi = np.clip(b * (C if mut == "stride_C" else Cm) * HW + rem, 0, B * Cm * HW - 1)
    return b, rem, mi


def _flat(c):
    return [f32(c[k]).reshape(-1) for k in ("x", "grad", "noise")]


def ddim_step32(c, cf, grad=True, noise=True, contract=False, mut=None):
    """gaussian_diffusion.py ddim_sample (epsilon model, clip_denoised False) -> (sample, pred_xstart), float32, every operation
    rounded once in the reference's order: pred = k0 x - k1 eps_m; with a gradient eps = (k0 x - pred) / k1, eps = eps - k2 g,
    pred = k0 x - k1 eps; eps = (k0 x - pred) / k1; sample = pred k3 + k4 eps (+ k5 noise)."""
    B, C, HW, Cm = c["B"], c["C"], c["HW"], c["Cm"]
    b, _, mi = _index(B, C, HW, Cm, mut)
    x, g, nz = _flat(c)
    k = [cf[b, i] for i in range(8)]
    em = f32(c["mo"]).reshape(-1)[mi]
    p = k[0] * x
    pred = fma(k[0], x, -(k[1] * em)) if contract else p - k[1] * em
    if grad:
        e = (p - pred) / k[1]
        e = fma(-k[2], g, e) if contract else e - k[2] * g
        pred = fma(-k[1], e, p) if contract else p - k[1] * e
    e = (p - pred) / k[1]
    s = pred * k[3] + k[4] * e
    if noise:
        s = fma(k[5], nz, s) if contract else s + k[5] * nz
    return s.reshape(B, C, HW), pred.reshape(B, C, HW)


def ddim_step64(c, cf, grad=True, noise=True):
    """the same expressions in float64 on the float32 inputs (no rounding model: the float32 chain cancels in (k0 x - pred) / k1, so
    this is a plausibility twin, not a bound's basis - the device is held to the float32 restatement bit for bit)"""
    B, C = c["B"], c["C"]
    k = [f64(cf[:, i]).reshape(B, 1, 1) for i in range(8)]
    x, em = f64(c["x"]), f64(c["mo"][:, :C])
    e = em - k[2] * f64(c["grad"]) if grad else em
    pred = k[0] * x - k[1] * e
    s = pred * k[3] + k[4] * e
    return (s + k[5] * f64(c["noise"]) if noise else s), pred


def plms_eps32(c, cf, grad=True, contract=False, mut=None):
    """plms_sample's get_model_output -> (eps, pred_xstart, pred_xstart_orig): ddim_step32's head, same order"""
    B, C, HW, Cm = c["B"], c["C"], c["HW"], c["Cm"]
    b, _, mi = _index(B, C, HW, Cm, mut)
    x, g, _ = _flat(c)
    k = [cf[b, i] for i in range(8)]
    em = f32(c["mo"]).reshape(-1)[mi]
    p = k[0] * x
    orig = fma(k[0], x, -(k[1] * em)) if contract else p - k[1] * em
    pred = orig
    if grad:
        e = (p - pred) / k[1]
        e = fma(-k[2], g, e) if contract else e - k[2] * g
        pred = fma(-k[1], e, p) if contract else p - k[1] * e
    return tuple(a.reshape(B, C, HW) for a in ((p - pred) / k[1], pred, orig))


def plms_update32(c, cf, weights, div, contract=False, mut=None):
    """eps' = (w0 e0 + w1 e1 + ...) / div left to right, pred' = k0 x - k1 eps', mean = pred' k2 + k3 eps',
    sample = mean k4 + pred (1 - k4); float32, every operation rounded once.  mut 'mask': k4 taken as 1."""
    B, C, HW = c["B"], c["C"], c["HW"]
    b = _index(B, C, HW, C, mut)[0]
    x, pr = f32(c["x"]).reshape(-1), f32(c["pred"]).reshape(-1)
    k = [cf[b, i] for i in range(8)]
    if mut == "mask":
        k[4] = np.ones_like(k[4])
    ep = np.float32(weights[0]) * c["eps"][0].reshape(-1)
    for w, e in zip(weights[1:], c["eps"][1:]):
        ep = fma(np.float32(w), e.reshape(-1), ep) if contract else ep + np.float32(w) * e.reshape(-1)
    ep = ep / np.float32(div)
    pp = fma(k[0], x, -(k[1] * ep)) if contract else k[0] * x - k[1] * ep
    mean = fma(pp, k[2], k[3] * ep) if contract else pp * k[2] + k[3] * ep
    return (mean * k[4] + pr * (np.float32(1) - k[4])).reshape(B, C, HW)


def plms_update64(c, cf, weights, div):
    B = c["B"]
    k = [f64(cf[:, i]).reshape(B, 1, 1) for i in range(8)]
    ep = sum(w * f64(e) for w, e in zip(weights, c["eps"])) / div
    pp = k[0] * f64(c["x"]) - k[1] * ep
    return (pp * k[2] + k[3] * ep) * k[4] + f64(c["pred"]) * (1 - k[4])


def axpby_rows32(x, y, ab, mut=None):
    """q_sample: out[b] = ab[b][0] x[b] + ab[b][1] y[b], two rounded products and their rounded sum (contraction changes nothing the
    build ever did here: it emitted two products and a sum before and after)"""
    B, row = x.shape[0], x[0].size
    b = np.minimum(np.arange(B * row) // (row + {"idx+1": 1, "idx-1": -1}.get(mut, 0)), B - 1)
    return (ab[b, 0] * f32(x).reshape(-1) + ab[b, 1] * f32(y).reshape(-1)).reshape(x.shape)


def axpby_rows64(x, y, ab):
    sh = (-1,) + (1,) * (x.ndim - 1)
    return f64(ab[:, 0]).reshape(sh) * f64(x) + f64(ab[:, 1]).reshape(sh) * f64(y)


def p_sample(c, cf, grad=True, mut=None):
    """gaussian_diffusion.py p_sample + p_mean_variance (learned range, epsilon model) + condition_mean.
    -> pred32 (exact: k0 x - k1 eps, rounded once each), sample32 (the float32 restatement with numpy's float32 exp) and
    ("bound", sample64, bound).  Rounding model of the sample: mean = k2 pred + k3 x (+ variance g) is exact float32 up to the
    exponential, so the float64 reference starts from the float32 mean k2 pred + k3 x; frac = (vv + 1) / 2 rounds once (d_frac = v
    |frac|), log-variance = frac k5 + (1 - frac) k4 rounds four times on top (d_lv); exp carries d_lv (and half of it for the
    standard deviation) plus EXP_ULPS; each product and sum after it rounds once.
    mut: 'idx+1' / 'idx-1' / 'mask' (k6 taken as 1) / 'frac' (frac and 1 - frac swapped in the log-variance)."""
    B, C, HW = c["B"], c["C"], c["HW"]
    chw = C * HW
    b, rem, _ = _index(B, C, HW, 2 * C, mut)
    x, g, nz = _flat(c)
    k = [cf[b, i] for i in range(8)]
    if mut == "mask":
        k[6] = np.ones_like(k[6])
    mo = f32(c["mo"]).reshape(-1)
    base = np.clip(b * 2 * chw + rem, 0, mo.size - chw - 1)
    eps, vv = mo[base], mo[base + chw]
    one, two, half = np.float32(1), np.float32(2), np.float32(0.5)
    frac = (vv + one) / two
    fa, fb = (one - frac, frac) if mut == "frac" else (frac, one - frac)
    lv = fa * k[5] + fb * k[4]
    pred = k[0] * x - k[1] * eps
    mean = k[2] * pred + k[3] * x
    s32 = mean + np.exp(lv) * g if grad else mean
    s32 = s32 + k[6] * np.exp(half * lv) * nz
    # float64 reference and bound
    k5, k4, k6 = f64(k[5]), f64(k[4]), f64(k[6])
    fr = (f64(vv) + 1) / 2
    d_fr = V * np.abs(fr)
    lv64 = fr * k5 + (1 - fr) * k4
    d_lv = np.abs(k5) * d_fr + V * np.abs(fr * k5) + np.abs(k4) * (d_fr + V * np.abs(1 - fr)) + V * np.abs((1 - fr) * k4) + V * np.abs(lv64)
    a_exp = EXP_ULPS * 2 * V
    m64, bound = f64(mean), np.zeros(x.size)
    if grad:
        tg = np.exp(lv64) * f64(g)
        bound = bound + np.abs(tg) * (d_lv + a_exp + V)
        m64 = m64 + tg
        bound = bound + V * np.abs(m64)
    tn = k6 * np.exp(0.5 * lv64) * f64(nz)
    bound = bound + np.abs(tn) * (0.5 * d_lv + a_exp + 2 * V) + TINY
    s64 = m64 + tn
    bound = bound + V * np.abs(s64)
    sh = (B, C, HW)
    return pred.reshape(sh), s32.reshape(sh), ("bound", s64.reshape(sh), bound.reshape(sh))


def mse_guide_grad32(img, target, k):
    """MSEGuide's gradient with the NaN rule of guided.py:262-265: (img - target) k, two roundings; any NaN zeroes everything.
    target: [B][row] or one row for all samples."""
    v = (f32(img) - f32(target)) * np.float32(k)
    return np.zeros_like(v) if np.isnan(v).any() else v


# ------------------------------------------------------------------------------------------------------------- timestep path
def freqs32(dim):
    """nn.py timestep_embedding's frequency table as the host uploads it: float32 exp(-ln(10000) i / half) evaluated in float64"""
    half = dim // 2
    return f32(np.exp(-math.log(10000.0) * np.arange(half) / half))


def timestep_embedding(t, dim, table=True):
    """-> ("bound", e64 [B][dim], bound).  With the uploaded table the argument is the float32 product t f_i (one rounding, restated
    here) and the float64 cos / sin of that same float32 argument is the reference: the bound is TRIG_ULPS units of the result.
    Without it (freqs = NULL) the device computes f_i = expf(-logf(10000) i / half): three roundings of the exponent q (|q| 3 v each
    on the frequency, relatively) and EXP_ULPS; that relative error times |t f_i|, plus the product's own rounding, is the
    argument's error and enters cos and sin one to one.  The reference is then cos / sin of the float64 product.  Odd dim: a zero
    last column, exact."""
    t = f32(t)
    half = dim // 2
    if table:
        arg = f64(t[:, None] * freqs32(dim)[None])
        d_arg = np.zeros_like(arg)
    else:
        q = math.log(10000.0) * np.arange(half) / half
        f = np.exp(-q)
        arg = f64(t)[:, None] * f[None]
        d_arg = np.abs(arg) * ((3 * V * q + EXP_ULPS * 2 * V)[None] + V)
    e = np.zeros((t.size, dim))
    e[:, :half], e[:, half:2 * half] = np.cos(arg), np.sin(arg)
    bound = np.zeros_like(e)
    bound[:, :half], bound[:, half:2 * half] = d_arg + TRIG_ULPS * ulp32(e[:, :half]), d_arg + TRIG_ULPS * ulp32(e[:, half:2 * half])
    return ("bound", e, bound)


def silu64(v):
    with np.errstate(over="ignore"):
        return v / (1 + np.exp(-v))


SILU_REL = (EXP_ULPS * 2 + 2) * V       # expf, the sum 1 + e, the quotient


def linear_rows(x, W, bias, act_in, act_out, mut=None):
    """y = act_out(W . act_in(x) + b), SiLU as v / (1 + exp(-v)) -> ("bound", y64, bound).  Rounding model: a SiLU's value carries
    SILU_REL relatively (expf at EXP_ULPS of a factor at most 1 in the quotient, the sum, the quotient) and TINY absolutely (its
    overflow side: expf(104) is infinite in float32 and the quotient a signed zero where the float64 value is 7e-44); the row
    product is an fma chain of ceil(K / 64) terms per lane, six additions across the wave and the bias: ceil(K / 64) + 7 roundings
    of the magnitudes' sum; the outer SiLU's slope is at most 1.1.
    mut: 'silu_side' (the SiLU of act_in applied to the product, that of act_out to x), 'drop8' (row 8 not computed: zeros)."""
    x, W = f64(f32(x)), f64(f32(W))
    B, K = x.shape
    b = np.zeros(W.shape[0]) if bias is None else f64(f32(bias))
    if mut == "silu_side":
        act_in, act_out = act_out, act_in
    s = silu64(x) if act_in else x
    d_s = np.abs(s) * SILU_REL + TINY if act_in else np.zeros_like(s)
    z = s @ W.T + b
    mag = np.abs(s) @ np.abs(W).T + np.abs(b)
    d_z = d_s @ np.abs(W).T + (math.ceil(K / 64) + 7) * V * mag if K else np.zeros_like(z)
    if act_out:
        y = silu64(z)
        d_y = 1.1 * d_z + np.abs(y) * SILU_REL + TINY
    else:
        y, d_y = z, d_z
    if mut == "drop8" and B > 8:
        y = y.copy()
        y[8] = 0
    return ("bound", y, d_y)


# ------------------------------------------------------------------------------------------------------------- secondary glue
TWO_PI32 = np.float32(2) * np.float32(math.pi)
HALF_PI32 = np.float32(math.pi / 2)


def sec_input(x, t, wemb, dtype):
    """[x | cos(2 pi t w_k) | sin(2 pi t w_k) | 13 zeros] per pixel, NHWC [B][HW][32] -> (exact part [B][HW][32] with NaN where the
    trigonometric channels are, ("bound", e64, bound) for all 32 channels).  The argument is the float32 chain ((2 pi) t) w_k (two
    roundings, restated); the float64 cos / sin of that float32 argument is the reference, TRIG_ULPS units allowed, then the store."""
    x, t, wemb = f32(x), f32(t), f32(wemb)
    B, _, HW = x.shape
    arg = f64((TWO_PI32 * t)[:, None] * wemb[None])
    ref = np.zeros((B, HW, 32))
    ref[:, :, :3] = f64(store(x, dtype)).transpose(0, 2, 1)
    ref[:, :, 3:11], ref[:, :, 11:19] = np.cos(arg)[:, None], np.sin(arg)[:, None]
    bound = np.zeros_like(ref)
    bound[:, :, 3:19] = TRIG_ULPS * ulp32(ref[:, :, 3:19]) + store_bound(ref[:, :, 3:19], dtype)
    exact = ref.astype(np.float32)
    exact[:, :, 3:19] = np.nan
    return exact, ("bound", ref, bound)


def sec_output(vn, x, t, dtype):
    """v (the first 3 of 32 NHWC channels, as stored in dtype), pred = x cos(a) - v sin(a), eps = x sin(a) + v cos(a), a = t pi / 2
    as one float32 product (restated) -> v32 [B][3][HW] exact, ("bound", pred64, .), ("bound", eps64, .): cos and sin at TRIG_ULPS,
    then two products and a sum (three roundings at most, fused or not)."""
    x, t = f32(x), f32(t)
    v = store(f32(vn), dtype)[:, :, :3].transpose(0, 2, 1)
    a = f64(t * HALF_PI32)[:, None, None]
    al, si = np.cos(a), np.sin(a)
    d_al, d_si = TRIG_ULPS * ulp32(al), TRIG_ULPS * ulp32(si)
    X, Vv = f64(x), f64(v)
    pred, eps = X * al - Vv * si, X * si + Vv * al
    bp = np.abs(X) * d_al + np.abs(Vv) * d_si + 3 * V * (np.abs(X * al) + np.abs(Vv * si)) + TINY
    be = np.abs(X) * d_si + np.abs(Vv) * d_al + 3 * V * (np.abs(X * si) + np.abs(Vv * al)) + TINY
    return f32(v), ("bound", pred, bp), ("bound", eps, be)


def avgpool2_32(src, dtype, mut=None):
    """src [B][H][W][C] (values as stored) -> [B][H/2][W/2][C]: (((0 + a00) + a01) + a10) + a11 in float32, times 0.25 (exact), stored"""
    s = store(src, dtype)
    acc = np.zeros_like(s[:, 0::2, 0::2])
    for dy in (0, 1):
        for dx in (0, 1):
            acc = acc + s[:, dy::2, dx::2]
    return store(acc * np.float32(0.5 if mut == "half" else 0.25), dtype)


def avgpool2_64(src):
    s = f64(src)
    return (s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]) / 4


def bil_src(o, n, mut=None):
    """F.interpolate(scale_factor=2, bilinear, align_corners=False): source = max((o + 0.5) / 2 - 0.5, 0) -> (i0, i1, frac); every
    step is exact in float32.  mut: 'offset' (-0.25 instead of -0.5), 'noclamp' (the upper neighbour not clamped: it wraps)."""
    s = max((o + 0.5) * 0.5 - (0.25 if mut == "offset" else 0.5), 0.0)
    i0 = int(s)
    i1 = (i0 + 1) % n if mut == "noclamp" else min(i0 + 1, n - 1)
    return i0, i1, np.float32(s - i0)


def up_matrix(n, mut=None):
    """the [2n][n] matrix of the one-dimensional map (float64; its entries are 0, 0.25, 0.75 and 1)"""
    M = np.zeros((2 * n, n))
    for o in range(2 * n):
        i0, i1, f = bil_src(o, n, mut)
        M[o, i0] += 1 - float(f)
        M[o, i1] += float(f)
    return M


def bilinear_up2_32(src, dtype, mut=None):
    """src [B][h][w][C] -> [B][2h][2w][C]: (1 - fy) ((1 - fx) a + fx b) + fy ((1 - fx) c + fx d), float32, every product and sum
    rounded once (the kernel switches contraction off), stored"""
    s = store(src, dtype)
    B, h, w, C = s.shape
    out = np.zeros((B, 2 * h, 2 * w, C), np.float32)
    one = np.float32(1)
    for oy in range(2 * h):
        y0, y1, fy = bil_src(oy, h, mut)
        for ox in range(2 * w):
            x0, x1, fx = bil_src(ox, w, mut)
            a, b, c, d = s[:, y0, x0], s[:, y0, x1], s[:, y1, x0], s[:, y1, x1]
            out[:, oy, ox] = (one - fy) * ((one - fx) * a + fx * b) + fy * ((one - fx) * c + fx * d)
    return store(out, dtype)


def bilinear_up2_64(src, mut=None):
    s = f64(src)
    return np.einsum("oy,px,byxc->bopc", up_matrix(s.shape[1], mut), up_matrix(s.shape[2], mut), s)


def bilinear_up2_adjoint32(gout, act, dtype, mut=None):
    """the adjoint, gathered per input pixel over the output rows 2y - 1 .. 2y + 2 and columns 2x - 1 .. 2x + 2 (ascending, clipped to
    the grid; a zero row or column weight is skipped): sum += (wy wx) g, each of the three operations rounded once; then zero where
    act is not above 0 (act None: no mask); stored.  mut: 'short_lo' / 'short_hi' (the window one short at that end)."""
    g = store(gout, dtype)
    B, H2, W2, C = g.shape
    h, w = H2 // 2, W2 // 2
    lo, hi = (0 if mut == "short_lo" else 1), (1 if mut == "short_hi" else 2)
    out = np.zeros((B, h, w, C), np.float32)
    for y in range(h):
        for x in range(w):
            v = np.zeros((B, C), np.float32)
            for oy in range(max(2 * y - lo, 0), min(2 * y + hi, 2 * h - 1) + 1):
                y0, y1, fy = bil_src(oy, h)
                wy = (np.float32(1) - fy if y0 == y else np.float32(0)) + (fy if y1 == y else np.float32(0))
                if wy == 0:
                    continue
                for ox in range(max(2 * x - lo, 0), min(2 * x + hi, 2 * w - 1) + 1):
                    x0, x1, fx = bil_src(ox, w)
                    wx = (np.float32(1) - fx if x0 == x else np.float32(0)) + (fx if x1 == x else np.float32(0))
                    if wx == 0:
                        continue
                    v = v + (wy * wx) * g[:, oy, ox]
            out[:, y, x] = v
    if act is not None:
        out = np.where(store(act, dtype) > 0, out, np.float32(0))
    return store(out, dtype)


def bilinear_up2_adjoint64(gout, act=None):
    """the explicit transposed matrix of the map applied to gout, with the ReLU mask"""
    g = f64(gout)
    out = np.einsum("oy,px,bopc->byxc", up_matrix(g.shape[1] // 2), up_matrix(g.shape[2] // 2), g)
    return out if act is None else np.where(f64(act) > 0, out, 0.0)


def adjoint_bound(gout, dtype):
    """the float32 gather against the transposed matrix: at most 16 terms, each with two roundings of its own and the sums after it"""
    g = np.abs(f64(gout))
    mag = np.einsum("oy,px,bopc->byxc", up_matrix(g.shape[1] // 2), up_matrix(g.shape[2] // 2), g)
    return 18 * V * mag + store_bound(mag, dtype)


def relu_mask32(g, act, dtype):
    """g where act > 0, else 0 (act = 0, -0, negative or NaN: zero)"""
    return np.where(store(act, dtype) > 0, store(g, dtype), np.float32(0))


def skip_grad32(gcat, act, gpool, dtype):
    """act > 0 ? gcat + 0.25 gpool[y / 2][x / 2] : 0; 0.25 gpool is exact, the sum rounds once (fused or not: the same number); stored"""
    gp = np.repeat(np.repeat(store(gpool, dtype), 2, axis=1), 2, axis=2)
    v = store(gcat, dtype) + np.float32(0.25) * gp
    return store(np.where(store(act, dtype) > 0, v, np.float32(0)), dtype)


def grad_to_nhwc(g, dtype):
    """planar f32 [B][3][HW] -> [B][HW][32] in dtype, channels 3.. zero"""
    B, _, HW = g.shape
    out = np.zeros((B, HW, 32), np.float32)
    out[:, :, :3] = store(g, dtype).transpose(0, 2, 1)
    return out


def grad_from_nhwc(g, dtype):
    """[B][HW][32] in dtype -> planar f32 [B][3][HW]"""
    return f32(store(g, dtype)[:, :, :3].transpose(0, 2, 1))


# the GPU file's glue cases: (B, H, W) of the FINE grid, C in pieces, pixel stride in elements beyond C
GLUE_GRIDS = ((1, 2, 2), (2, 2, 6), (1, 6, 2), (2, 4, 4))
GLUE_PIECES = (1, 3)
MASK_SPECIALS = (0.0, -0.0, -1.5, float("nan"))


def glue_case(B, H, W, pieces, dtype, wide, seed=0):
    """fine-grid tensors [B][H][W][stride] (the C used channels first, NaN in the gap), coarse ones dense [B][H/2][W/2][C]"""
    C = pieces * EPC[dtype]
    stride = C + (EPC[dtype] if wide else 0)
    s = 1000 * B + 100 * H + 10 * W + pieces + 5 * dtype + seed

    def dense(shape, seed_, specials=False):
        a = store(normal(shape, seed_), dtype)
        if specials:                                   # (every tensor has at least one piece: four elements)
            a.reshape(-1)[:len(MASK_SPECIALS)] = MASK_SPECIALS
        return a

    def strided(seed_, specials=False):
        a = np.full((B, H, W, stride), np.nan, np.float32)
        a[..., :C] = dense((B, H, W, C), seed_, specials)
        return a

    act_f, act_c = strided(s + 1, True), dense((B, H // 2, W // 2, C), s + 2, True)
    return dict(B=B, H=H, W=W, C=C, stride=stride, dtype=dtype, fine=strided(s), act_fine=act_f, act_coarse=act_c,
                coarse=store(normal((B, H // 2, W // 2, C), s + 3), dtype), gdense=store(normal((B, H, W, C), s + 4), dtype))
