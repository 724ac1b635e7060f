"""The float64 twin of the latent schedule and noise kernels (csrc/latent.hip, csrc/noise.hip), in plain numpy: for each of the 8 entry
points of latent.hip and the 5 of noise.hip a float64 result written from the formula in include/maua_hip.h, a float32 restatement
where the operation order is the contract (the uncontracted chains of blend_kernel, resample_linear_kernel and latent_merge_kernel,
scale_round_index's half-to-even, noise_combine), and the bound of the random family as a function of the operands.  The inputs of
tests/test_latent_host.py and tests/test_gpu_latent_kernels.py are generated here, so that what the host test proves about an input
is proved about the one the GPU test uploads.  The host test holds this file against torch, a dense spline solve and the oracle,
proves the preconditions of the exact families and shows that the comparisons reject off-by-one mutants (the `mutant=` arguments).

v = 2^-24 (half a unit in the last place of float32), u = 2^-53."""
import numpy as np

V = 2.0 ** -24
U = 2.0 ** -53
EPS32 = 1.1920928955078125e-07                          # torch.finfo(float32).eps, the Loop module's epsilon


def f32(a):
    return np.asarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def measured_dev(fn32, fn64, args, relative=False):
    """the project's convention for a device library function: the float32 CPU function against float64 over the case's own
    arguments; 4 x the largest deviation is what a bound may allow"""
    a32 = [f32(a) for a in args]
    with np.errstate(all="ignore"):
        got = f64(fn32(*a32))
        want = fn64(*[f64(a) for a in a32])
    ok = np.isfinite(want) & np.isfinite(got)
    err = np.abs(got - want)[ok]
    if relative:
        err = err[np.abs(want[ok]) > 0] / np.abs(want[ok])[np.abs(want[ok]) > 0]
    return float(err.max()) if err.size else 0.0


def products_exact(a, b):
    """a * b is a float32 number (so a contracted multiply-add rounds the same sum as a separate one)"""
    p = f64(a) * f64(b)
    return bool(np.array_equal(f64(f32(p)), p))


def is_f32(a):
    return bool(np.array_equal(f64(f32(a)), f64(a)))


# ----------------------------------------------------------------------------------------------------------------- the cases
TC_C = (1, 255, 256, 257, 513)                          # the edges of the 256-thread block
TC_T = (1, 2, 5)
BIG_T = 65537                                           # two rows more than one launch's gridDim.y holds: a second range of two rows
SLERP_D = (2, 255, 256, 257, 512)
NOISE_HW = (1, 3, 4, 5, 1020, 1023, 1024, 1025, 1028, 4100, 8193, 32 * 1024 + 4, 65537, 256 * 1024 + 4)
NOISE_SIGMA = (5.0, 0.5, 0.05)
BATCH_HW = (32 * 1024 + 4, 5, 65537, 4, 8193, 1024, 256 * 1024 + 4, 1023, 4100, 1)     # large, small, large ...: both paths, both caps
MIX_M = (1, 3, 257)
LDS_MAX = 16384                                         # floats of dynamic LDS a launch gets: the A of weighted_sum, the M of noise_mix


def normal(shape, seed):
    return f32(np.random.default_rng(seed).standard_normal(shape))


def envelope(T, seed):
    """[T] in [0, 1] with exact 0 and 1 among the values"""
    e = f32(np.random.default_rng(seed).uniform(0, 1, T))
    e[0] = 0.0
    e[-1] = 1.0 if T > 1 else e[-1]
    return e


# ----------------------------------------------------------------------------------------------------------------- blend
def blend64(a, b, env):
    """out[t] = a[t] (1 - env[t]) + b[t] env[t]; a, b [T][C] or [1][C] (a constant row)"""
    e = f64(env)[:, None]
    return f64(a) * (1 - e) + f64(b) * e


def blend32(a, b, env, mutant=None):
    """the kernel's chain, each operation rounded once: (a * (1 - e)) + (b * e)"""
    e = f32(env)[:, None]
    w0 = np.float32(1) - e
    if mutant == "swap":
        w0, e = e, w0
    if mutant == "row+1":
        e, w0 = np.roll(e, -1, 0), np.roll(w0, -1, 0)
    return (f32(a) * w0) + (f32(b) * e)


# ----------------------------------------------------------------------------------------------------------------- weighted_sum
def weighted_sum(env, lat, mutant=None):
    """out[t] = sum_a (env[t][a] / sum_a' env[t][a']) lat[a % n] and its bound for positive envelopes: the sequential sum s carries
    (A - 1) v, the division one more (A v on every weight); each term then takes its product and at most A - 1 additions (A v):
    (2 A + 1) v sum |w| |lat| to first order, the + 1 and the division by 1 - (2 A + 1) v covering the higher orders"""
    env, lat = f64(env), f64(lat)
    A, n = env.shape[1], lat.shape[0]
    sel = np.minimum(np.arange(A), n - 1) if mutant == "no_mod" else np.arange(A) % n
    with np.errstate(all="ignore"):
        w = env / env.sum(1, keepdims=True)
        out = w @ lat[sel]
        mag = np.abs(w) @ np.abs(lat[sel])
    k = (2 * A + 1) * V
    return out, k / (1 - k) * mag


def weighted_sum32(env, lat):
    """the kernel's order in float32: for the rows whose weights are infinite or NaN (a row of env summing to 0), where only that
    order decides between inf and NaN"""
    env, lat = f32(env), f32(lat)
    T, A = env.shape
    n = lat.shape[0]
    out = np.zeros((T, lat.shape[1]), np.float32)
    with np.errstate(all="ignore"):
        for t in range(T):
            s = np.float32(0)
            for a in range(A):
                s = s + env[t, a]
            for a in range(A):
                out[t] = out[t] + (env[t, a] / s) * lat[a % n]
    return out


# ----------------------------------------------------------------------------------------------------------------- index kernels
def scale_round_index(x, scale, mutant=None):
    """int64(round_half_even(x * scale)), the product rounded to float32 first"""
    p = f32(x) * np.float32(scale)
    if mutant == "half_away":
        return (np.sign(p) * np.floor(np.abs(f64(p)) + 0.5)).astype(np.int64)
    if mutant == "floor":
        return np.floor(f64(p)).astype(np.int64)
    return np.rint(p).astype(np.int64)


def round_input():
    """ties at .5 on both sides of zero, their float32 neighbours, and values whose product with the scale becomes a tie"""
    k = np.arange(-6, 7, dtype=np.float64)
    t = np.concatenate((k + 0.5, np.nextafter(f32(k + 0.5), np.float32(100)), np.nextafter(f32(k + 0.5), np.float32(-100)), k, 2 * k + 1,
                        [1e6 + 0.5, -1e6 - 0.5, 8388607.5, -8388607.5, 0.0, -0.0]))
    return f32(t)


def gather_rows(src, idx, mutant=None):
    """out[t] = src[idx[t]], a negative index counting from the end; indices in [-n_rows, n_rows)"""
    src, idx = np.asarray(src), np.asarray(idx, dtype=np.int64)
    n = src.shape[0]
    assert mutant or ((idx >= -n) & (idx < n)).all(), "an index outside the documented range"
    if mutant == "neg-1":
        r = np.where(idx < 0, idx + n - 1, idx)
    elif mutant == "lt-1":
        r = np.where(idx < -1, idx + n, idx) + (idx == -1)      # (-1 taken for a row of its own: the first)
    elif mutant == "row+1":
        r = (np.where(idx < 0, idx + n, idx) + 1) % n
    else:
        r = np.where(idx < 0, idx + n, idx)
    return src[r]


def gather_input(n_rows, T, seed):
    """every row, the two ends of the negative branch (-1 and -n_rows), 0 and n_rows - 1"""
    idx = np.random.default_rng(seed).integers(-n_rows, n_rows, size=T)
    fixed = [-1, -n_rows, 0, n_rows - 1]
    idx[:min(T, 4)] = fixed[:min(T, 4)]
    return idx.astype(np.int64)


# ----------------------------------------------------------------------------------------------------------------- resample
def resample_index32(n, size, mutant=None, contract=False):
    """(i0, i1, l0, l1, src) of F.interpolate(mode="linear", align_corners=False) in the kernel's float32 chain, every operation
    rounded once.  contract: scale (j + 0.5) - 0.5 as one fused multiply-add, which is what a build of torch that contracts computes
    (the host test matches torch's CPU kernel bit for bit with it; the library pins the uncontracted chain: contraction is switched off in that kernel)"""
    scale = np.float32(n) / np.float32(size)
    j = np.arange(size, dtype=np.float32)
    src = fma32(scale, j + np.float32(0.5), np.float32(-0.5)) if contract else (scale * (j + np.float32(0.5))) - np.float32(0.5)
    if mutant != "no_low_clamp":
        src = np.where(src < 0, np.float32(0), src)
    i0 = np.minimum(src.astype(np.int64), n - 1)
    if mutant == "no_low_clamp":
        i0 = np.maximum(i0, 0)
    i1 = i0 + (i0 < n - 1)
    if mutant == "clamp_end":
        i1 = i0 + (i0 < n - 2)
    if mutant == "i1+1":
        i1 = np.minimum(i0 + 2, n - 1)
    if mutant == "i0-1":
        i0 = np.maximum(i0 - 1, 0)
    l1 = src - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    return i0, i1, f32(l0), f32(l1), f32(src)


def resample_linear32(x, size, mutant=None, contract=False):
    x = f32(x)
    i0, i1, l0, l1, _ = resample_index32(x.shape[0], size, mutant, contract)
    if contract:
        return fma32(l0[:, None], x[i0], l1[:, None] * x[i1])
    return (l0[:, None] * x[i0]) + (l1[:, None] * x[i1])


def resample_linear64(x, size):
    """the same interpolation with the source position in exact arithmetic"""
    x = f64(x)
    n = x.shape[0]
    src = np.maximum((np.arange(size) + 0.5) * n / size - 0.5, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), n - 1)
    i1 = np.minimum(i0 + 1, n - 1)
    l1 = (src - i0)[:, None]
    return (1 - l1) * x[i0] + l1 * x[i1]


RESAMPLE = ((1, 1), (1, 5), (5, 1), (2, 5), (5, 2), (5, 5), (3, 9), (7, 21), (5, 13), (13, 5))    # (n, size); 3 -> 9 and 7 -> 21: src an ulp from an integer


# ----------------------------------------------------------------------------------------------------------------- spline
def spline_natural(tk, y, te, mutant=None):
    """the natural cubic spline through (tk, y [n][C]) at te, as the library computes it: second derivatives by the Thomas sweep of
    the interior tridiagonal system (M_0 = M_{n-1} = 0), the interval by searchsorted(right) - 1 clipped to [0, n - 2] (so the end
    cubics extrapolate), all in float64.  Returns (value, bound).

    Bound: v |value| for the rounding to float32, plus the float64 part.  The system is strictly diagonally dominant by rows,
    ||A^-1||_inf <= 1 / min_i (h_{i-1} + h_i) (Varah), and the sweep without pivoting is backward stable for it with |dA| <= 5 u |A|
    (Higham, Accuracy and Stability, 9.5); the right-hand side 6 ((y2 - y1) / h_i - (y1 - y0) / h_{i-1}) carries 5 u of the sum of its
    two magnitudes R.  So |dM| <= ||A^-1|| 5 u (max R + ||A||_inf max |M|) =: dm; the evaluation adds 12 u of the sum S of its terms'
    magnitudes and carries dm through (a^3 + b^3) / (6 h) + h (a + b) / 6 (with |a|, |b|)."""
    tk, y, te = f64(tk), f64(y), f64(te)
    n = tk.size
    h = np.diff(tk)
    M = np.zeros_like(y)
    if n > 2:
        cp, d = np.zeros(n), np.zeros_like(y)
        for i in range(1, n - 1):
            den = 2.0 * (h[i - 1] + h[i]) - h[i - 1] * cp[i - 1]
            cp[i] = h[i] / den if i < n - 2 else 0.0
            rhs = 6.0 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
            d[i] = (rhs - h[i - 1] * d[i - 1]) / den
        M[n - 2] = d[n - 2]
        for i in range(n - 3, 0, -1):
            M[i] = d[i] - cp[i] * M[i + 1]
    side = "left" if mutant == "left" else "right"
    idx = np.clip(np.searchsorted(tk, te, side=side) - 1, 0, n - 2)
    if mutant == "no_clip_hi":
        idx = np.clip(np.searchsorted(tk, te, side=side) - 1, 0, n - 1) % (n - 1)
    if mutant == "idx+1":
        idx = np.minimum(idx + 1, n - 2)
    hi = h[idx][:, None]
    a, b = (tk[idx + 1] - te)[:, None], (te - tk[idx])[:, None]
    m0, m1, y0, y1 = M[idx], M[idx + 1], y[idx], y[idx + 1]
    val = (m0 * a ** 3 + m1 * b ** 3) / (6 * hi) + (y0 / hi - m0 * hi / 6) * a + (y1 / hi - m1 * hi / 6) * b
    aa, ab = np.abs(a), np.abs(b)
    S = (np.abs(m0) * aa ** 3 + np.abs(m1) * ab ** 3) / (6 * hi) + (np.abs(y0) / hi + np.abs(m0) * hi / 6) * aa + (np.abs(y1) / hi + np.abs(m1) * hi / 6) * ab
    if n > 2:
        hs = h[:-1] + h[1:]
        R = 6 * (np.abs(np.diff(y, axis=0))[1:] / h[1:, None] + np.abs(np.diff(y, axis=0))[:-1] / h[:-1, None])
        dm = 5 * U / hs.min() * (R.max(0) + 3 * hs.max() * np.abs(M).max(0))[None, :]
    else:
        dm = np.zeros((1, y.shape[1]))
    bound = V * np.abs(val) + 12 * U * S + dm * ((aa ** 3 + ab ** 3) / (6 * hi) + hi * (aa + ab) / 6)
    return val, bound


def spline_dense(tk, y, te):
    """the same interpolant by a dense solve of the full n x n system (numpy.linalg.solve): independent of the sweep"""
    tk, y, te = f64(tk), f64(y), f64(te)
    n = tk.size
    h = np.diff(tk)
    A, rhs = np.zeros((n, n)), np.zeros_like(y)
    A[0, 0] = A[-1, -1] = 1.0
    for i in range(1, n - 1):
        A[i, i - 1:i + 2] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
        rhs[i] = 6 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
    M = np.linalg.solve(A, rhs)
    idx = np.clip(np.searchsorted(tk, te, side="right") - 1, 0, n - 2)
    hi, a, b = h[idx][:, None], (tk[idx + 1] - te)[:, None], (te - tk[idx])[:, None]
    return (M[idx] * a ** 3 + M[idx + 1] * b ** 3) / (6 * hi) + (y[idx] / hi - M[idx] * hi / 6) * a + (y[idx + 1] / hi - M[idx + 1] * hi / 6) * b


def spline_knots(n):
    """unequal spacing, every interval a power of two (so that data linear in t divides exactly)"""
    return np.concatenate(([0.0], np.cumsum([0.125, 0.25, 0.5, 0.125, 1.0, 0.25][:n - 1])))


def spline_eval_points(tk, T):
    """the knots themselves, a point before the first and one after the last (the end cubics extrapolate), dyadic points inside;
    then cut or cycled to T points"""
    inner = tk[0] + (tk[-1] - tk[0]) * np.array([0.0625, 0.3125, 0.5, 0.71875, 0.96875])
    pts = np.concatenate((tk, [tk[0] - 0.25, tk[-1] + 0.375], inner))
    return np.resize(pts, T)


def spline_linear_data(tk, C, seed):
    """y = alpha t + beta with small dyadic alpha, beta: every slope is the same exact number, so M = 0 and every product is exact"""
    rng = np.random.default_rng(seed)
    alpha, beta = rng.integers(-8, 9, size=C) / 4.0, rng.integers(-16, 17, size=C) / 8.0
    return f32(tk[:, None] * alpha[None, :] + beta[None, :]), alpha, beta


def loop_eval_points(size, n_loops):
    """spline_loop_latents: linspace(0, n_loops, size) % 1 - the last point wraps to 0"""
    return np.linspace(0.0, float(n_loops), size) % 1.0


# ----------------------------------------------------------------------------------------------------------------- slerp
def slerp_sums(D):
    """roundings of one of the kernel's fixed-order sums of D terms: ceil(D / 256) per thread (the product included), six shuffle
    levels, three additions of the four waves"""
    return -(-D // 256) + 6 + 3


def slerp(y, t, acos_dev=0.0, cos_dev=0.0, sin_dev=0.0, mutant=None):
    """y [n_seg + 1][L][D], t [k] -> (out [k][n_seg][L][D], bound, dot, p): between consecutive rows, a and b normalised, c the
    normalised part of b orthogonal to a, out = (a cos p + c sin p) normalised, p = t acos(a . b).

    Bound, first order, per element (k_s = slerp_sums(D), *_dev = 4 x the measured absolute deviation of the float32 function):
      a norm                    e_n = (k_s / 2 + 1) v relative (the sum, halved by the root, and the root)
      a unit element            e_u = e_n + v relative
      dot                       d_dot = 2 e_u + k_s v             (sum |a^ b^| <= 1)
      p                         d_p = |t| (d_dot / sqrt(1 - dot^2) + acos_dev) + v |p|
      c = b^ - dot a^           d_c = e_u |b^| + (d_dot + (e_u + v) |dot|) |a^| + v |c|, in the 2-norm D_c = e_u + d_dot + (e_u + v) |dot| + v s
      c^ = c / s, s = |c|       d_ch = d_c / s + |c^| (D_c / s + e_n + v), in the 2-norm D_ch = D_c / s + D_c / s + e_n + v
      cos p, sin p              d_p + cos_dev, d_p + sin_dev
      d = a^ cos p + c^ sin p   d_d = |a^| (e_u |cos p| + d_cos) + d_ch |sin p| + |c^| d_sin + 2 v (|a^ cos p| + |c^ sin p|)
      out = d / |d|, |d| = 1    d_d + |d| (D_d + e_n + v), D_d the same expression with the 2-norms (|a^|, |c^| -> 1)"""
    y, t = f64(y), f64(t)
    a, b = y[:-1], y[1:]
    ah = a / np.sqrt((a * a).sum(-1, keepdims=True))
    bh = b / np.sqrt((b * b).sum(-1, keepdims=True))
    D = y.shape[-1]
    with np.errstate(all="ignore"):
        dot = (ah * bh).sum(-1, keepdims=True)
        theta = np.arccos(np.minimum(dot, 1.0)) if mutant == "clip" else np.arccos(dot)
        c = bh - dot * ah
        s = np.sqrt((c * c).sum(-1, keepdims=True))
        ch = c / s
        tt = (1.0 - t if mutant == "1-t" else t)[:, None, None, None]
        p = tt * theta[None]
        cp, sp = np.cos(p), np.sin(p)
        d = ah[None] * cp + ch[None] * sp
        out = d / np.sqrt((d * d).sum(-1, keepdims=True))
        ks = slerp_sums(D)
        e_n = (ks / 2 + 1) * V
        e_u = e_n + V
        d_dot = 2 * e_u + ks * V
        d_p = np.abs(tt) * (d_dot / np.sqrt(1 - dot * dot) + acos_dev)[None] + V * np.abs(p)
        d_c = e_u * np.abs(bh) + (d_dot + (e_u + V) * np.abs(dot)) * np.abs(ah) + V * np.abs(c)
        D_c = e_u + d_dot + (e_u + V) * np.abs(dot) + V * s
        d_ch = d_c / s + np.abs(ch) * (D_c / s + e_n + V)
        D_ch = 2 * D_c / s + e_n + V
        d_cos, d_sin = d_p + cos_dev, d_p + sin_dev
        d_d = np.abs(ah)[None] * (e_u * np.abs(cp) + d_cos) + d_ch[None] * np.abs(sp) + np.abs(ch)[None] * d_sin + \
            2 * V * (np.abs(ah[None] * cp) + np.abs(ch[None] * sp))
        D_d = (e_u * np.abs(cp) + d_cos) + D_ch[None] * np.abs(sp) + d_sin + 4 * V
        bound = d_d + np.abs(out) * (D_d + e_n + V)
    return out, bound, dot, p


def slerp_input(n_seg, L, D, seed):
    """rows of different lengths (the normalisation matters), consecutive rows between 20 and 160 degrees apart"""
    rng = np.random.default_rng(seed)
    while True:
        y = rng.standard_normal((n_seg + 1, L, D)) * rng.uniform(0.5, 4.0, size=(n_seg + 1, L, 1))
        y = f32(y)
        dot = slerp(y, np.zeros(1))[2]
        if (np.abs(dot) < 0.94).all():
            return y


# ----------------------------------------------------------------------------------------------------------------- latent_merge
def latent_merge32(lat, seq, mod, mode, l0, l1, mutant=None):
    """lat, seq [T][L][D]; layers [l0, l1) of a copy of lat: (lat + seq) / 2, lat (1 - m) + m seq in the kernel's order, or seq"""
    out = f32(lat).copy()
    if l1 <= l0:
        return out
    if mutant == "l0+1":
        l0 += 1
    if mutant == "l1+1":
        l1 = min(l1 + 1, out.shape[1])
    a, s = out[:, l0:l1], f32(seq)[:, l0:l1]
    if mode == 0:
        out[:, l0:l1] = (a + s) / np.float32(2)
    elif mode == 1:
        m = f32(mod)[:, None, None]
        if mutant == "swap":
            m = np.float32(1) - m
        out[:, l0:l1] = (a * (np.float32(1) - m)) + (m * s)
    else:
        out[:, l0:l1] = s
    return out


def latent_merge64(lat, seq, mod, mode, l0, l1):
    out = f64(lat).copy()
    a, s = out[:, l0:l1], f64(seq)[:, l0:l1]
    m = f64(mod)[:, None, None] if mod is not None else None
    out[:, l0:l1] = (a + s) / 2 if mode == 0 else a * (1 - m) + m * s if mode == 1 else s
    return out


# ----------------------------------------------------------------------------------------------------------------- noise: Loop
def fma32(a, b, c):
    """fmaf on float32 operands: the product is exact in float64, the sum is rounded to float64 and then to float32 (a double
    rounding that moves a result by one ulp in about one case in 2^29: of no weight against a 4 x allowance)"""
    return f32(f64(f32(a)) * f64(f32(b)) + f64(f32(c)))


def _reduce_pio2(x):
    x = f32(x)
    k = np.rint(x * np.float32(0.63661977236758134))
    r = fma32(-k, np.float32(1.5707963705062866), x)
    r = fma32(-k, np.float32(-4.3711388286737929e-08), r)
    return r, k.astype(np.int64)


def _poly_sin(r):
    z = r * r
    return fma32(r * z, fma32(fma32(np.float32(-1.9515295891e-4), z, np.float32(8.3321608736e-3)), z, np.float32(-1.6666654611e-1)), r)


def _poly_cos(r):
    z = r * r
    return fma32(z * z, fma32(fma32(np.float32(2.443315711809948e-5), z, np.float32(-1.388731625493765e-3)), z, np.float32(4.166664568298827e-2)),
                 fma32(np.float32(-0.5), z, np.float32(1.0)))


def fast_sin32(x):
    """noise.hip's fast_sin restated operation by operation (what the kernels' sine is, on the CPU)"""
    r, q = _reduce_pio2(x)
    v = np.where(q & 1, _poly_cos(r), _poly_sin(r))
    return f32(np.where(q & 2, -v, v))


def fast_cos32(x):
    r, q = _reduce_pio2(x)
    v = np.where(q & 1, _poly_sin(r), _poly_cos(r))
    return f32(np.where((q + 1) & 2, -v, v))


def noise_path(hw):
    """(16-byte path?, elements per block sweep, blocks per frame before the cap, blocks of every pass: capped at 256)"""
    vec = hw % 4 == 0
    per = 1024 if vec else 256
    blocks = -(-hw // per)
    return vec, per, blocks, min(256, blocks)


def tree_roundings(hw, nblk):
    """roundings on the way of one square into the sum of hw squares over nblk blocks: its product, the thread's sequential sum
    (ceil(hw / (256 nblk)) terms, in fours on the 16-byte path), six shuffle levels, four waves, then the nblk partial sums in order"""
    per_thread = 4 * -(-(hw // 4) // (nblk * 256)) if hw % 4 == 0 else -(-hw // (nblk * 256))
    return 1 + per_thread + 6 + 4 + nblk


def loop_values(planes, idv, sigma, cos_dev=0.0, sin_dev=0.0, mutant=None):
    """planes [3][hw], idv [B] (the float32 idx values of the frames), sigma (a float32 number) -> (val [B][hw], bound):
    val = sin(cos(idx + n0) / (sigma / 50) + n1) n2.  Per element, *_dev = 4 x the measured absolute deviation of the float32 function:
      x0 = idx + n0           v |x0|
      c = cos x0              d_c = v |x0| + cos_dev
      f = c * float32(50 / sigma)     d_f = d_c |50 / sigma| + 2 v |f|   (the constant's rounding and the product's)
      x1 = f + n1             d_1 = d_f + v |x1|
      s = sin x1              d_s = d_1 + sin_dev
      val = s n2              d_s |n2| + v |val|"""
    n0, n1, n2 = f64(planes)
    if mutant == "planes":
        n1, n2 = n2, n1
    idv = f64(idv)[:, None]
    inv = 50.0 / float(np.float32(sigma))
    x0 = idv + n0[None]
    c = np.cos(x0)
    f = c * inv
    x1 = f + n1[None]
    s = np.sin(x1)
    val = s * n2[None]
    d_c = V * np.abs(x0) + cos_dev
    d_f = d_c * abs(inv) + 2 * V * np.abs(f)
    d_1 = d_f + V * np.abs(x1)
    d_s = d_1 + sin_dev
    return val, d_s * np.abs(n2)[None] + V * np.abs(val), x0, x1


def loop_normalised(val, dval, nblk):
    """(out, bound, scale, relative bound of the scale): out = val / (sqrt(mean val^2) + eps).  The sum of squares tot carries
    sum 2 |val| d_val from its terms and tree_roundings v of itself; rms = sqrt(tot / hw) half of that relative plus 2 v (division,
    root); + eps one more v; the reciprocal one more; out = val * scale: d_val scale + |out| (scale's relative bound + v)"""
    hw = val.shape[1]
    tot = (val * val).sum(1)
    d_tot = (2 * np.abs(val) * dval).sum(1) + tree_roundings(hw, nblk) * V * tot
    rms = np.sqrt(tot / hw)
    with np.errstate(all="ignore"):
        d_rms = np.where(tot > 0, d_tot / np.maximum(tot, 1e-300) / 2, 0.0) * rms + 2 * V * rms
    den = rms + EPS32
    scale = 1.0 / den
    rel = d_rms / den + 2 * V
    out = val * scale[:, None]
    return out, dval * scale[:, None] + np.abs(out) * (rel[:, None] + V), scale, rel


def loop_idx(T, n_loops=2.0):
    return f32(np.linspace(0.0, 2.0 * np.pi * n_loops, T))


# ----------------------------------------------------------------------------------------------------------------- noise: mix, combine
def noise_mix(noise, noise2, mod):
    """noise, noise2 [M][hw], mod [B][M] -> (out [B][hw], bound): sum_m noise[m] mod[b][m] (+ sum_m noise2[m] w2[b][m], w2 the float32
    1 - mod).  Every term takes its product and at most M - 1 additions, with two banks one more for l + r: (M + 1) v sum |terms|"""
    noise, mod = f64(noise), f64(mod)
    M = mod.shape[1]
    out, mag = mod @ noise, np.abs(mod) @ np.abs(noise)
    if noise2 is not None:
        w2 = f64(np.float32(1) - f32(mod))
        out, mag = out + w2 @ f64(noise2), mag + np.abs(w2) @ np.abs(f64(noise2))
    return out, (M + 1) * V * mag


def mix_exact_input(M, hw, B, seed):
    """integer planes, modulators in {0, 1/4, 1/2, 3/4, 1}: every product and every partial sum is a float32 number"""
    rng = np.random.default_rng(seed)
    lim = max(1, min(8, (1 << 20) // (8 * M)))
    return (f32(rng.integers(-lim, lim + 1, size=(M, hw))), f32(rng.integers(-lim, lim + 1, size=(M, hw))),
            f32(rng.integers(0, 5, size=(B, M)) / 4.0))


def noise_combine32(x, y, mod, mode, scale, bias, mutant=None):
    """x, y [B][hw]: (x + y) / 2; x m + y (1 - m); scale x + bias, each operation rounded once.  The device may contract a product
    into the following sum: the exact family uses operands whose products are float32 numbers (combine_exact_input)"""
    x = f32(x)
    if mode == 0:
        return (x + f32(y)) / np.float32(2)
    if mode == 1:
        m = f32(mod)[:, None]
        if mutant == "swap":
            m = np.float32(1) - m
        if mutant == "row+1":
            m = np.roll(m, -1, 0)
        return (x * m) + (f32(y) * (np.float32(1) - m))
    return (np.float32(scale) * x) + np.float32(bias)


def combine_exact_input(B, hw, seed):
    """x, y integers below 2^12, mod in {0, 1/4, 1/2, 1}; scale 0.75, bias -2.5"""
    rng = np.random.default_rng(seed)
    x, y = f32(rng.integers(-4000, 4001, size=(B, hw))), f32(rng.integers(-4000, 4001, size=(B, hw)))
    mod = f32(rng.choice([0.0, 0.25, 0.5, 1.0], size=B))
    return x, y, mod, 0.75, -2.5
