"""Float64 twins of the image-space kernels (csrc/resize.hip, csrc/cutouts.hip, csrc/colormatch.hip, csrc/image_ops.hip: sixteen entry
points), each with a bound derived from the operation's own terms, and float32 restatements (numpy float32 arrays: one rounding per
operation) of the families whose order is the contract with the reference: perlin, restitch, the colour-match pixel chain with its
2^-40 fixed-point sums and the normalisation's sum, the cutouts' tap tables.  A plain module: it holds no test and no fixture.
tests/test_image_kernels_host.py holds it against torch, tests/image_pipeline_ref.py, the oracle, maua_amd/image.py and g33 / g34 / g37;
tests/test_gpu_image_kernels.py holds the kernels against it.  The GPU tests' shapes live here, so that the host tests show the
mutants rejected at exactly those.

u = 2^-24 (half a unit in the last place of a float32 number near 1).  The rules every bound below is put together from:
    a chain of n multiply-adds, fused or not          n u sum |w_i s_i|   (each product rounds at most once, each partial sum once and
                                                                          is at most the sum of magnitudes; first order in u)
    a two-pass separable filter                       the product form: the second pass carries the first pass's error through its own
                                                      |weights| and adds its own chain on the first pass's magnitudes
    one more rounded operation on a value r           u |r|
    a store to bf16 / f16                             half a unit in the last place of the output type at the value's own binade
                                                      (half_ulp; f16 at normal magnitudes: the tests stay there)
Every discrete decision (floor of a source coordinate, byte truncation, padding index) is taken in the float32 restatement and
the float64 value is evaluated at the same choice.  `mutant=` arguments switch one off-by-one error on: the host tests show that the
GPU file's comparisons reject each of them at the GPU file's own shapes."""
import ctypes
import ctypes.util

import numpy as np

U = 2.0 ** -24
F = np.float32
SIG_BITS = {"f32": 24, "bf16": 8, "f16": 11}


def half_ulp(v, dt):
    """half a unit in the last place of the type at magnitude |v| (normal numbers): 2^(floor(log2 |v|) - bits)"""
    a = np.maximum(np.abs(v), 1e-30)
    return np.ldexp(1.0, np.floor(np.log2(a)).astype(np.int64) - SIG_BITS[dt])

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fmaf.restype = ctypes.c_float
_libm.fmaf.argtypes = [ctypes.c_float] * 3


def fmaf(a, b, c):
    """libm's exact fused multiply-add on float32 numbers (this Python has no math.fma)"""
    return F(_libm.fmaf(float(a), float(b), float(c)))


def rng(seed):
    return np.random.default_rng(seed)


def normal(shape, seed):
    return rng(seed).standard_normal(shape).astype(F)


def uniform(shape, seed, lo=-1.0, hi=1.0):
    return (rng(seed).random(shape) * (hi - lo) + lo).astype(F)


def d(x):
    return np.asarray(x, dtype=np.float64)


# ============================================================================================================ maua_image_resize
def resize_axis64(x, left, w, mutant=None):
    """one pass along the LAST axis: out[..., o] = sum_j w[o, j] x[..., left[o] + j] over the taps inside the image (zero padding);
    -> (value, sum of |w x|) in float64"""
    x = d(x)
    n = x.shape[-1]
    idx = np.asarray(left, dtype=np.int64)[:, None] + np.arange(w.shape[1])[None, :]
    if mutant == "tap+1":
        idx = idx + 1
    if mutant == "tap-1":
        idx = idx - 1
    ok = (idx >= 0) & (idx < (n + 1 if mutant == "clamp_n" else n))
    g = x[..., np.clip(idx, 0, n - 1)] * (d(w) * ok)
    return g.sum(-1), np.abs(g).sum(-1)


def image_resize(src, Ho, Wo, left_y, w_y, left_x, w_x, prior=None, add=0.0, mutant=None):
    """src [planes, H, W] -> (out [planes, Ho, Wo] float64, bound).  Rows first (the kernel's vertical pass into LDS), then columns.
    Bound: the vertical chain of ty multiply-adds leaves at most ty u A with A = sum |w_y| |src|; the horizontal chain of tx carries
    that through |w_x| and adds tx u sum |w_x| |vertical| <= tx u sum |w_x| A: (ty + tx) u sum |w_x| A (a kept axis has no chain: 0 for
    it).  Then `resized + add` (one rounding) or `(dst + resized) + add` (two), each at most u times the magnitudes added."""
    src = d(src)
    ty = tx = 0
    v, A = src, np.abs(src)
    if left_y is not None:
        ty = w_y.shape[1]
        v, A = (np.moveaxis(t, -1, -2) for t in resize_axis64(np.moveaxis(src, -2, -1), left_y, w_y, mutant))
    out, mag = v, A
    if left_x is not None:
        tx = w_x.shape[1]
        out, _ = resize_axis64(v, left_x, w_x, mutant)
        _, mag = resize_axis64(A, left_x, np.abs(d(w_x)), mutant)
    bound = (ty + tx) * U * mag
    if prior is not None:
        bound = bound + U * (np.abs(d(prior)) + np.abs(out)) + U * (np.abs(d(prior)) + np.abs(out) + abs(add))
        out = d(prior) + out + add
    else:
        bound = bound + U * (np.abs(out) + abs(add))
        out = out + add
    assert out.shape[-2:] == (Ho, Wo)
    return out, bound


# ============================================================================================================ destitch / restitch
def destitch(img, T, ys, xs, mutant=None):
    """img [B, 3, H, W] -> [n_tiles * B, 3, T, T], tile-major (rows, then columns), then batch: exact"""
    order = [(y, x) for x in xs for y in ys] if mutant == "columns_first" else [(y, x) for y in ys for x in xs]
    return np.concatenate([img[..., y:y + T, x:x + T] for y, x in order], 0)


def restitch32(tiles, T, ys, xs, wy, wx, H, W, mutant=None):
    """tiles [n_tiles, 3, T, T], wy [n_rows, T], wx [n_cols, T] float32 -> (out [3, H, W], acc, norm) float32, in the reference's order
    (ops/image.py:54-62): per tile weight = wy * wx (rounded), acc += tile * weight (product rounded, sum rounded), norm += weight; tiles
    visited rows first; one division.  A pixel sees its covering tiles in that order, which is the kernel's loop."""
    tiles, wy, wx = np.asarray(tiles, F), np.asarray(wy, F), np.asarray(wx, F)
    acc, norm = np.zeros((3, H, W), F), np.zeros((1, H, W), F)
    visits = [(r, c) for r in range(len(ys)) for c in range(len(xs))]
    if mutant == "columns_first":
        visits = [(r, c) for c in range(len(xs)) for r in range(len(ys))]
    for r, c in visits:
        y, x = ys[r], xs[c]
        weight = wy[r][:, None] * wx[c][None, :]
        acc[:, y:y + T, x:x + T] += tiles[r * len(xs) + c] * weight[None]
        norm[:, y:y + T, x:x + T] += weight[None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return acc / norm, acc, norm


# ============================================================================================================ sharpen
K1, K5 = F(1.0) / F(13.0), F(5.0) / F(13.0)        # the float32 kernel of adjust_sharpness: ones, centre 5, divided by its sum


def sharpen(img, strength, mutant=None):
    """img [planes, H, W] float32 -> (out float64, bound): maua/ops/image.py:70-71 on torchvision's adjust_sharpness.
    v = (p + 1) / 2: one rounding, ev = u |v| (the halving is exact).  H <= 2 or W <= 2: out = 2 v - 1, 2 ev + u |out|.
    blur (interior): nine multiply-adds on rounded v: eb = sum k ev + 9 u sum k |v|; the border keeps v (eb = ev).
    r = s v + (1 - s) blur: |s| (ev + u |v|) [product] + |1 - s| (eb + 2 u |blur|) [1 - s rounds, product] + u (|s v| + |(1 - s) blur|)
    [the sum, bounded by its terms so that a fused form is covered]; the clamp does not expand; out = 2 r - 1: 2 er + u |out|."""
    p = d(img)
    s = float(F(strength))
    v = (p + 1.0) / 2.0
    ev = U * np.abs(v)
    H, W = p.shape[-2:]
    if H <= 2 or W <= 2:
        out = 2.0 * v - 1.0
        return out, 2.0 * ev + U * np.abs(out)
    blur, eb, absb = v.copy(), ev.copy(), np.abs(v)
    k = np.full((3, 3), float(K1))
    k[1, 1] = float(K5)
    acc, eacc, mag = (np.zeros_like(v[..., 1:-1, 1:-1]) for _ in range(3))
    for dy in range(3):
        for dx in range(3):
            sy, sx = (dy, dx) if mutant != "tap+1" else (dy, min(dx + 1, 2))
            win = (Ellipsis, slice(sy, sy + H - 2), slice(sx, sx + W - 2))
            acc += k[dy, dx] * v[win]
            eacc += k[dy, dx] * ev[win]
            mag += k[dy, dx] * np.abs(v[win])
    blur[..., 1:-1, 1:-1], eb[..., 1:-1, 1:-1], absb[..., 1:-1, 1:-1] = acc, eacc + 9 * U * mag, mag
    r = s * v + (1.0 - s) * blur
    er = abs(s) * (ev + U * np.abs(v)) + abs(1.0 - s) * (eb + 2 * U * absb) + U * (abs(s) * np.abs(v) + abs(1.0 - s) * absb)
    r = np.clip(r, 0.0, 1.0)
    out = 2.0 * r - 1.0
    return out, 2.0 * er + U * np.abs(out)


# ============================================================================================================ moments / match_apply
HM_SLICE, HM_REC = 4096, 11


def moments_slices(HW):
    return (HW + HM_SLICE - 1) // HM_SLICE


def _tree(vals):
    """vals [.., 4096] (zero past the slice's end) summed as the kernel does: thread t adds pixels t, t + 256, ... in order, then the
    fixed halving tree over the 256 threads.  -> (sum, sum of |every intermediate value|): each addition rounds once, so the error of
    the whole sum is at most u times the second number (a running error bound: exact to first order, no depth constant)."""
    per = vals.reshape(*vals.shape[:-1], HM_SLICE // 256, 256)
    run = np.cumsum(per, axis=-2)
    mags = np.abs(run).sum(-2)
    cur = run[..., -1, :]
    o = 128
    while o:
        cur = cur[..., :o] + cur[..., o:2 * o]
        mags = mags[..., :o] + mags[..., o:2 * o] + np.abs(cur)
        o >>= 1
    return cur[..., 0], mags[..., 0]


def moments(img, navg, noise=None, noise_scale=0.0):
    """img [frames * navg, 3, HW] (noise [frames, 3, HW]) -> (partial [frames, slices, 11] float64, bound; columns 9 / 10, min / max over
    the raw images, are exact: bound 0).
    Value of a pixel: v = (x_1 + ... + x_navg) / navg + ns * noise.  Its error ev: the navg - 1 sequential additions, u each on at most
    sum |x| (navg > 1), the division u |mean|, the noise product and the addition 2 u |ns noise| + u |v| (covers a fused form).
    Sums: u (the tree's intermediates) + the tree of ev.  Products: each multiply-add rounds once on the running sum (the tree bound on
    the exact products) and carries ev |v'| + ev' |v| in."""
    x = d(img)
    frames = x.shape[0] // navg
    HW = x.shape[-1]
    x = x.reshape(frames, navg, 3, HW)
    mean = x.sum(1) / navg
    ev = ((navg - 1) * U * np.abs(x).sum(1) / navg + U * np.abs(mean)) if navg > 1 else np.zeros_like(mean)
    v = mean
    if noise is not None:
        nn = float(F(noise_scale)) * d(noise).reshape(frames, 3, HW)
        v = mean + nn
        ev = ev + 2 * U * np.abs(nn) + U * np.abs(v)
    S = moments_slices(HW)
    pad = S * HM_SLICE - HW

    def sl(a):
        return np.pad(a, [(0, 0)] * (a.ndim - 1) + [(0, pad)]).reshape(*a.shape[:-1], S, HM_SLICE)
    part, bound = np.zeros((frames, S, HM_REC)), np.zeros((frames, S, HM_REC))
    for c in range(3):
        s, m = _tree(sl(v[:, c]))
        part[:, :, c], bound[:, :, c] = s, U * m + _tree(sl(ev[:, c]))[0]
    for k, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        s, m = _tree(sl(v[:, a] * v[:, b]))
        carried = _tree(sl(ev[:, a] * np.abs(v[:, b]) + ev[:, b] * np.abs(v[:, a])))[0]
        part[:, :, 3 + k], bound[:, :, 3 + k] = s, U * (m + _tree(sl(np.abs(v[:, a] * v[:, b])))[0]) + carried
    raw = sl(x.reshape(frames, navg * 3, HW))
    live = sl(np.ones((1, 1, HW), bool))
    part[:, :, 9] = np.where(live, raw, np.inf).min((1, 3))
    part[:, :, 10] = np.where(live, raw, -np.inf).max((1, 3))
    return part, bound


def match_apply(img, noise, noise_scale, m, mu_t, mu_s, scale, prior, clamp, lo, hi, mutant=None):
    """one frame [3, HW]: out = clamp(prior + scale (m (img + ns noise - mu_t) + mu_s)) -> (out float64, bound).
    v: 2 u |ns noise| + u |img + ns noise| (product and sum, fused or not) + u |v| (the subtraction); r: three multiply-adds 3 u sum |m v|
    + sum |m| ev, + u |r| (mu_s); times scale: u |scale r|; the accumulation u |sum|; the clamp does not expand."""
    x, m = d(img), d(np.asarray(m, F)).reshape(3, 3)
    mu_t, mu_s, scale = d(np.asarray(mu_t, F)), d(np.asarray(mu_s, F)), float(F(scale))
    v, ev = x, np.zeros_like(x)
    if noise is not None:
        nn = float(F(noise_scale)) * d(noise)
        v = x + nn
        ev = 2 * U * np.abs(nn) + U * np.abs(v)
    v = v - mu_t[:, None]
    ev = ev + U * np.abs(v)
    if mutant == "transposed":
        m = m.T
    r = m @ v + mu_s[:, None]
    er = 3 * U * (np.abs(m) @ np.abs(v)) + np.abs(m) @ ev + U * np.abs(r)
    r, er = r * scale, abs(scale) * er + U * np.abs(r * scale)
    if prior is not None:
        r = r + d(prior)
        er = er + U * np.abs(r)
    if clamp:
        r = np.clip(r, float(F(lo)), float(F(hi)))
    return r, er


# ============================================================================================================ perlin
def perlin_interp32(t):
    t2 = t * t
    t3 = t2 * t
    return F(3.0) * t2 - F(2.0) * t3


def perlin_at32(g, scale, mutant=None):
    """ops/noise.py:94-106 for one octave, g [2, w + 1, h + 1] float32 -> [w * scale, h * scale] float32, every operation rounded on its
    own in the reference's order ((wx * wy) * (gx * xs + gy * ys), the four corners added to 0 in turn).  Precondition (asserted): scale
    is a power of two, so a / scale is exact and equals torch.linspace(0, 1, scale + 1)[:-1]."""
    assert scale >= 1 and scale & (scale - 1) == 0
    g = np.asarray(g, F)
    gx, gy = g[0], g[1]
    w, h = gx.shape[0] - 1, gx.shape[1] - 1
    R, Cc = np.arange(w * scale), np.arange(h * scale)
    i, j = (R // scale)[:, None], (Cc // scale)[None, :]
    xs = ((R % scale).astype(F) / F(scale))[:, None]
    ys = ((Cc % scale).astype(F) / F(scale))[None, :]
    one = F(1.0)
    wx, wy = one - perlin_interp32(xs), one - perlin_interp32(ys)
    x1, y1, wx1, wy1 = one - xs, one - ys, one - wx, one - wy
    i1, j1 = (i + 1, j + 1) if mutant != "corner" else (i, j + 1)
    dots = np.zeros((w * scale, h * scale), F)
    dots = dots + (wx * wy) * (gx[i, j] * xs + gy[i, j] * ys)
    dots = dots + (wx1 * wy) * (-gx[i1, j] * x1 + gy[i1, j] * ys)
    dots = dots + (wx * wy1) * (gx[i, j1] * xs - gy[i, j1] * y1)
    dots = dots + (wx1 * wy1) * (-gx[i1, j1] * x1 - gy[i1, j1] * y1)
    assert dots.dtype == F
    return dots


def perlin32(grads, octaves, width, height, grayscale, mutant=None):
    """create_perlin_noise (ops/noise.py:109-132) -> dict(raw [ch, S_r, S_c] float32, q uint8 [ch, ..], lut int [ch, 256], out [3, ..]
    float32): the octave sum from 0.5 (`out += p * oct`, the product rounded, then the sum), clamp, mul(255).byte() (truncation),
    ImageOps.autocontrast's table (cutoff 0, double arithmetic: int(i * scale + offset) clipped; the identity when hi <= lo) and
    to_tensor (byte / 255 in float32).  grads: channel-major list of [2, w + 1, h + 1], w / h doubling per octave."""
    n, ch = len(octaves), (1 if grayscale else 3)
    raw = []
    for c in range(ch):
        v = np.full((width << n, height << n), 0.5, F)
        scale = 1 << n
        for k in range(n):
            v = v + perlin_at32(grads[c * n + k], scale, mutant) * F(octaves[k])
            scale >>= 1
        raw.append(v)
    raw = np.stack(raw)
    q = (np.clip(raw, F(0), F(1)) * F(255.0)).astype(np.int32).astype(np.uint8)       # the product is < 256 and >= 0: truncation
    luts, planes = [], []
    for c in range(ch):
        lo, hi = int(q[c].min()), int(q[c].max())
        lut = list(range(256))
        if hi > lo:
            scale = 255.0 / (hi - lo)
            offset = -lo * scale
            lut = [min(max(int(ix * scale + offset), 0), 255) for ix in range(256)]
        luts.append(lut)
        planes.append(np.asarray(lut, F)[q[c]] / F(255.0))
    out = np.stack(planes if ch == 3 else planes * 3)
    return dict(raw=raw, q=q, lut=np.asarray(luts), out=out)


def perlin_offsets(grads):
    offs, pos = [], 0
    for g in grads:
        offs.append(pos)
        pos += g.size
    return offs


# ============================================================================================================ grad_accumulate
def grad_accumulate32(sub, acc, first):
    """guided.py:258-266: acc = (first ? 0 : acc) + (sub holds a NaN ? 0 : sub), float32, exact (inf is not a NaN and passes)"""
    sub, acc = np.asarray(sub, F), np.asarray(acc, F)
    v = np.zeros_like(sub) if np.isnan(sub).any() else sub
    with np.errstate(invalid="ignore"):
        return v.copy() if first else acc + v


# ============================================================================================================ resize2d, mode 1 (F.pad)
PAD_CIRCULAR, PAD_REFLECT, PAD_REPLICATE, PAD_CONSTANT = 0, 1, 2, 3      # enum maua_pad_mode


def pad_src(p, n, how, mutant=None):
    """source index of padded position p (array) for F.pad's modes; -1 where the constant goes"""
    p = np.asarray(p, dtype=np.int64)
    inside = (p >= 0) & (p < n)
    if how == PAD_REFLECT:
        if n == 1:
            q = np.zeros_like(p)
        else:
            period = 2 * n if mutant == "period_2n" else 2 * (n - 1)
            q = np.mod(p, period)
            q = np.where(q < n, q, period - q)
            q = np.clip(q, 0, n - 1) if mutant == "period_2n" else q
    elif how == PAD_REPLICATE:
        q = np.clip(p, 0, n - 1)
    elif how == PAD_CIRCULAR:
        q = np.mod(p, n)
    else:
        q = np.full_like(p, -1)
    return np.where(inside, p, q)


def pad2d(x, oh, ow, pl, pt, how, value, mutant=None):
    """x [N, C, H, W] (any dtype) -> [N, C, oh, ow]: output (oy, ox) <- input (oy - pt, ox - pl); negative offsets crop.  Exact: a copy,
    and `value` converted to the array's type"""
    H, W = x.shape[-2:]
    sy, sx = pad_src(np.arange(oh) - pt, H, how, mutant), pad_src(np.arange(ow) - pl, W, how, mutant)
    out = x[..., np.clip(sy, 0, H - 1)[:, None], np.clip(sx, 0, W - 1)[None, :]].copy()
    out[..., (sy[:, None] < 0) | (sx[None, :] < 0)] = value
    return out


# ============================================================================================================ the GPU tests' shapes
# (here, so that tests/test_image_kernels_host.py shows the mutants rejected at exactly these)
IMAGE_RESIZE_CASES = [(5, 7, 11, 13), (37, 53, 9, 53), (37, 53, 37, 20), (3, 1025, 2, 700), (2, 16384, 3, 5), (6, 7, 17, 9)]


GRIDS = [  # H, W, T, ys, xs
    (5, 5, 5, [0], [0]),                                    # 1 x 1
    (5, 13, 5, [0], [0, 4, 8]),                             # 1 x 3
    (11, 10, 5, [0, 3, 6], [0, 5]),                         # 3 x 2
    (11, 13, 5, [0, 1, 2, 3, 4, 5, 6], [0, 5, 8]),          # rows overlapping by T - 1; columns 0 and 5 abut
    (11, 13, 5, [0, 5, 6], [0, 4, 8]),                      # rows 0 and 5 abut
    (3, 66, 3, [0], list(range(64))),                       # 64 tile columns of a small tile
]


PAD_CASES = [  # H, W, oh, ow, pl, pt; every how unless listed
    (5, 7, 5, 7, 0, 0, None),                        # pads of 0
    (5, 7, 13, 19, 6, 4, None),                      # n - 1 on every side
    (5, 7, 6, 7, -2, 3, None),                       # mixed signs: crops the left and the bottom, pads the top and the right
    (2, 2, 4, 4, 1, 1, (PAD_REFLECT,)),            # reflect at n == 2
    (3, 4, 9, 12, 4, 3, (PAD_CIRCULAR,)),          # circular at pad == n
    (3, 4, 17, 4, 0, 7, (PAD_CIRCULAR,)),          # circular at pad > n: wraps again (include/maua_hip.h; torch refuses)
]


CONV_SHAPES = [(1, 2, 129), (1, 129, 2), (2, 3, 43), (2, 43, 3), (1, 17, 121), (1, 121, 17), (258, 1, 1)]     # planes H W = 257 k + 1


# ============================================================================================================ conv1d_reflect and its vjp
def conv1d_matrix(n, taps, mutant=None):
    """M [n, n] float64: y = M x for the correlation with reflect padding (maua/ops/image.py:226-236), radius < n"""
    radius = (len(taps) - 1) // 2
    M = np.zeros((n, n))
    for k in range(-radius, radius + 1):
        src = pad_src(np.arange(n) + k + (1 if mutant == "tap+1" else 0), n, PAD_REFLECT, mutant)
        np.add.at(M, (np.arange(n), src), float(taps[k + radius]))
    return M


def conv1d_reflect(x, taps, axis, vjp=False, mutant=None):
    """x [planes, H, W] float32 -> (y float64, bound): along H (axis 0) or W (axis 1); vjp: the transposed matrix (the adjoint).
    Bound: a chain of 2 radius + 1 multiply-adds, (2 radius + 1) u sum |taps| |x| - the adjoint's chain visits up to three reflections of
    each tap, so its count is the largest number of non-zero terms of a row, 3 (2 radius + 1) at most."""
    x = d(x)
    n = x.shape[1 + axis]
    taps = np.asarray(taps, F)
    M = conv1d_matrix(n, taps, mutant)
    A = np.zeros((n, n))
    radius = (len(taps) - 1) // 2
    for k in range(-radius, radius + 1):
        np.add.at(A, (np.arange(n), pad_src(np.arange(n) + k, n, PAD_REFLECT)), abs(float(taps[k + radius])))
    terms = len(taps)
    if vjp:
        M, A, terms = M.T, A.T, 3 * len(taps)
    xm = np.moveaxis(x, 1 + axis, -1)
    y, mag = xm @ M.T, np.abs(xm) @ A.T
    return np.moveaxis(y, -1, 1 + axis), np.moveaxis(terms * U * mag, -1, 1 + axis)


# ============================================================================================================ bicubic (modes 0 / 2) and its vjp
A_KEYS = -0.75
BICUBIC_SHAPES = [(1, 1, 3, 5), (5, 7, 1, 1), (2, 3, 2, 3), (4, 4, 33, 31), (67, 61, 8, 9), (3, 515, 2, 1029)]     # (H, W) -> (oh, ow)
BICUBIC_VJP_EXTRA = [(5, 7, 1, 6), (1, 7, 4, 6)]                                                                 # n_out == 1 / n_in == 1 on one axis only


def _keys(t):
    """the four Keys weights (A = -0.75) of fraction t in float64, their derivatives in t and their float32 evaluation's error: Horner's
    steps with a running bound (every product and every sum rounds once on its own magnitude, the earlier error rides through the
    later multiplications by x) plus the argument's rounding (t + 1, 1 - t, 2 - t: u |x| through the derivative; t itself is exact)"""
    A = A_KEYS

    def outer(x):                                                 # ((A x - 5 A) x + 8 A) x - 4 A
        a = A * x
        p1 = a - 5 * A
        b = p1 * x
        p2 = b + 8 * A
        c = p2 * x
        p3 = c - 4 * A
        e = U * (np.abs(a) + np.abs(p1))
        e = e * x + U * (np.abs(b) + np.abs(p2))
        e = e * x + U * (np.abs(c) + np.abs(p3))
        dv = 3 * A * x * x - 10 * A * x + 8 * A
        return p3, dv, e + np.abs(dv) * U * x

    def inner(x, exact_arg):                                      # ((A + 2) x - (A + 3)) x x + 1
        a = (A + 2) * x
        p1 = a - (A + 3)
        b = p1 * x
        c = b * x
        p3 = c + 1
        e = U * (np.abs(a) + np.abs(p1))
        e = e * x + U * np.abs(b)
        e = e * x + U * (np.abs(c) + np.abs(p3))
        dv = 3 * (A + 2) * x * x - 2 * (A + 3) * x
        return p3, dv, e + (0.0 if exact_arg else np.abs(dv) * U * x)
    c0, d0, e0 = outer(t + 1.0)
    c1, d1, e1 = inner(t, True)
    c2, d2, e2 = inner(1.0 - t, False)
    c3, d3, e3 = outer(2.0 - t)
    return np.stack([c0, c1, c2, c3], -1), np.stack([d0, d1, -d2, -d3], -1), np.stack([e0, e1, e2, e3], -1)


def bicubic_axis(n_in, n_out, align, mutant=None):
    """one axis of ATen's upsample_bicubic2d as matrices [n_out, n_in]: M (the weights, clamped taps added up), A (the same of
    magnitudes), D (of the weights' derivatives in the source coordinate), E (the coefficients' own error) and ds [n_out] (the
    coordinate's).  Decisions in float32 as ATen takes them: scale = float(in) / float(out) (align_corners: (in - 1) / (out - 1), 0 for one
    output), s = (o + 0.5) scale - 0.5 with every operation rounded, floor(s), t = s - floor(s) (exact); the weights from t in float64.
    ds = 2 ulp(p), p = (o + 0.5) scale: a kernel that fuses the multiply and the subtraction differs by one rounding of p, and the exact
    coordinate by the roundings of scale, p and s; a flip of floor(s) between the two needs no exclusion (the interpolant is continuous).
    E: the coefficients' own float32 evaluation (_keys)."""
    o = np.arange(n_out).astype(F)
    if align:
        scale = F(n_in - 1) / F(n_out - 1) if n_out > 1 else F(0)
        p = o * scale
        s = p
    else:
        scale = F(n_in) / F(n_out)
        p = (o + F(0.5)) * scale
        s = p - F(0.5)
    assert s.dtype == F
    f = np.floor(s)
    c, dc, ec = _keys(d(s - f))
    i0 = f.astype(np.int64) - 1 + (1 if mutant == "tap+1" else -1 if mutant == "tap-1" else 0)
    M, A, D, E = (np.zeros((n_out, n_in)) for _ in range(4))
    rows = np.arange(n_out)
    for k in range(4):
        idx = np.clip(i0 + k, 0, n_in if mutant == "clamp_n" else n_in - 1)
        keep = idx < n_in                                          # (the clamp_n mutant reads past the end: dropped)
        idx = np.minimum(idx, n_in - 1)
        np.add.at(M, (rows[keep], idx[keep]), c[keep, k])
        np.add.at(A, (rows[keep], idx[keep]), np.abs(c[keep, k]))
        np.add.at(D, (rows[keep], idx[keep]), dc[keep, k])
        np.add.at(E, (rows[keep], idx[keep]), ec[keep, k])
    ds = 2.0 * d(np.spacing(np.abs(p).astype(F)))
    if align and n_out == 1:
        ds = np.zeros(1)
    return M, A, D, E, ds


def bicubic(x, oh, ow, align, dt="f32", mutant=None):
    """x [N, C, H, W] (numbers of the dtype) -> (out float64, bound): rows of four x taps, then four y taps.
    x pass: r = sum_j cx_j x_j: 4 u sum |cx| |x| + sum ecx |x| + dsx |sum cx'_j x_j|.  y pass: 4 u sum |cy| (sum |cx| |x|) + sum ecy |r|
    + sum |cy| er + dsy |sum cy'_i r_i|.  The store: half a unit of the output type."""
    x = d(x)
    H, W = x.shape[-2:]
    Mx, Ax, Dx, Ex, dsx = bicubic_axis(W, ow, align, mutant)
    My, Ay, Dy, Ey, dsy = bicubic_axis(H, oh, align, mutant)
    r, rmag = x @ Mx.T, np.abs(x) @ Ax.T
    er = 4 * U * rmag + np.abs(x) @ Ex.T + dsx * np.abs(x @ Dx.T)
    v = My @ r
    ev = 4 * U * (Ay @ rmag) + Ey @ rmag + Ay @ er + dsy[:, None] * np.abs(Dy @ r)
    return v, ev + half_ulp(np.abs(v) + ev, dt)


def bicubic_vjp(gy, H, W, align, mutant=None):
    """gy [N, C, oh, ow] -> (gx [N, C, H, W] float64, bound): the transposed matrices, columns first (the kernel's order).
    A pass sums, per input sample, one term per output that touches it (its weight: up to four coefficients added up, 3 u): (count + 3) u
    sum |w| |g| + sum e |g| + sum_o ds_o |w'_o g_o| (every output has its own coordinate error: no cancellation is claimed)."""
    g = d(gy)
    oh, ow = g.shape[-2:]
    Mx, Ax, Dx, Ex, dsx = bicubic_axis(W, ow, align)
    My, Ay, Dy, Ey, dsy = bicubic_axis(H, oh, align)
    if mutant == "no_clamped_taps":                                # the window misses what the clamp folds onto the last sample
        Mx = Mx.copy()
        Mx[:, -1] = np.where(np.arange(ow) >= ow - 1, 0.0, Mx[:, -1])
    cx, cy = (Ax > 0).sum(0), (Ay > 0).sum(0)
    tmp, tmag = g @ Mx, np.abs(g) @ Ax
    et = (cx + 3) * U * tmag + np.abs(g) @ Ex + np.abs(g) @ (dsx[:, None] * np.abs(Dx))
    out = My.T @ tmp
    e = (cy + 3)[:, None] * U * (Ay.T @ tmag) + Ey.T @ tmag + Ay.T @ et + (dsy[:, None] * np.abs(Dy)).T @ tmag
    return out, e


# ============================================================================================================ cutouts and their vjp
CUT_GREY, CUT_FLIP, CUT_SIZE_MASK = 1 << 30, 1 << 29, (1 << 24) - 1
CT_MAXT = 16
LUMA = (F(0.2989), F(0.587), F(0.114))


def cubic32(x):
    """resize_right interp_methods.cubic in float32, every operation rounded (the masks multiply by 1 or 0: exact)"""
    a = np.abs(x)
    a2 = a * a
    a3 = a2 * a
    near = (F(1.5) * a3 - F(2.5) * a2) + F(1.0)
    far = ((F(-0.5) * a3 + F(2.5) * a2) - F(4.0) * a) + F(2.0)
    out = np.where(a <= F(1), near, np.where(a <= F(2), far, F(0)))
    assert out.dtype == F
    return out


def cutout_tables32(size, cs, mutant=None):
    """one dimension of resize_right.resize(out_shape = cs) of a cutout of `size` samples, the float32 arithmetic of the published
    algorithm in its order -> (left int [cs], w float32 [cs, taps]): the projected grid o / scale + (size - 1) / 2 - (cs - 1) / (2 scale),
    left = ceil(p - support / 2 - eps), taps = ceil(support - eps), weights cubic(p - i) (scale cubic(scale (p - i)) when shrinking),
    summed in tap order, divided by the sum."""
    scale_d = cs / size
    scale = F(scale_d)
    eps = 2.0 ** -23
    pf = np.arange(cs).astype(F) / scale
    pf = pf + F((size - 1) / 2.0)
    pf = pf - F((cs - 1) / (2.0 * scale_d))
    aa = scale_d < 1.0
    support = 4.0 / scale_d if aa else 4.0
    edge = (pf - F(support / 2.0)) - F(eps)
    left = (np.floor(edge) if mutant == "left_floor" else np.ceil(edge)).astype(np.int64)
    taps = min(int(np.ceil(support - eps)), CT_MAXT)
    arg = pf[:, None] - (left[:, None] + np.arange(taps)[None, :]).astype(F)
    w = scale * cubic32(scale * arg) if aa else cubic32(arg)
    s = np.zeros(cs, F)
    for k in range(taps):
        s = s + w[:, k]
    s[s == 0] = F(1)
    w = w / s[:, None]
    assert w.dtype == F
    return left, w


def cutout_matrix(size, cs, mutant=None):
    """the table as a dense [cs, size] matrix (taps outside the cutout dropped: zero padding) and the chain length"""
    left, w = cutout_tables32(size, cs, mutant)
    Wm = np.zeros((cs, size))
    for k in range(w.shape[1]):
        idx = left + k
        ok = (idx >= 0) & (idx < size)
        Wm[np.arange(cs)[ok], idx[ok]] += d(w[ok, k])
    return Wm, w.shape[1]


def cutouts(img, rects, cs, mul, add, mean, std, mutant=None):
    """img [B, 3, H, W], rects [(size | flags, top, left)] -> (out [n_cut * B, 3, cs, cs] float64 cutout-major, bound).
    v = img mul + add: one fused rounding, u |v|; a grey cutout's luma 0.2989 v0 + 0.587 v1 + 0.114 v2 carries those and three roundings
    on its terms.  Rows then columns, taps multiply-adds each: 2 taps u sum |wx| sum |wy| |v| + sum |wx| sum |wy| ev.  (acc - mean) / std
    as (acc - mean) * (1 / std): u |acc - mean|, then 2 u of the result (the reciprocal's rounding and the product's).  A flipped cutout
    is stored mirrored."""
    x = d(img)
    B = x.shape[0]
    mean, inv = d(np.asarray(mean, F)), d(F(1.0) / np.asarray(std, F))
    mul, add = float(F(mul)), float(F(add))
    outs, bounds = [], []
    for rs, top, left in rects:
        size = rs & CUT_SIZE_MASK
        Wm, taps = cutout_matrix(size, cs, mutant)
        v = x[:, :, top:top + size, left:left + size] * mul + add
        ev, mag = U * np.abs(v), np.abs(v)
        if rs & CUT_GREY:
            lum = d(np.asarray(LUMA))[None, :, None, None]
            ev = ((lum * ev).sum(1, keepdims=True) + 3 * U * (lum * mag).sum(1, keepdims=True)).repeat(3, 1)
            mag = (lum * mag).sum(1, keepdims=True).repeat(3, 1)
            v = (lum * v).sum(1, keepdims=True).repeat(3, 1) if mutant != "grey_one_plane" else v[:, :1].repeat(3, 1)
        acc = Wm @ v @ Wm.T
        Wa = np.abs(Wm)
        eacc = 2 * taps * U * (Wa @ mag @ Wa.T) + Wa @ ev @ Wa.T
        c = acc - mean[None, :, None, None]
        o = c * inv[None, :, None, None]
        e = (eacc + U * np.abs(c)) * inv[None, :, None, None] + 2 * U * np.abs(o)
        if rs & CUT_FLIP and mutant != "no_flip":
            o, e = o[..., ::-1], e[..., ::-1]
        outs.append(o)
        bounds.append(e)
    return np.concatenate(outs, 0), np.concatenate(bounds, 0)


def cutouts_vjp(d_out, B, H, W, rects, cs, mul, std, mutant=None):
    """d_out [n_cut * B, 3, cs, cs] -> (d_img [B, 3, H, W] float64, bound): the transpose of `cutouts`' linear part, the cutouts added up in
    their order.  Horizontal adjoint th = sum_x w d / std: (count + 2) u on its terms (the chain, the reciprocal and its product); the
    vertical adjoint and the sum over the cutouts that cover a pixel: a chain of all their terms, + 3 for a grey cutout's plane sum
    and luma product, + 1 for the final product with mul."""
    g = d(d_out)
    inv = d(F(1.0) / np.asarray(std, F))[None, :, None, None]
    mul = float(F(mul))
    out, mag, carried, count = (np.zeros((B, 3, H, W)) for _ in range(4))
    for n, (rs, top, left) in enumerate(rects):
        size = rs & CUT_SIZE_MASK
        Wm, _taps = cutout_matrix(size, cs)
        Wa = np.abs(Wm)
        dn = g[n * B:(n + 1) * B]
        if rs & CUT_FLIP and mutant != "store_only_flip":
            dn = dn[..., ::-1]
        dn = dn * inv
        cx = (Wa > 0).sum(0)
        th, tmag = dn @ Wm, np.abs(dn) @ Wa
        eth = (cx + 2) * U * tmag
        if rs & CUT_GREY:
            lum = d(np.asarray(LUMA))[None, :, None, None]
            s, smag, es = th.sum(1, keepdims=True), tmag.sum(1, keepdims=True), eth.sum(1, keepdims=True)
            if mutant == "grey_one_plane":
                s = th[:, :1]
            th, tmag, eth = lum * s, lum * smag, lum * (es + 3 * U * smag)
        sl = (slice(None), slice(None), slice(top, top + size), slice(left, left + size))
        out[sl] += Wm.T @ th
        mag[sl] += Wa.T @ tmag
        carried[sl] += Wa.T @ eth
        count[sl] += (cx[:, None] + (3 if rs & CUT_GREY else 0)) * np.ones((1, size))
    return out * mul, abs(mul) * ((count + 1) * U * mag + carried)


CUTOUT_IMAGES = {8: ((31, 29), (33, 31)), 32: ((31, 29), (129, 127))}    # per cut size: the image, and one whose short side is the largest size
#                                                                          the cut size allows (4 cs - 1 = 31 / 127: sixteen taps)


def cutout_rects(cs, H, W):
    """the GPU test's rectangles for cut size cs in an H x W image (the flag combinations spread over them): the cut size itself
    (identity weights 0, 0, 1, 0), 1, cs - 1 (up-sampling with four taps), min(H, W), the largest size the launcher allows, one flush in
    each corner, two that overlap, and grey / flipped ones on top of others - every size clipped to the image"""
    m = min(H, W, 4 * cs - 1)
    flags = (0, CUT_GREY, CUT_FLIP, CUT_GREY | CUT_FLIP)
    want = [(cs, 3, 2), (1, 5, 7), (cs - 1, 0, 0), (min(H, W), 0, 0), (m, 1, 1),
            (5, 0, 0), (5, 0, W - 5), (5, H - 5, 0), (5, H - 5, W - 5),
            (9, 10, 10), (9, 13, 12), (cs, 1, 1), (7, 11, 11), (cs, 0, 0), (6, 20, 3), (cs - 1, 2, 1)]
    out = []
    for i, (size, top, left) in enumerate(want):
        size = max(1, min(size, m))
        out.append((size | flags[i % 4], min(top, H - size), min(left, W - size)))
    return out


# ============================================================================================================ colour match
TWO_PI32 = F(6.283185307179586)
FIX = 2.0 ** 40
CM_NBINS = (2, 3, 64, 255, 1024)


def cm_odd_nbins():
    """the bin counts in 2 .. 1024 whose last inner edge float32(nbins - 1) * float32(1 / (nbins - 1)) is not 1"""
    return [n for n in range(2, 1025) if F(n - 1) * F(1.0 / (n - 1)) != F(1)]


def cm_edges32(nbins):
    return np.arange(nbins + 2).astype(F) * F(1.0 / (nbins - 1))


def cm_pixel32(r, g, b, sat_weighting):
    """one pixel of ColorMatchGrads.histogram up to the histogram's inputs, float32, every operation rounded, in kornia's order:
    u = (in + 1) / 2, clamp(1e-8, 1), max / min with the FIRST maximal / minimal channel, delta, s = delta / (max + 1e-8), the hue of the
    maximal channel's branch / delta', / 6, torch's % 1 (fmod, + 1 when negative), 2 pi, clamp(0, 1), w = sqrt(clamp(s) clamp(v))."""
    c = np.stack([np.asarray(t, F) for t in (r, g, b)])
    u = (c + F(1)) / F(2)
    live = (u >= F(1e-8)) & (u <= F(1))
    c = np.minimum(np.maximum(u, F(1e-8)), F(1))
    im, imin = np.argmax(c, 0), np.argmin(c, 0)                      # numpy's argmax / argmin: the first
    M, m = np.take_along_axis(c, im[None], 0)[0], np.take_along_axis(c, imin[None], 0)[0]
    delta = M - m
    s = delta / (M + F(1e-8))
    deltap = np.where(delta == 0, F(1), delta)
    rc, gc, bc = M - c[0], M - c[1], M - c[2]
    num = np.where(im == 0, bc - gc, np.where(im == 1, rc - bc, gc - rc))
    off = np.where(im == 0, F(0), np.where(im == 1, F(2), F(4)))
    hh = np.where(im == 0, num / deltap, (num + off * deltap) / deltap)
    q = hh / F(6)
    fr = np.fmod(q, F(1))
    fr = np.where(fr < 0, fr + F(1), fr)
    hue_raw = TWO_PI32 * fr
    x = np.minimum(np.maximum(hue_raw, F(0)), F(1))
    sc, vc = np.minimum(np.maximum(s, F(0)), F(1)), np.minimum(np.maximum(M, F(0)), F(1))
    w = np.sqrt(sc * vc) if sat_weighting else np.ones_like(x)
    for t in (u, delta, s, hh, q, fr, hue_raw, x, w):
        assert t.dtype == F
    return dict(c=c, live=live, im=im, imin=imin, M=M, delta=delta, deltap=deltap, num=num, hue_raw=hue_raw, x=x, s=s, v=M, sc=sc, vc=vc, w=w)


def cm_bins(x, nbins, mutant=None):
    """-> (k, lo, hi, ok): e_k <= x < e_k+1 on the float32 edges e_j = float32(j) * float32(1 / (nbins - 1)), k <= nbins - 1"""
    e = cm_edges32(nbins)
    if mutant == "delta_nbins":
        e = np.arange(nbins + 2).astype(F) * F(1.0 / nbins)
    k = np.minimum(np.searchsorted(e[:nbins], x, side="right") - 1, nbins - 1)
    lo, hi = e[k], e[k + 1]
    return k, lo, hi, (x >= lo) & (x < hi)


def cm_hist_fix(img, nbins, sat_weighting, mutant=None):
    """img [B, 3, HW] -> the 2^-40 fixed-point sums as exact Python-width integers (uint64 arithmetic: sums have no order)"""
    B = img.shape[0]
    fix = np.zeros((B, nbins), np.uint64)
    for b in range(B):
        h = cm_pixel32(img[b, 0], img[b, 1], img[b, 2], sat_weighting)
        k, lo, hi, ok = cm_bins(h["x"], nbins, mutant)
        a = (hi - h["x"]) * h["w"]
        c = (h["x"] - lo) * h["w"]
        assert a.dtype == F and c.dtype == F
        fa = np.floor(d(a) * FIX + 0.5).astype(np.uint64)
        fc = np.floor(d(c) * FIX + 0.5).astype(np.uint64)
        ka, kc = (k + 1, k) if mutant == "bins_swapped" else (k, k + 1)
        sel = ok & (ka <= nbins - 1)
        np.add.at(fix[b], ka[sel], fa[sel])
        sel = ok & (kc <= nbins - 1)
        np.add.at(fix[b], kc[sel], fc[sel])
    return fix


def cm_block_sum32(part):
    """block_sum of 256 per-thread float32 values [.., 256]: the xor butterfly over each wave of 64 lanes (every lane ends with the
    same sum: float32 addition commutes), then the four waves' sums added to 0 in order"""
    v = np.asarray(part, F).reshape(*part.shape[:-1], 4, 64)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    t = np.zeros(v.shape[:-2], F)
    for i in range(4):
        t = t + v[..., i, 0]
    return t


def cm_final32(fix):
    """-> (Hs float32 [B, nbins], S float32 [B], Hn = Hs / S): thread t adds bins t, t + 256, ... in order, then block_sum"""
    B, nbins = fix.shape
    Hs = (fix.astype(np.float64) / FIX).astype(F)
    pad = np.zeros((B, -(-nbins // 256) * 256), F)
    pad[:, :nbins] = Hs
    part = np.zeros((B, 256), F)
    for j in range(pad.shape[1] // 256):
        part = part + pad[:, j * 256:(j + 1) * 256]
    S = cm_block_sum32(part)
    with np.errstate(invalid="ignore", divide="ignore"):
        return Hs, S, Hs / S[:, None]


def cm_grad(img, nbins, sat_weighting, target, scale):
    """img [B, 3, HW], target [nbins] or [B, nbins] -> (grad [B, 3, HW] float64, bound, loss [B] float64, its bound): the closed form of csrc/colormatch.hip in
    float64 at the float32 decisions (first maximal / minimal channel, bin, live clamps, the exact float32 histogram sums Hs).
    Bound, first order in u, from the magnitudes of the terms added into each dc[i]:
      gR: S carries nS = ceil(nbins / 256) + 10 roundings (per-thread sums, six butterfly steps, four waves), Hn = Hs / S one more: eH =
      (nS + 1) u Hn; d = Hn - t: eH + u |d|; gk = 2 coef d: 2 coef ed + 2 u |gk|; the dot's terms 2 coef d Hn: 2 coef (|Hn| ed + |d| eH) +
      3 u |term|, summed with nS roundings on the magnitudes; gR = (gk - gdot) / S: (egk + egdot + u |gk - gdot|) / S + (nS + 1) u |gR|.
      per pixel: dx = w (g1 - g0) and dw = (hi - x) g0 + (x - lo) g1 carry egR through their factors and 3 u of their terms; every
      term added into dc[i] (dv, the two saturation terms, +-dnum, +-dd) carries its inputs' share and 5 u of its own magnitude (at
      most five rounded operations make a term: a product or quotient chain), and the additions into dc[i] u times the magnitudes added;
      the final 0.5 is exact."""
    B, _, HW = img.shape
    fix = cm_hist_fix(img, nbins, sat_weighting)
    Hs, S32, _ = cm_final32(fix)
    Hs = d(Hs)
    coef = float(F(scale) / (F(B) * F(nbins)))
    nS = -(-nbins // 256) + 10
    S = Hs.sum(1, keepdims=True)
    t = np.broadcast_to(d(target).reshape(-1, nbins), (B, nbins))
    with np.errstate(invalid="ignore", divide="ignore"):
        Hn = Hs / S
        eH = (nS + 1) * U * Hn
        dd_ = Hn - t
        ed = eH + U * np.abs(dd_)
        gk = 2 * coef * dd_
        egk = 2 * coef * ed + 2 * U * np.abs(gk)
        term = 2 * coef * dd_ * Hn
        gdot = term.sum(1, keepdims=True)
        egdot = (2 * coef * (np.abs(Hn) * ed + np.abs(dd_) * eH) + (3 + nS) * U * np.abs(term)).sum(1, keepdims=True)
        gR = (gk - gdot) / S
        egR = (egk + egdot + U * np.abs(gk - gdot)) / S + (nS + 1) * U * np.abs(gR)
        loss = coef * (dd_ ** 2).sum(1)
        # the loss's share: d^2 carries 2 |d| ed and its own rounding, the sum nS roundings on the terms, coef one more
        eloss = coef * ((2 * np.abs(dd_) * ed + U * dd_ ** 2).sum(1) + nS * U * (dd_ ** 2).sum(1)) + U * loss
    e = d(cm_edges32(nbins))
    grad, bound = np.zeros((B, 3, HW)), np.zeros((B, 3, HW))
    for b in range(B):
        h = cm_pixel32(img[b, 0], img[b, 1], img[b, 2], sat_weighting)
        k, lo, hi, ok = cm_bins(h["x"], nbins)
        x, w = d(h["x"]), d(h["w"])
        has1 = k + 1 <= nbins - 1
        g0, eg0 = gR[b][k], egR[b][k]
        g1, eg1 = np.where(has1, gR[b][np.minimum(k + 1, nbins - 1)], 0.0), np.where(has1, egR[b][np.minimum(k + 1, nbins - 1)], 0.0)
        dx = np.where(ok, w * (g1 - g0), 0.0)
        edx = np.where(ok, w * (eg0 + eg1) + 3 * U * w * (np.abs(g0) + np.abs(g1)), 0.0)
        lo64, hi64 = e[k], e[k + 1]
        dw = np.where(ok, (hi64 - x) * g0 + (x - lo64) * g1, 0.0)
        edw = np.where(ok, (hi64 - x) * eg0 + (x - lo64) * eg1 + 3 * U * ((hi64 - x) * np.abs(g0) + (x - lo64) * np.abs(g1)), 0.0)
        dc, mag, err = np.zeros((3, HW)), np.zeros((3, HW)), np.zeros((3, HW))
        px = np.arange(HW)

        def add(ch, val, e_in):
            np.add.at(dc, (ch, px), val)
            np.add.at(mag, (ch, px), np.abs(val))
            np.add.at(err, (ch, px), e_in + 5 * U * np.abs(val))
        sd, vv, sc, vc = d(h["s"]), d(h["v"]), d(h["sc"]), d(h["vc"])
        with np.errstate(invalid="ignore", divide="ignore"):
            on = bool(sat_weighting) & (w > 0)
            ds = np.where(on & (sd >= 0) & (sd <= 1), dw * vc / (2 * w), 0.0)
            eds = np.where(on & (sd >= 0) & (sd <= 1), edw * vc / (2 * w) + 4 * U * np.abs(ds), 0.0)
            dv = np.where(on & (vv >= 0) & (vv <= 1), dw * sc / (2 * w), 0.0)
            edv = np.where(on & (vv >= 0) & (vv <= 1), edw * sc / (2 * w) + 4 * U * np.abs(dv), 0.0)
        im, imin = h["im"], h["imin"]
        M, delta, deltap, num = d(h["M"]), d(h["delta"]), d(h["deltap"]), d(h["num"])
        Me = M + float(F(1e-8))
        add(im, dv, edv)
        add(im, ds / Me, eds / Me)
        add(im, -ds * delta / (Me * Me), eds * delta / (Me * Me))
        add(imin, -ds / Me, eds / Me)
        hue_on = (h["hue_raw"] >= 0) & (h["hue_raw"] <= 1) & ~(dx == 0)
        k6 = float(TWO_PI32 / F(6))
        dhh, edhh = np.where(hue_on, dx * k6, 0.0), np.where(hue_on, edx * k6, 0.0)
        dnum, ednum = dhh / deltap, edhh / deltap
        ia = np.where(im == 0, 1, np.where(im == 1, 2, 0))
        ib = np.where(im == 0, 2, np.where(im == 1, 0, 1))
        add(ia, dnum, ednum)
        add(ib, -dnum, ednum)
        ddv = np.where(delta != 0, -dhh * num / (deltap * deltap), 0.0)
        edd = np.where(delta != 0, edhh * np.abs(num) / (deltap * deltap), 0.0)
        add(im, ddv, edd)
        add(imin, -ddv, edd)
        grad[b] = np.where(h["live"], 0.5 * dc, 0.0)
        bound[b] = np.where(h["live"], 0.5 * (err + 7 * U * mag), 0.0)
    return grad, bound, loss, eloss


def cm_edge_pixels(nbins, want=4):
    """pixels whose hue lands exactly on an inner edge e_k (0 < e_k < 1): red maximal at u = 1, blue minimal at u = 0.25, the green
    channel searched over the float32 neighbours of the real solution -> list of (k, (r, g, b))"""
    e = cm_edges32(nbins)
    found = []
    for k in range(1, nbins - 1):
        if e[k] >= 1 or len(found) >= want:
            break
        gu = 0.25 + 0.75 * 6.0 * float(e[k]) / (2 * np.pi)
        g0 = F(2 * gu - 1)
        cand = g0 + np.arange(-64, 65).astype(F) * np.spacing(g0)
        h = cm_pixel32(np.ones_like(cand), cand, np.full_like(cand, -0.5), True)
        hit = np.nonzero(h["x"] == e[k])[0]
        if hit.size:
            found.append((k, (F(1), cand[hit[0]], F(-0.5))))
    return found


def cm_special_pixels(nbins):
    """-> (pixels [B, 3] float32, tags): one single-pixel image per special colour.  u = (in + 1) / 2 cannot be exactly float32(1e-8) (the
    inputs next to -1 are 2^-24 apart, so u steps by 2^-25 = 2.98e-8): the clamp's two sides are u = 0 (clamped, not live) and u = 2^-25
    (the smallest live value), both here."""
    tiny = F(-1) + F(2.0 ** -24)
    px = [("grey", (0.2, 0.2, 0.2)), ("red max", (0.5, 0.1, -0.3)), ("green max", (-0.3, 0.5, 0.1)), ("blue max", (0.1, -0.3, 0.5)),
          ("tie r g", (0.5, 0.5, 0.1)), ("tie g b", (0.1, 0.5, 0.5)), ("tie r b", (0.5, 0.1, 0.5)), ("tie of three at 1", (1.0, 1.0, 1.0)),
          ("min tie", (0.5, 0.1, 0.1)), ("below -1 and above 1", (-1.5, 0.2, 2.0)), ("exactly -1 and 1", (-1.0, 1.0, 0.3)),
          ("all at -1", (-1.0, -1.0, -1.0)), ("u = 2^-25", (tiny, 0.5, 0.2)), ("u = 0", (-1.0, 0.5, 0.2)),
          ("small hue", (0.9, -0.2, -0.3)), ("hue above one radian", (0.2, 0.9, -0.5)), ("black to red", (1.0, -1.0, -1.0))]
    # a tiny negative q: red maximal, green just below blue -> (bc - gc) / delta / 6 is a tiny negative number, fmod keeps it, + 1 gives 1
    # (steps of 2^-23 in the input: what survives (in + 1) / 2 near 0.1; one step gives q = -2.5e-8 and q + 1 rounds to exactly 1)
    for ulp in (1, 2, 3):
        b = F(0.1)
        px.append((f"q tiny negative ({ulp} steps)", (0.9, b - F(ulp * 2.0 ** -23), b)))
    for k, p in cm_edge_pixels(nbins):
        px.append((f"hue on edge {k}", p))
    for i, p in enumerate(uniform((300, 3), 17 + nbins, -1.2, 1.2)):              # and random colours up to a few hundred images
        px.append((f"random {i}", tuple(p)))
    arr = np.array([p for _, p in px], F)
    return arr, [t for t, _ in px]


def cm_random_image():
    """[3, 3, 37 * 53] in [-1.2, 1.2] with a grey band (delta == 0, weight 0) and a clipped band"""
    img = uniform((3, 3, 37 * 53), 2, -1.2, 1.2)
    img[:, :, :200] = img[:, :1, :200]
    return img


def cm_target(nbins, sat_weighting, B):
    """B normalised histograms of other random images (float32)"""
    t = uniform((B, 3, 400), 11 + nbins, -1.0, 1.0)
    return cm_final32(cm_hist_fix(t, nbins, sat_weighting))[2]
