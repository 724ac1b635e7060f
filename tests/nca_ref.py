"""Numpy restatement of the neural cellular automaton (maua/nca/train.py:152-193, generate.py:25-36) - TEST INFRASTRUCTURE.

Shares nothing with maua_amd.  Everything is evaluated in ``dtype`` (float64 by default) EXCEPT the update mask, which is float32 arithmetic
by definition: ``floor(float32(u) + float32(rate))``, what both the reference (torch.rand + rate in float32) and the kernel compute.

``step(..., bound=...)`` also returns an element-wise bound on |float32 evaluation - exact value| that holds for any summation order:
every sum of n terms is charged n * 2^-24 * sum|terms| (Higham's gamma_n, one rounding per operation), errors of an earlier stage travel
through the later ones by the triangle inequality (ReLU is 1-Lipschitz), and an incoming error ``dx`` of the state travels the same way, so a
trajectory's bound is built step by step.  ``split=True`` adds 2^-16 * sum|products| per product for the hi/lo bf16 form: |lo| <= 2^-9 |v|,
so the dropped lo*lo term is <= 2^-18 of a product and the bf16 rounding of the two lo parts another 2 * 2^-18.

``mutant`` names one deliberate mistake (tests/test_nca_host.py shows that each changes a compared result).
"""
import numpy as np

EPS = 2.0 ** -24

# taps [filter][dy][dx] applied as a correlation (torch.nn.functional.conv2d): identity, sobel_x, sobel_x^T, laplacian (train.py:153-155)
IDENT = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], dtype=np.float64)
SOBEL_X = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.float64)
LAP = np.array([[1, 2, 1], [2, -12, 2], [1, 2, 1]], dtype=np.float64)

MUTANTS = ("zero_pad", "swap_sobel", "filter_major", "mask_per_channel", "mask_on_sum", "no_bias", "relu_after_w2", "window_no_margin",
           "window_full_torus")
HEAD_MUTANTS = ("gram_no_hw", "mean_after_square")       # of the batch-mean Gram loss (gram_mean_head)


def filters(mutant=None):
    f = [IDENT, SOBEL_X, SOBEL_X.T, LAP]
    if mutant == "swap_sobel":
        f = [IDENT, SOBEL_X.T, SOBEL_X, LAP]
    return f


def _shift(x, dy, dx, zero_pad):
    """x[..., y + dy, x + dx] (circular, or zero outside the grid)"""
    out = np.roll(x, (-dy, -dx), axis=(-2, -1))
    if zero_pad:
        h, w = x.shape[-2:]
        if dy == -1:
            out[..., 0, :] = 0
        if dy == 1:
            out[..., h - 1, :] = 0
        if dx == -1:
            out[..., :, 0] = 0
        if dx == 1:
            out[..., :, w - 1] = 0
    return out


def perception(x, dtype=np.float64, mutant=None, reverse=False):
    """[B, C, H, W] -> [B, 4 C, H, W], feature 4 c + f.  ``reverse``: the taps summed in the opposite order (exactness checks)."""
    x = np.asarray(x, dtype=dtype)
    b, c, h, w = x.shape
    out = np.zeros((b, c, 4, h, w), dtype=dtype)
    order = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
    if reverse:
        order = order[::-1]
    for fi, f in enumerate(filters(mutant)):
        for dy, dx in order:
            t = f[dy + 1, dx + 1]
            if t != 0:
                out[:, :, fi] = out[:, :, fi] + dtype(t) * _shift(x, dy, dx, mutant == "zero_pad")
    if mutant == "filter_major":
        return out.transpose(0, 2, 1, 3, 4).reshape(b, 4 * c, h, w)
    return out.reshape(b, 4 * c, h, w)


def _abs_perception(x):
    """sum |tap| |x| per feature: perception with the taps' magnitudes"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    b, c, h, w = x.shape
    out = np.zeros((b, c, 4, h, w))
    for fi, f in enumerate(filters()):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                out[:, :, fi] += abs(f[dy + 1, dx + 1]) * _shift(x, dy, dx, False)
    return out.reshape(b, 4 * c, h, w)


def mask_of(u, rate):
    """floor(u + rate) in float32; u [B, H, W], rate a scalar or [H, W]"""
    return np.floor(np.asarray(u, dtype=np.float32) + np.asarray(rate, dtype=np.float32)).astype(np.float32)


def _dot(w, v, dtype, reverse):
    """sum_k w[n, k] v[b, k, y, x] accumulated term by term in ``dtype`` (k ascending, or descending)"""
    ks = range(w.shape[1])
    if reverse:
        ks = reversed(ks)
    acc = np.zeros((v.shape[0], w.shape[0]) + v.shape[2:], dtype=dtype)
    for k in ks:
        acc = acc + w[None, :, k, None, None] * v[:, None, k]
    return acc


def step(x, w1, b1, w2, u, rate=0.5, dtype=np.float64, mutant=None, reverse=False, bound=None, split=False):
    """One update.  u [B, H, W].  bound: None, or the incoming state's element-wise error (0 for an exact state): then returns (x', dx')."""
    x = np.asarray(x, dtype=dtype)
    w1, b1, w2 = (np.asarray(a, dtype=dtype) for a in (w1, b1, w2))
    p = perception(x, dtype, mutant, reverse)
    if dtype is np.float64 and not reverse:
        pre = np.einsum("nk,bkyx->bnyx", w1, p)
    else:
        pre = _dot(w1, p, dtype, reverse)
    if mutant != "no_bias":
        pre = pre + b1[None, :, None, None]
    hid = pre if mutant == "relu_after_w2" else np.maximum(pre, 0)
    if dtype is np.float64 and not reverse:
        y = np.einsum("cn,bnyx->bcyx", w2, hid)
    else:
        y = _dot(w2, hid, dtype, reverse)
    if mutant == "relu_after_w2":
        y = np.maximum(y, 0)
    m = mask_of(u, rate).astype(dtype)[:, None]
    if mutant == "mask_per_channel":      # a different draw per channel: the pixel's draws of its row neighbours
        m = np.stack([np.roll(m[:, 0], c, axis=-1) for c in range(x.shape[1])], 1)
    out = (x + y) * m if mutant == "mask_on_sum" else x + y * m
    if bound is None:
        return out
    assert dtype is np.float64 and mutant is None
    dx = np.broadcast_to(np.asarray(bound, dtype=np.float64), x.shape)
    a1, a2 = np.abs(w1), np.abs(w2)
    k1, nh = w1.shape[1], w1.shape[0]
    extra = 2.0 ** -16 if split else 0.0
    dp = _abs_perception(dx) + 9 * EPS * _abs_perception(x)
    sum1 = np.einsum("nk,bkyx->bnyx", a1, np.abs(p))
    dh = np.einsum("nk,bkyx->bnyx", a1, dp) + (k1 + 1) * EPS * (sum1 + np.abs(b1)[None, :, None, None]) + extra * sum1
    sum2 = np.einsum("cn,bnyx->bcyx", a2, np.abs(hid))
    dy = np.einsum("cn,bnyx->bcyx", a2, dh) + nh * EPS * sum2 + extra * sum2
    return out, dx + m * dy + EPS * np.abs(out) + m * EPS * np.abs(y)


def steps(x, w1, b1, w2, u, rate=0.5, keep=False, **kw):
    """u [n, B, H, W]: n updates; keep: every state, [n + 1, B, C, H, W]"""
    xs = [np.asarray(x, dtype=kw.get("dtype", np.float64))]
    for t in range(len(u)):
        xs.append(step(xs[-1], w1, b1, w2, u[t], rate, **kw))
    return np.stack(xs) if keep else xs[-1]


def steps_bound(x, w1, b1, w2, u, rate=0.5, split=False):
    """(x_n, bound) of n float32 updates from an exactly known x"""
    x, dx = np.asarray(x, dtype=np.float64), 0.0
    for t in range(len(u)):
        x, dx = step(x, w1, b1, w2, u[t], rate, bound=dx, split=split)
    return x, dx


def window_step(x, w1, b1, w2, u, col0, w_sub, margin, rate=0.5, mutant=None, **kw):
    """Window mode on the full grid x [B, C, H, W]: columns [col0, col0 + w_sub) are a torus, the window's columns [margin, w_sub - margin) are
    written back.  u (and a rate map) are laid out like the full rows.  Returns the new full grid."""
    x = np.array(x, dtype=kw.get("dtype", np.float64))
    sl = slice(col0, col0 + w_sub)
    rate_w = rate[..., sl] if np.ndim(rate) else rate
    if mutant == "window_full_torus":
        new = step(x, w1, b1, w2, u, rate, **kw)[..., sl]
    else:
        new = step(x[..., sl], w1, b1, w2, np.asarray(u)[..., sl], rate_w, mutant=mutant if mutant not in MUTANTS[-2:] else None, **kw)
    lo, hi = (0, w_sub) if mutant == "window_no_margin" else (margin, w_sub - margin)
    x[..., col0 + lo:col0 + hi] = new[..., lo:hi]
    return x


# the window calls of the exact-family window test on a 12-column grid: two overlapping windows that keep a one-column margin (the second
# sees the first one's fresh column), then one without a margin, whose edge columns show which torus the stencil wrapped on
WINDOWS = ((0, 7, 1), (5, 7, 1), (2, 6, 0))


def window_rounds(x, w1, b1, w2, u, windows=WINDOWS, rate=0.5, mutant=None, **kw):
    """one window_step per entry of windows, in order, on full-row uniforms u [len(windows), B, H, W]"""
    for i, (col0, w_sub, margin) in enumerate(windows):
        x = window_step(x, w1, b1, w2, u[i], col0, w_sub, margin, rate, mutant=mutant, **kw)
    return x


def adjoint_perception(gp, absolute=False):
    """[B, 4 C, H, W] -> [B, C, H, W]: sum_f sum_taps F_f[dy][dx] gp[4 c + f][y - dy][x - dx], the stencils with flipped taps"""
    gp = np.asarray(gp, dtype=np.float64)
    b, k, h, w = gp.shape
    q = gp.reshape(b, k // 4, 4, h, w)
    out = np.zeros((b, k // 4, h, w))
    for fi, f in enumerate(filters()):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                t = abs(f[dy + 1, dx + 1]) if absolute else f[dy + 1, dx + 1]
                if t != 0:
                    out += t * _shift(q[:, :, fi], -dy, -dx, False)
    return out


def vjp(states, w1, b1, w2, u, g_last, rate=0.5, bound=False, g_err=None):
    """The gradient of len(u) updates through states [n + 1, B, C, H, W] (exact inputs: the states the device stored): returns
    (g_first, dw1, db1, dw2), and with bound=True their element-wise float32 bounds as a second tuple.  The bound charges every sum of n
    terms n * 2^-24 * sum|terms| in any order (the parameter gradients: n = pixels x steps), carries each stage's error through the later
    ones, and lets every ReLU whose pre-activation lies inside its own float32 error go either way.  g_err: the element-wise error g_last
    arrives with (0 when it is exactly known)."""
    w1, b1, w2 = (np.asarray(a, dtype=np.float64) for a in (w1, b1, w2))
    a1, a2 = np.abs(w1), np.abs(w2)
    g = np.asarray(g_last, dtype=np.float64)
    dg = np.zeros_like(g) if g_err is None else np.array(g_err, dtype=np.float64)
    dw1, db1, dw2 = np.zeros_like(w1), np.zeros_like(b1), np.zeros_like(w2)
    e1, eb, e2 = np.zeros_like(w1), np.zeros_like(b1), np.zeros_like(w2)        # propagated errors
    s1, sb, s2 = np.zeros_like(w1), np.zeros_like(b1), np.zeros_like(w2)        # sum |terms|
    n_steps = len(u)
    k1, nh = w1.shape[1], w1.shape[0]
    for t in range(n_steps - 1, -1, -1):
        x = np.asarray(states[t], dtype=np.float64)
        p = perception(x)
        pre = np.einsum("nk,bkyx->bnyx", w1, p) + b1[None, :, None, None]
        hid = np.maximum(pre, 0)
        m = mask_of(u[t], rate).astype(np.float64)[:, None]
        gy = g * m
        dw2 += np.einsum("bcyx,bnyx->cn", gy, hid)
        v = np.einsum("cn,bcyx->bnyx", w2, gy)
        gh = v * (pre > 0)
        dw1 += np.einsum("bnyx,bkyx->nk", gh, p)
        db1 += gh.sum((0, 2, 3))
        gp = np.einsum("nk,bnyx->bkyx", w1, gh)
        if bound:
            dgy = dg * m
            dp = 9 * EPS * _abs_perception(x)
            dpre = np.einsum("nk,bkyx->bnyx", a1, dp) + (k1 + 1) * EPS * (np.einsum("nk,bkyx->bnyx", a1, np.abs(p)) + np.abs(b1)[None, :, None, None])
            unsure = np.abs(pre) <= dpre
            e2 += np.einsum("bcyx,bnyx->cn", dgy, hid) + np.einsum("bcyx,bnyx->cn", np.abs(gy), dpre)
            s2 += np.einsum("bcyx,bnyx->cn", np.abs(gy), hid)
            dv = np.einsum("cn,bcyx->bnyx", a2, dgy) + 16 * EPS * np.einsum("cn,bcyx->bnyx", a2, np.abs(gy))
            dgh = dv * ((pre > 0) | unsure) + unsure * np.abs(v)
            e1 += np.einsum("bnyx,bkyx->nk", dgh, np.abs(p)) + np.einsum("bnyx,bkyx->nk", np.abs(gh), dp)
            s1 += np.einsum("bnyx,bkyx->nk", np.abs(gh), np.abs(p))
            eb += dgh.sum((0, 2, 3))
            sb += np.abs(gh).sum((0, 2, 3))
            dgp = np.einsum("nk,bnyx->bkyx", a1, dgh) + nh * EPS * np.einsum("nk,bnyx->bkyx", a1, np.abs(gh))
            dg = dg + adjoint_perception(dgp, True) + 28 * EPS * (np.abs(g) + adjoint_perception(np.abs(gp), True))
        g = g + adjoint_perception(gp)
    if not bound:
        return g, dw1, db1, dw2
    n = n_steps * int(np.prod(np.asarray(states).shape[1:2])) * int(np.prod(np.asarray(states).shape[3:]))
    return (g, dw1, db1, dw2), (dg, e1 + n * EPS * s1, eb + n * EPS * sb, e2 + n * EPS * s2)


def vjp_magnitude(states, w1, b1, w2, u, g_last, rate=0.5):
    """The largest sum of |terms| any partial sum of vjp can reach: the same walk with every operand's magnitude (ReLU's mask kept)."""
    w1, b1, w2 = (np.asarray(a, dtype=np.float64) for a in (w1, b1, w2))
    a1, a2 = np.abs(w1), np.abs(w2)
    g = np.abs(np.asarray(g_last, dtype=np.float64))
    s1, sb, s2, top = np.zeros_like(w1), np.zeros_like(b1), np.zeros_like(w2), 0.0
    for t in range(len(u) - 1, -1, -1):
        x = np.asarray(states[t], dtype=np.float64)
        p = perception(x)
        pre = np.einsum("nk,bkyx->bnyx", w1, p) + b1[None, :, None, None]
        gy = g * mask_of(u[t], rate).astype(np.float64)[:, None]
        gh = np.einsum("cn,bcyx->bnyx", a2, gy) * (pre > 0)
        s2 += np.einsum("bcyx,bnyx->cn", gy, np.maximum(pre, 0))
        s1 += np.einsum("bnyx,bkyx->nk", gh, np.abs(p))
        sb += gh.sum((0, 2, 3))
        g = g + adjoint_perception(np.einsum("nk,bnyx->bkyx", a1, gh), True)
        top = max(top, float(g.max()), float(_abs_perception(x).max()))
    return max(top, float(s1.max()), float(sb.max()), float(s2.max()))


def params_from_seed(seed, chn=12, hidden=96):
    """The fixture's CA parameters (it stores the seed, not the values): w1 and b1 uniform in +-1 / sqrt(4 chn) as Conv2d draws them, w2
    N(0, 0.1^2) - the reference's zero w2 would make every step the identity."""
    rng = np.random.default_rng(seed)
    lim = 1.0 / np.sqrt(4 * chn)
    w1 = rng.uniform(-lim, lim, (hidden, 4 * chn)).astype(np.float32)
    b1 = rng.uniform(-lim, lim, hidden).astype(np.float32)
    w2 = (0.1 * rng.standard_normal((chn, hidden))).astype(np.float32)
    return w1, b1, w2


def load_g40(path):
    """tests/golden/g40_nca.npz with the parameter sets a_* and b_* rebuilt from their seeds"""
    z = np.load(path)
    g = {k: z[k] for k in z.files}
    for p in "ab":
        g[f"{p}_w1"], g[f"{p}_b1"], g[f"{p}_w2"] = params_from_seed(int(g[f"{p}_seed"]))
    g["v_g_last"] = np.zeros_like(g["v_x0"])          # dL/dx_3: stored on the RGB channels the loss reads, zero elsewhere
    g["v_g_last"][:, :3] = g["v_g_img"]
    return g


def unit23(words):
    return ((np.asarray(words, dtype=np.uint32) >> np.uint32(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)


def philox_u(seed, stream, t, b, h, w):
    """The library's in-kernel uniforms of step t: unit23 of words (t B H W) .. of the Philox stream (seed, stream), as [B, H, W]."""
    from oracle import rng
    n = b * h * w
    return unit23(rng.u32(seed, stream, n, offset=t * n)).reshape(b, h, w)


def to_u8(x):
    """tensor2bytes on value range (0, 1): [B, C, H, W] float -> [B, H, W, C] uint8, round half to even"""
    v = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return np.rint(v).astype(np.uint8).transpose(0, 2, 3, 1)


# ---- inputs on which every float32 evaluation, in any order and as hi + lo bf16 products, is exact --------------------------------------------

def exact_family(seed, b, c, h, w, hidden, n_steps, dense):
    """Integer state and parameters whose n_steps updates stay within 16 significant bits per operand and 24 per sum.

    dense (one step only): every w1 / w2 entry in {-2 .. 2}, every stencil in play, asymmetric - any wrong index changes a result.
    not dense: three +-1 entries per w1 row on identity and sobel features of a state in {-1, 0, 1} and two per w2 row, so that the state's
    growth over several steps stays inside the budget.  The budget is asserted here, on magnitudes, not assumed."""
    rng = np.random.default_rng(seed)
    k1 = 4 * c
    if dense:
        x = rng.integers(-3, 4, (b, c, h, w))
        w1 = rng.integers(-2, 3, (hidden, k1))
        w2 = rng.integers(-2, 3, (c, hidden))
        b1 = rng.integers(-40, 41, hidden)
    else:
        x = rng.integers(-1, 2, (b, c, h, w))
        w1 = np.zeros((hidden, k1), dtype=np.int64)
        w2 = np.zeros((c, hidden), dtype=np.int64)
        for n in range(hidden):
            cols = rng.choice(k1 // 4, 3, replace=False) * 4 + np.array([0, 0, rng.integers(1, 3)])
            w1[n, cols] = rng.choice([-1, 1], 3)
        for ch in range(c):
            w2[ch, rng.choice(hidden, 2, replace=False)] = rng.choice([-1, 1], 2)
        b1 = rng.integers(-2, 2, hidden)
    u = rng.random((n_steps, b, h, w), dtype=np.float32)
    xs = x.astype(np.float64)
    for t in range(n_steps):
        p = perception(xs)
        pre = np.einsum("nk,bkyx->bnyx", np.abs(w1).astype(np.float64), np.abs(p)) + np.abs(b1)[None, :, None, None]
        hid = np.maximum(np.einsum("nk,bkyx->bnyx", w1.astype(np.float64), p) + b1[None, :, None, None], 0)
        ysum = np.einsum("cn,bnyx->bcyx", np.abs(w2).astype(np.float64), hid)
        assert np.abs(p).max() < 2 ** 16 and hid.max() < 2 ** 16, "exact_family: an operand needs more than 16 bits"
        assert pre.max() < 2 ** 24 and (ysum + np.abs(xs)).max() < 2 ** 24, "exact_family: a sum needs more than 24 bits"
        xs = step(xs, w1, b1, w2, u[t])
    f = np.float32
    return x.astype(f), w1.astype(f), b1.astype(f), w2.astype(f), u


# (seed, B, chn, H, W, hidden, steps, dense) of exact_family: grids below a tile, across tiles with remainders, the three instantiation paths
EXACT_CASES = [(1, 1, 12, 3, 3, 96, 1, True), (2, 3, 12, 5, 7, 96, 1, True), (3, 1, 12, 20, 36, 96, 1, True), (4, 1, 12, 19, 70, 96, 1, True),
               (5, 1, 16, 5, 7, 128, 1, True), (6, 2, 4, 9, 33, 32, 1, True),
               (7, 1, 12, 3, 3, 96, 3, False), (8, 3, 12, 5, 7, 96, 5, False), (9, 1, 12, 20, 36, 96, 3, False), (10, 1, 12, 19, 70, 96, 5, False)]


def checkgrid_round(g40, mutant=None, dtype=np.float64):
    """one round of the two recorded models on their strips; the recorded uniforms are [model, 1, H, w + 2]: laid into full rows per call"""
    x, w = g40["g_x0"].astype(dtype), int(g40["g_w"])
    for ci, p in enumerate("ab"):
        u = np.zeros((1,) + x.shape[2:], dtype=np.float32)
        u[..., ci * w:ci * w + w + 2] = g40["g_u"][ci]
        x = window_step(x, g40[f"{p}_w1"], g40[f"{p}_b1"], g40[f"{p}_w2"], u, ci * w, w + 2, 1, mutant=mutant, dtype=dtype)
    return x


# ---- the batch-mean Gram loss on the VGG taps (train.py:122-142, 228-229) ---------------------------------------------------------------------
# The network arithmetic is tests/perceptor_ref.py's; this adds the head.  The fixture's style case runs the reference's own calc_styles /
# style_loss on a three-convolution stand-in for vgg16: calc_styles taps its hard-coded indices 1, 6, ..., which on
# [conv, ReLU, conv, ReLU, pool, conv, ReLU] are the first and the last ReLU: plan entries 0 and 3.

STYLE_PLAN = (64, 64, 0, 128)
STYLE_TAPS = (0, 3)
STYLE_SEED = 4040


def style_pre():
    import perceptor_ref as P
    return (1.0, 0.0, P.GAUSS_PRE[2], P.GAUSS_PRE[3])


def style_net(seed=STYLE_SEED):
    """the stand-in network from a seed (the fixture stores no weights): bf16-representable weights after the first convolution, so that
    one fixture serves the library's f32 and bf16 network modes; zero padding, in_mul 1, in_add 0, ImageNet mean / std"""
    import perceptor_ref as P
    return (list(STYLE_PLAN), P.gaussian_params(STYLE_PLAN, "bf16", seed), style_pre(), False)


def style_image(seed, B, H, W):
    """float32 values in [0, 1)"""
    return np.random.default_rng(seed).random((B, 3, H, W), dtype=np.float32).astype(np.float64)


def calc_styles(net, img, taps=STYLE_TAPS):
    """[G_b = F_b F_b^T / (h w)] per tap, [B, C, C]"""
    import perceptor_ref as P
    acts = P.forward(net, img)
    return [P.gram(acts[e]) / (acts[e].shape[2] * acts[e].shape[3]) for e in taps], acts


def gram_mean_head(F, T, mutant=None):
    """(L, dL/dF) of one tap: L = mean((mean_b G_b - T)^2), G_b = F_b F_b^T / (h w)"""
    import perceptor_ref as P
    B, C, h, w = F.shape
    hw = 1 if mutant == "gram_no_hw" else h * w
    G = P.gram(F) / hw
    if mutant == "mean_after_square":
        D = G - T[None]
        loss = (D * D).mean((1, 2)).mean()
        dG = 2 * D / (C * C * B * hw)
    else:
        D = G.mean(0) - T
        loss = (D * D).mean()
        dG = np.broadcast_to(2 * D / (C * C * B * hw), G.shape)
    sym = dG + dG.transpose(0, 2, 1)
    return loss, (sym @ F.reshape(B, C, -1)).reshape(F.shape)


def gram_mean_grad(net, img, targets, taps=STYLE_TAPS, mutant=None, acts=None):
    """(L, dL/d img): the restatement of maua_vgg_gram_mean_grad.  acts: activations to use instead of the float64 forward (the device's)"""
    import perceptor_ref as P
    acts = P.forward(net, img) if acts is None else acts
    loss, heads = 0.0, {}
    for e, T in zip(taps, targets):
        l, heads[e] = gram_mean_head(acts[e], T, mutant)
        loss += l
    return loss, P.backward(net, acts, heads)


def gram_mean_bounds(F, T, dt):
    """(bound of the tap's loss term, bound of the stored head gradient F Sym) following the head's launches in csrc/perceptor.hip:
    gram (perceptor_ref.gram_bound) -> s = sum_b G_b (B float32 additions) -> m = s * inv with inv = 1.f / (B h w) (two roundings) ->
    D = m - T (one) -> Sym = k (d1 + d2), k = 2.f / (C^2 B h w) (k: three roundings; the sum and the product: two), stored in the network
    type -> the head GEMM (C float32 terms, stored).  The loss: d^2 per element, a 256-lane block sum (6 shuffle additions + 4 wave sums),
    then ceil(blocks / 256) + 10 additions over the blocks, the product with 1 / C^2 and the += onto the loss: positive terms, relative."""
    import perceptor_ref as P
    V, U = P.V, P.U
    B, C, h, w = F.shape
    hw, CC = h * w, C * C
    G = P.gram(F)
    s = G.sum(0)
    es = P.gram_bound(F).sum(0) + B * V * np.abs(G).sum(0)
    inv = 1.0 / (B * hw)
    m = s * inv
    em = inv * es + 2 * V * np.abs(m)
    D = m - T
    eD = em + V * (np.abs(m) + np.abs(T))
    k = 2.0 / (CC * B * hw)
    sym = k * (D + D.T)
    esym = k * (eD + eD.T) + 5 * V * k * (np.abs(D) + np.abs(D.T))
    esym = esym * (1 + U[dt]) + U[dt] * np.abs(sym)
    f = np.abs(F).reshape(B, C, -1)
    hg = sym @ F.reshape(B, C, -1)
    ehg = esym @ f + C * V * ((np.abs(sym) + esym) @ f)
    ehg = ehg * (1 + 2 * U[dt]) + 2 * U[dt] * np.abs(hg)
    blocks = -(-CC // 256)
    ns = (2 + 10 + -(-blocks // 256) + 10 + 3) * V
    Q = (D * D).sum()
    eQ = (2 * np.abs(D) * eD + eD * eD).sum() + ns * Q
    return eQ / CC, ehg.reshape(F.shape)


def gram_mean_grad_bound(net, acts, targets, dt, taps=STYLE_TAPS):
    """(L, bound of L, dL/d img, its element-wise bound) on given stored activations"""
    import perceptor_ref as P
    loss, eloss, heads, hb = 0.0, 0.0, {}, {}
    for e, T in zip(taps, targets):
        l, heads[e] = gram_mean_head(acts[e], T)
        el, hb[e] = gram_mean_bounds(acts[e], T, dt)
        loss, eloss = loss + l, eloss + el
    grad, bound = P.backward_with_bound(net, acts, heads, hb, dt)
    return loss, eloss + (len(taps) + 1) * P.V * loss, grad, bound


# ---- one training iteration (train.py:221-236) -----------------------------------------------------------------------------------------------

def normalise(g):
    """train.py:233"""
    return g / (np.sqrt((g * g).sum()) + 1e-8)


def adam_first_step(p, g, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam's first step from zero moments, float64"""
    m, v = (1 - b1) * g, (1 - b2) * g * g
    return p - lr * (m / (1 - b1)) / (np.sqrt(v / (1 - b2)) + eps)


def adam_first_step_bound(p, g, eg, lr=1e-3, eps=1e-8):
    """|float32 Adam step on a gradient within eg of g - adam_first_step(p, g)|: the step is lr g / (|g| + eps), whose slope in g is
    lr eps / (|g| + eps)^2 (at most 2 lr in all where the sign is in doubt), plus a dozen float32 roundings on |p| + lr"""
    lo = np.maximum(np.abs(g) - eg, 0.0)
    return np.minimum(lr * eg * eps / (lo + eps) ** 2, 2 * lr) + 16 * EPS * (np.abs(p) + lr)


def normalise_bound(g, eg):
    """normalise() of a float32 gradient within eg of g: the norm's relative error is |eg| / |g| + (n + 4) 2^-24"""
    n = np.sqrt((g * g).sum())
    rel = np.sqrt((eg * eg).sum()) / n + (g.size + 4) * EPS
    return eg / n + np.abs(g) / n * rel


def _half(a):
    """float32 values with float16's significand: the fixture's inputs compress, and nothing about the arithmetic depends on it"""
    return np.asarray(a, dtype=np.float32).astype(np.float16).astype(np.float32)


def style_case(seed=STYLE_SEED + 1):
    """(x0 [2,12,16,16], u [3,2,16,16]) of the fixture's training-loss case"""
    rng = np.random.default_rng(seed)
    return _half(rng.standard_normal((2, 12, 16, 16))), _half(rng.random((3, 2, 16, 16)))


STYLE_TARGET_SCALE = (1000.0, 1800.0)


def style_targets(seed=STYLE_SEED + 2):
    """one float32 [C, C] target per tap of STYLE_PLAN, at the magnitude of the taps' Gram entries (any matrix is a valid target)"""
    rng = np.random.default_rng(seed)
    return [(s * rng.random((STYLE_PLAN[e], STYLE_PLAN[e]))).astype(np.float32) for e, s in zip(STYLE_TAPS, STYLE_TARGET_SCALE)]


def ca_init(seed, chn=12, hidden=96):
    """what maua_amd.nca.train starts from: torch's Conv2d initialisation of w1 under torch.manual_seed(seed), w2 zero (train.py:176-178)"""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        c1 = torch.nn.Conv2d(4 * chn, hidden, 1)
    return [c1.weight.detach().numpy().reshape(hidden, 4 * chn).astype(np.float64), c1.bias.detach().numpy().astype(np.float64),
            np.zeros((chn, hidden))]


def train_run(style_u8, lr, iters, seed=3, pool_size=8, batch=2, size=16, step_n=8, stop_above=None):
    """train.py:196-237 in float64 on the stand-in network, with maua_amd.nca.train's draws (numpy generator ``seed`` for the pool indices
    and step counts, Philox masks of stream (seed, 0)): the losses.  stop_above: leave once a loss exceeds it."""
    net = style_net()
    style = (np.float32(style_u8) / np.float32(255)).transpose(2, 0, 1)[None].astype(np.float64)
    targets = [g[0] for g in calc_styles(net, style)[0]]
    prm = ca_init(seed)
    m, v = [np.zeros_like(p) for p in prm], [np.zeros_like(p) for p in prm]
    pool, rng, t0, losses = np.zeros((pool_size, 12, size, size)), np.random.default_rng(seed), 0, []
    for i in range(iters):
        idx = rng.choice(pool_size, batch, replace=False)
        x = pool[idx].copy()
        if i % 32 == 0:
            x[:1] = 0
        n = int(rng.integers(step_n, step_n + 1))
        u = np.stack([philox_u(seed, 0, t0 + t, batch, size, size) for t in range(n)])
        t0 += n
        st = steps(x, *prm, u, keep=True)
        loss, dimg = gram_mean_grad(net, st[-1][:, :3], targets)
        gl = np.zeros_like(x)
        gl[:, :3] = dimg
        grads = vjp(st, *prm, u, gl)[1:]
        for k, g in enumerate(grads):
            g = normalise(g)
            m[k], v[k] = 0.9 * m[k] + 0.1 * g, 0.999 * v[k] + 0.001 * g * g
            prm[k] = prm[k] - lr * (m[k] / (1 - 0.9 ** (i + 1))) / (np.sqrt(v[k] / (1 - 0.999 ** (i + 1))) + 1e-8)
        pool[idx] = st[-1]
        losses.append(loss)
        if stop_above is not None and loss > stop_above:
            break
    return losses
