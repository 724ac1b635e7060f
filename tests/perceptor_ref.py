"""float64 restatement of csrc/perceptor.hip - the VGG / LPIPS perceptors' forward, their two loss heads and the hand-walked gradient -
for tests/test_perceptor_host.py (CPU) and tests/test_gpu_perceptor.py (device).  Plain numpy on [B][C][H][W] arrays; nothing here
is shared with the code under test or with torch's convolutions (the host test compares the two).

A network is (plan, params, pre, replicate): plan = channels per entry, 0 = MaxPool2d(2); params = [(w [Co][Ci][3][3], b [Co])] per
convolution; pre = (mul, add, mean[3], std[3]) - the first convolution sees ((img * mul + add) - mean_c) / std_c.

The backward walk takes the STORED activations: ReLU's mask and the pool's argmax are functions of them alone, so a walk fed the
activations read back from the device is the same linear map as the device's, whatever rounding the forward had.

The second half builds the exact family's operands (integers and dyadic numbers whose every partial sum is exact in float32) and the
element-wise error bounds of the Gaussian family, each read from the kernel it bounds (tests/test_gpu_perceptor.py lists them)."""
import numpy as np

V = 2.0 ** -24                                                  # float32 rounding unit
U = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8}                      # the storage type's
GRAM_PX = 256                                                   # pixels per slice of gram_partial
EPS_STYLE = float(np.float32(1e-8))
EPS_LPIPS = float(np.float32(1e-10))


# ---------------------------------------------------------------------------------------------------------------- the operators
def _pad(x, replicate):
    return np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode="edge" if replicate else "constant")


def conv3x3(x, w, b=None, replicate=False):
    """cross-correlation, padding 1 (zeros, or the edge pixel repeated)"""
    H, W = x.shape[2:]
    xp = _pad(x, replicate)
    out = np.zeros((x.shape[0], w.shape[0], H, W))
    for ky in range(3):
        for kx in range(3):
            out += np.einsum("bchw,oc->bohw", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx])
    return out if b is None else out + b.reshape(1, -1, 1, 1)


def conv3x3_adjoint(g, w):
    """the zero-padded convolution's adjoint: the convolution with the transposed, flipped kernel"""
    return conv3x3(g, np.ascontiguousarray(w.transpose(1, 0, 2, 3)[:, :, ::-1, ::-1]))


def pre_affine(img, pre):
    mul, add, mean, std = pre
    return ((img * mul + add) - np.asarray(mean, np.float64).reshape(1, 3, 1, 1)) / np.asarray(std, np.float64).reshape(1, 3, 1, 1)


def conv0(img, pre, w, b, replicate):
    return np.maximum(conv3x3(pre_affine(img, pre), w, b, replicate), 0.0)


def conv0_adjoint(g, w, factors, replicate):
    """d / d img of sum(g * conv(pad(affine(img)))): the gradient lands on the padded grid; with replicate padding a border pixel also
    collects what its virtual copies outside the image received (a corner: three of them); then the affine's mul / std_c."""
    B, _, H, W = g.shape
    gp = np.zeros((B, w.shape[1], H + 2, W + 2))
    for ky in range(3):
        for kx in range(3):
            gp[:, :, ky:ky + H, kx:kx + W] += np.einsum("bohw,oc->bchw", g, w[:, :, ky, kx])
    if replicate:
        gp[:, :, 1, :] += gp[:, :, 0, :]
        gp[:, :, H, :] += gp[:, :, H + 1, :]
        gp[:, :, :, 1] += gp[:, :, :, 0]
        gp[:, :, :, W] += gp[:, :, :, W + 1]
    return gp[:, :, 1:H + 1, 1:W + 1] * np.asarray(factors, np.float64).reshape(1, -1, 1, 1)


def vjp_factors(pre):
    """mul / std_c (the library forms in_mul * (1.f / std_c) in float32: two roundings, counted in the bound)"""
    mul, _, _, std = pre
    return [mul / s for s in std]


def _windows(x):
    B, C, H, W = x.shape
    return x.reshape(B, C, H // 2, 2, W // 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)   # q = dy * 2 + dx


def maxpool2(x):
    return _windows(x).max(-1)


def pool_argmax(x):
    """the FIRST maximal pixel of each window: row-major scan, replaced only by a strictly greater value"""
    v = _windows(x)
    a, m = np.zeros(v.shape[:-1], np.int64), v[..., 0].copy()
    for q in range(1, 4):
        up = v[..., q] > m
        m = np.where(up, v[..., q], m)
        a = np.where(up, q, a)
    return a


def maxpool2_adjoint(x, g):
    B, C, H, W = x.shape
    a = pool_argmax(x)
    out = np.zeros((B, C, H // 2, W // 2, 4))
    for q in range(4):
        out[..., q] = np.where(a == q, g, 0.0)
    return out.reshape(B, C, H // 2, W // 2, 2, 2).transpose(0, 1, 2, 4, 3, 5).reshape(B, C, H, W)


def gram(F):
    f = F.reshape(F.shape[0], F.shape[1], -1)
    return f @ f.transpose(0, 2, 1)


def style_head(F, T, strength, eps=1e-8):
    """loss[b] = strength sum D^2 / (sum |D| + eps) / numel with D = G_b - T_b; returns (loss, dL/dG, dL/dF = (dG + dG^T) F)"""
    G = gram(F)
    D = G - (T if T.ndim == 3 else T[None])
    Q, A = (D * D).sum((1, 2), keepdims=True), np.abs(D).sum((1, 2), keepdims=True) + eps
    n = D.shape[1] * D.shape[2]
    dG = strength * (2 * D * A - Q * np.sign(D)) / (A * A) / n
    sym = dG + dG.transpose(0, 2, 1)
    hg = (sym @ F.reshape(F.shape[0], F.shape[1], -1)).reshape(F.shape)
    return (strength * Q / A / n).reshape(-1), dG, hg


def lpips_normalize(F):
    r = np.sqrt((F * F).sum(1, keepdims=True))
    return F / (r + EPS_LPIPS)


def lpips_head(F, nt, lin, scale):
    """nt: unit-normalised target features [Bt][C][h][w].  val[b][p] = sum_c lin_c (n_c - nt_c)^2, dist[b] = mean_p val, and the gradient of
    scale * dist with respect to F through n = F / (|F| + eps); where |F| == 0 the projection term is 0 (the kernel's stated value)."""
    hw = F.shape[2] * F.shape[3]
    r = np.sqrt((F * F).sum(1, keepdims=True))
    re = r + EPS_LPIPS
    d = F / re - nt
    w = lin.reshape(1, -1, 1, 1)
    val = (w * d * d).sum(1)
    gv = 2 * w * d * (scale / hw)
    proj = (gv * F).sum(1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        k2 = np.where(r > 0, proj / (r * re * re), 0.0)
    return val, val.reshape(val.shape[0], -1).mean(1), gv / re - F * k2


def forward(net, img):
    """every plan entry's stored activation"""
    plan, params, pre, replicate = net
    acts, k = [], 0
    for i, c in enumerate(plan):
        if c == 0:
            acts.append(maxpool2(acts[-1]))
        elif i == 0:
            acts.append(conv0(img, pre, *params[0], replicate))
            k = 1
        else:
            acts.append(np.maximum(conv3x3(acts[-1], *params[k]), 0.0))
            k += 1
    return acts


def conv_of(plan):
    out, k = [], 0
    for c in plan:
        out.append(k if c else -1)
        k += 1 if c else 0
    return out


def backward(net, acts, heads, trace=None):
    """heads {plan entry: dL/d(its activation)} -> dL/d img.  At a convolution entry the head gradient and the gradient arriving from
    above are summed first, then masked by the stored activation > 0.  trace: a list that receives every intermediate the device
    stores in the network type (the masked sums and what each adjoint hands down)."""
    plan, params, pre, replicate = net
    ci = conv_of(plan)
    g = None
    for i in range(max(heads), -1, -1):
        if plan[i]:
            v = (0.0 if g is None else g) + heads.get(i, 0.0)
            gpre = np.where(acts[i] > 0, v, 0.0)
            if trace is not None:
                trace.append(gpre)
            if i == 0:
                return conv0_adjoint(gpre, params[0][0], vjp_factors(pre), replicate)
            g = conv3x3_adjoint(gpre, params[ci[i]][0])
        else:
            assert g is not None, "a pooling layer cannot be the deepest tap"
            g = maxpool2_adjoint(acts[i - 1], g)
        if trace is not None:
            trace.append(g)


# ---------------------------------------------------------------------------------------------------------------- storage types
def to_storage(a, dt):
    """float64 -> rounded to the storage type (round to nearest even), back in float64"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))
    return (t.to(torch.bfloat16) if dt == "bf16" else t.to(torch.float32)).double().numpy()


def representable(a, dt):
    return bool(np.array_equal(to_storage(a, dt), np.asarray(a, np.float64)))


def exact_sums(a_abs_sum, lsb):
    """every partial sum of terms that are multiples of `lsb`, with the absolute values summing to a_abs_sum, is exact in float32"""
    return float(np.max(a_abs_sum)) / lsb < 2.0 ** 24


# ---------------------------------------------------------------------------------------------------------------- exact family
EXACT_PRE = (0.5, 0.5, (0.5, 0.25, 0.75), (0.25, 0.5, 0.25))     # mul, add, mean dyadic; std powers of two
HEAD_SETS = {8: (2, -1, 1, -2, 1, 1), 4: (2, -1, 1), 2: (2,), 1: (1,)}   # sum |D0| -> the non-zero entries of D0


def exact_image(B, H, W, seed):
    """the image whose pre-processed value is a chosen integer in [-1, 1]: img = ((x' std + mean) - add) / mul, every step dyadic; from
    eight pixels on the top left 2 x 2 block is 0: with biases <= 0 the corner pixel is zero in every channel after ReLU"""
    rng = np.random.default_rng(seed)
    xp = rng.integers(-1, 2, size=(B, 3, H, W)).astype(np.float64)
    if H * W >= 8:
        xp[:, :, :2, :2] = 0
    mul, add, mean, std = EXACT_PRE
    img = ((xp * np.reshape(std, (1, 3, 1, 1)) + np.reshape(mean, (1, 3, 1, 1))) - add) / mul
    assert np.array_equal(pre_affine(img, EXACT_PRE), xp)
    return img, xp


def exact_params(plan, seed):
    """integer weights in {-1, 0, 1} (one in eight for the first convolution, one in sixty-four after it) and biases in [-1, 0]: negative
    pre-activations everywhere, whole pixels zero after ReLU, activations small integers full of ties"""
    rng = np.random.default_rng(seed + 1000)
    params, cin = [], 3
    for c in plan:
        if c == 0:
            continue
        p = 1 / 8 if cin == 3 else 1 / 64
        w = rng.integers(-1, 2, size=(c, cin, 3, 3)) * (rng.random((c, cin, 3, 3)) < (3 * p / 2))
        b = rng.integers(-1, 1, size=(c,))
        params.append((w.astype(np.float64), b.astype(np.float64)))
        cin = c
    return params


def exact_d0(F, total, seed, per_sample=True):
    """non-symmetric integer matrices, mostly zero, sum |D0| == total (a power of two): the entries of HEAD_SETS[total] at random
    places (rows and columns among channels that are alive), the second at the transposed place of the first (Sym adds the two)"""
    rng = np.random.default_rng(seed + 2000)
    vals = HEAD_SETS[total]
    B, C = F.shape[:2]
    out = np.zeros((B if per_sample else 1, C, C))
    for b, d in enumerate(out):
        # among the channels alive at the sample's busiest pixel where there are enough of them: F Sym is then not all masked away
        alive = (F[b] > 0).reshape(C, -1)
        ch = np.flatnonzero(alive[:, alive.sum(0).argmax()])
        ch = ch if len(ch) >= 4 else np.arange(C)
        while True:
            d[:] = 0
            r, c = rng.choice(ch, len(vals)), rng.choice(ch, len(vals))
            if len(vals) > 1:
                r[1], c[1] = c[0], r[0]
            if len(vals) > 2:
                c[-1] = r[-1]                                     # one entry on the diagonal: Sym doubles it
            if len(set(zip(r.tolist(), c.tolist()))) < len(vals) or (r[:2] == c[:2]).any():
                continue
            d[r, c] = vals
            if not np.array_equal(d, d.T):
                break
    return out


def exact_style(F, d0, strength):
    """The style head on integer features with target T = G - D0, as float32 computes it: A0 = sum |D0| is a power of two >= 1, so
    A0 + 1e-8f == A0; Q an integer; k = strength / C^2 a power of two.  Returns (T, loss, Sym, hg) - all exact dyadic numbers."""
    C = F.shape[1]
    G = gram(F)
    d = np.broadcast_to(d0, G.shape)
    A = np.abs(d).sum((1, 2), keepdims=True)
    Q = (d * d).sum((1, 2), keepdims=True)
    assert all(float(np.float32(a) + np.float32(1e-8)) == a and np.log2(a) % 1 == 0 and a >= 1 for a in A.reshape(-1))
    k = float(np.float32(strength) / np.float32(C * C))
    assert np.log2(k) % 1 == 0
    sym = k * ((2 * d * A - Q * np.sign(d)) + (2 * d.transpose(0, 2, 1) * A - Q * np.sign(d.transpose(0, 2, 1)))) / (A * A)
    hg = (sym @ F.reshape(F.shape[0], C, -1)).reshape(F.shape)
    return G - d0, (k * Q / A).reshape(-1), sym, hg


def _lsb(a, kmax=30):
    """smallest k with a * 2^k integer-valued everywhere"""
    for k in range(kmax):
        v = np.asarray(a) * 2.0 ** k
        if np.array_equal(v, np.round(v)):
            return k
    raise AssertionError("not dyadic")


def exact_case(case):
    """Everything an exact case needs, in float64: (plan, B, H, W, replicate, [(tap entry, sum |D0|, per-sample target)], seed) ->
    image, network, stored activations, targets, expected loss and image gradient, and `stored`: every value the device keeps in the
    network type on the way, each with the magnitude sum that bounds its partial sums ([(name, values, sum of |terms|)])."""
    plan, B, H, W, replicate, taps, seed = case[:7]
    if len(case) == 7:                                           # the first seed of seed, seed + 7919, ... whose gradient is not all zero
        for k in range(16):
            d = exact_case(case[:6] + (seed + 7919 * k, None))
            if np.abs(d["grad"]).max() > 0:
                return d
        raise AssertionError("no seed gives a gradient")
    img, _ = exact_image(B, H, W, seed)
    if B > 1 and not all(t[2] for t in taps):
        img[:] = img[:1]                                         # a shared target T = G - D0 needs one G
    params = exact_params(plan, seed)
    net = (list(plan), params, EXACT_PRE, replicate)
    acts = forward(net, img)
    ci = conv_of(plan)
    stored = []
    for i, c in enumerate(plan):
        if c and i == 0:
            stored.append((f"act{i}", acts[i], conv3x3(np.abs(pre_affine(img, EXACT_PRE)), np.abs(params[0][0]), np.abs(params[0][1]), replicate)))
        elif c:
            stored.append((f"act{i}", acts[i], conv3x3(np.abs(acts[i - 1]), np.abs(params[ci[i]][0]), np.abs(params[ci[i]][1]))))
    strength = float(plan[taps[0][0]] ** 2)
    heads, targets, loss = {}, [], np.zeros(B)
    for k, (entry, total, per_sample) in enumerate(taps):
        F = acts[entry]
        d0 = exact_d0(F, total, seed + 17 * k, per_sample)
        T, l, sym, hg = exact_style(F, d0, strength)
        targets.append(T if per_sample else T[0])
        heads[entry] = hg
        loss += l
        f = np.abs(F).reshape(B, plan[entry], -1)
        stored += [(f"gram{entry}", gram(F), gram(np.abs(F))), (f"sym{entry}", sym, np.abs(sym)),
                   (f"hg{entry}", hg, (np.abs(sym) @ f).reshape(F.shape))]
    trace, mags = [], []
    grad = backward(net, acts, heads, trace)
    backward((net[0], [(np.abs(w), b) for w, b in params], net[2], replicate), acts, {k: np.abs(v) for k, v in heads.items()}, mags)
    stored += [(f"walk{j}", t, m) for j, (t, m) in enumerate(zip(trace, mags))]
    gmag = backward((net[0], [(np.abs(w), b) for w, b in params], net[2], replicate), acts, {k: np.abs(v) for k, v in heads.items()})
    return dict(img=img, net=net, acts=acts, taps=[t[0] for t in taps], targets=targets, strength=strength, loss=loss, grad=grad,
                grad_mag=gmag, stored=stored, heads=heads)


def exact_premises(data, dt):
    """None when torch.equal may be trusted for this case in this storage type, else what fails: every stored value representable,
    every partial sum (bounded by the sum of the absolute terms) below 2^24 units of the values' last bit"""
    for name, val, mag in data["stored"] + [("grad", data["grad"], data["grad_mag"])]:
        k = _lsb(val)
        if float(np.max(mag)) * 2.0 ** k >= 2.0 ** 24:
            return f"{name}: partial sums reach 2^24 units of 2^-{k}"
        if name != "grad" and not name.startswith("gram") and not representable(val, dt):
            return f"{name}: not representable in {dt}"
    return None


def _conv0_cases():
    out, seed = [], 40
    for C in (64, 128):
        for rep in (0, 1):
            for (H, W) in ((1, 1), (1, 7), (3, 5), (9, 17)):
                for B in (1, 3):
                    seed += 1
                    out.append(((C,), B, H, W, rep, [(0, (8, 4, 2, 1)[seed % 4], bool(seed % 2) or B == 1)], seed))
    return out


CONV0_CASES = _conv0_cases()                                     # vgg_conv0, vgg_conv0_vjp64 (Co = 64) and vgg_conv0_vjp (Co = 128)
POOL_CASES = [((C, 0, C), B, H, W, 1, [(2, A, ps)], 100 + j) for j, (C, B, H, W, A, ps) in enumerate(
    [(64, 1, 2, 2, 8, True), (64, 3, 6, 10, 4, True), (64, 2, 16, 32, 8, False), (128, 1, 2, 2, 4, True), (128, 2, 6, 10, 8, True),
     (128, 1, 16, 32, 2, True)])]
# mask_add: the deepest tap has no gradient from above (every case); (64, 64) with its one tap at entry 1: entry 0 has no head
# gradient; (64, 64, "M", 64, 64) with taps at entries 1 and 4: both, and five layers of the ga / gb ping-pong
MASK_CASES = [((64, 64), 2, 3, 5, 0, [(1, 8, True)], 200), ((64, 64, 0, 64, 64), 2, 4, 6, 1, [(1, 2, True), (4, 1, True)], 201),
              ((64, 64, 0, 64, 64), 3, 8, 12, 0, [(1, 1, False), (4, 2, False)], 202), ((128, 128), 1, 2, 2, 1, [(0, 4, True), (1, 8, True)], 203)]
EXACT_CASES = CONV0_CASES + POOL_CASES + MASK_CASES
# cases whose stored intermediates do not all fit bf16's eight bits run in f32 only (the Gaussian family covers them in bf16)
EXACT_F32_ONLY = set()


def tie_patterns(x):
    """which sets of window positions hold the maximum: a 4-bit mask per window"""
    v = _windows(x)
    m = v.max(-1, keepdims=True)
    return ((v == m) * np.array([1, 2, 4, 8])).sum(-1)


# ---------------------------------------------------------------------------------------------------------------- Gaussian family
def gaussian_image(B, H, W, seed):
    return np.random.default_rng(seed).normal(size=(B, 3, H, W)).astype(np.float32).astype(np.float64)


def gaussian_params(plan, dt, seed):
    """He-scaled Gaussian weights rounded to what stores them: float32 for the first convolution (the direct kernel), the network type
    after it; float32 biases"""
    rng = np.random.default_rng(seed + 3000)
    params, cin = [], 3
    for c in plan:
        if c == 0:
            continue
        w = rng.normal(size=(c, cin, 3, 3)) * np.sqrt(2.0 / (cin * 9))
        b = rng.normal(size=(c,)) * 0.05
        params.append((to_storage(w, "f32" if cin == 3 else dt), to_storage(b, "f32")))
        cin = c
    return params


GAUSS_PRE = (0.5, 0.5, tuple(float(np.float32(m)) for m in (0.485, 0.456, 0.406)), tuple(float(np.float32(s)) for s in (0.229, 0.224, 0.225)))


def conv0_bound(img, pre, w, b, replicate, ref, dt):
    """x' = (img mul + add - mean) istd: three float32 operations (contracted or not) on terms of size |img mul|, |add|, |mean|, and
    istd = 1.f / std against the reference's division: 4 v (|img mul| + |add| + |mean|) / std.  Then 27 products and 27 additions onto
    the bias in float32, ReLU (1-Lipschitz), the store."""
    mul, add, mean, std = pre
    s = np.reshape(std, (1, 3, 1, 1))
    ex = 4 * V * (np.abs(img * mul) + abs(add) + np.abs(np.reshape(mean, (1, 3, 1, 1)))) / s
    mag = conv3x3(np.abs(pre_affine(img, pre)), np.abs(w), np.abs(b), replicate)
    return conv3x3(ex, np.abs(w), None, replicate) + 28 * V * mag + 2 * U[dt] * np.abs(ref)


def conv_bound(x, w, b, ref, dt):
    """tests/test_gpu_modconv.py's bound at unit styles (x * 1 is exact: no operand rounding, n = 0): 2 u |ref| + 9 Ci 2^-24 A"""
    return 2 * U[dt] * np.abs(ref) + 9 * w.shape[1] * V * conv3x3(np.abs(x), np.abs(w), np.abs(b))


def gram_bound(F):
    """gram_partial: float32 products and a running sum of at most 256 of them per slice; gram_reduce adds the S slices in order"""
    hw = F.shape[2] * F.shape[3]
    S = -(-hw // GRAM_PX)
    return (min(hw, GRAM_PX) + S) * V * gram(np.abs(F))


def norm_bound(F):
    """lpips_norm / lpips_head's r: C / 64 terms per lane and six shuffle additions (positive terms: relative (C / 64 + 7) v), a
    square root (halves it, + v), + 1e-10f (v), the division (v)"""
    per = F.shape[1] // 64
    return ((per + 7) / 2 + 3) * V


def lpips_bounds(F, nt, lin, scale, dt):
    """(bound of val, bound of dist, bound of the stored head gradient), from lpips_head_kernel and rows_sum_kernel line by line"""
    hw = F.shape[2] * F.shape[3]
    per = F.shape[1] // 64
    kr = norm_bound(F)                                           # relative error of re and of n
    r = np.sqrt((F * F).sum(1, keepdims=True))
    re = r + EPS_LPIPS
    n = F / re
    d = n - nt
    w = np.abs(lin).reshape(1, -1, 1, 1)
    ed = kr * np.abs(n) + V * np.abs(d)
    eval_ = (w * (2 * np.abs(d) * ed + 3 * V * d * d)).sum(1) + (per + 7) * V * (w * d * d).sum(1)
    val = (w * d * d).sum(1)
    runs = -(-hw // 1024) + 6 + 16 + 3                           # a thread's run, the wave's shuffles, the 16 wave sums, mul, +=
    edist = eval_.reshape(F.shape[0], -1).sum(1) / hw + runs * V * val.reshape(F.shape[0], -1).sum(1) / hw
    coef = scale / hw
    gv = 2 * w * np.abs(d) * coef
    egv = 2 * w * coef * ed + 4 * V * gv
    proj_mag = (gv * np.abs(F)).sum(1, keepdims=True)
    eproj = (egv * np.abs(F)).sum(1, keepdims=True) + (per + 8) * V * proj_mag
    _, _, hg = lpips_head(F, nt, lin, scale)
    with np.errstate(divide="ignore", invalid="ignore"):
        den = r * re * re
        k2 = np.where(r > 0, (2 * lin.reshape(1, -1, 1, 1) * d * coef * F).sum(1, keepdims=True) / den, 0.0)
        ek2 = np.where(r > 0, eproj / den + np.abs(k2) * (3 * kr + 4 * V), 0.0)
    e = egv / re + gv / re * (kr + 2 * V) + np.abs(F) * ek2 + 2 * V * np.abs(F * k2) + V * np.abs(hg)
    return eval_, edist, e * (1 + 2 * U[dt]) + 2 * U[dt] * np.abs(hg)


def style_bounds(F, T, strength, dt):
    """(bound of the loss, bound of the stored head gradient F Sym), following the head's launches:
    gram (gram_bound) -> D = G - T (v) -> Q = sum D^2, A = sum |D| (float32 runs of CC / 64 / 256 terms, a block sum, 64 chunk sums;
    positive terms: relative n_s v) -> Sym = k (2 D A - Q sign D + transposed) / A^2, about eight float32 operations, stored in the
    network type; where |D| is inside its own error the sign may differ: k Q / A^2 more -> the head GEMM (C terms in float32, stored)."""
    B, C = F.shape[:2]
    CC = C * C
    G = gram(F)
    D = G - (T if T.ndim == 3 else T[None])
    eD = gram_bound(F) + V * (np.abs(G) + np.abs(T if T.ndim == 3 else T[None]))
    ns = (-(-CC // 64 // 256) + 1 + 6 + 4 + 64 + 2) * V
    Q, A = (D * D).sum((1, 2), keepdims=True), np.abs(D).sum((1, 2), keepdims=True) + EPS_STYLE
    eQ = (2 * np.abs(D) * eD + eD * eD).sum((1, 2), keepdims=True) + ns * Q
    eA = eD.sum((1, 2), keepdims=True) + ns * A
    k = strength / CC
    loss = (k * Q / A).reshape(-1)
    eloss = (k * (eQ / A + Q * eA / (A * A)) + 4 * V * k * Q / A).reshape(-1)
    dG = k * (2 * D * A - Q * np.sign(D)) / (A * A)
    edG = k * (2 * (eD * A + np.abs(D) * eA) + eQ) / (A * A) + 2 * np.abs(dG) * eA / A + k * np.where(np.abs(D) <= eD, 2 * Q / (A * A), 0.0)
    mag = k * (2 * np.abs(D) * A + Q) / (A * A)
    sym = dG + dG.transpose(0, 2, 1)
    esym = edG + edG.transpose(0, 2, 1) + 8 * V * (mag + mag.transpose(0, 2, 1))
    esym = esym * (1 + U[dt]) + U[dt] * np.abs(sym)
    f = np.abs(F).reshape(B, C, -1)
    hg = sym @ F.reshape(B, C, -1)
    ehg = esym @ f + C * V * ((np.abs(sym) + esym) @ f)
    ehg = ehg * (1 + 2 * U[dt]) + 2 * U[dt] * np.abs(hg)
    return loss, eloss, ehg.reshape(F.shape)


def backward_with_bound(net, acts, heads, head_bounds, dt):
    """backward() and the element-wise bound of the device's walk against it, layer by layer (u = the storage unit):
      mask_add      v = g + hg: one float32 addition, the store: e = e_g + e_hg + 2 u (|v| + e)
      pool adjoint  routes the value and its error, no arithmetic
      transposed convolution (the MFMA kernel)   |W^T| e + 9 Ci v |W^T| (|g| + e), + 2 u |out|
      conv0 adjoint a float32 run of n products: t (virtual pixel, tap) pairs reach the pixel - 9 inside, fewer at a zero-padded
                    border, up to 36 at a corner that replicate padding folds -; the generic kernel runs over all t Co, the
                    64-channel kernel over 8 t per lane and three shuffle additions.  Then the factor in_mul * (1.f / std) (two
                    roundings) and the product with it: f |W0^T| e + (n + 2) v f |W0^T| (|g| + e) + 4 v |out|"""
    plan, params, pre, replicate = net
    ci = conv_of(plan)
    u = U[dt]
    g, e = None, None
    for i in range(max(heads), -1, -1):
        if plan[i]:
            v = (0.0 if g is None else g) + heads.get(i, 0.0)
            ev = (0.0 if e is None else e) + head_bounds.get(i, 0.0)
            n_in = (g is not None) + (i in heads)
            if n_in == 2:
                ev = ev + 2 * u * (np.abs(v) + ev)
            m = acts[i] > 0
            gpre, epre = np.where(m, v, 0.0), np.where(m, ev, 0.0)
            if i == 0:
                w, fac = params[0][0], vjp_factors(pre)
                out = conv0_adjoint(gpre, w, fac, replicate)
                mag = conv0_adjoint(np.abs(gpre) + epre, np.abs(w), fac, replicate)
                t = conv0_adjoint(np.ones((1, 1) + out.shape[2:]), np.ones((1, 1, 3, 3)), (1.0,), replicate)
                n = 8 * t + 3 if w.shape[0] == 64 else w.shape[0] * t
                return out, conv0_adjoint(epre, np.abs(w), fac, replicate) + (n + 2) * V * mag + 4 * V * np.abs(out)
            w = params[ci[i]][0]
            g = conv3x3_adjoint(gpre, w)
            e = (conv3x3_adjoint(epre, np.abs(w)) + 9 * w.shape[0] * V * conv3x3_adjoint(np.abs(gpre) + epre, np.abs(w))) * (1 + 2 * u) + 2 * u * np.abs(g)
        else:
            g, e = maxpool2_adjoint(acts[i - 1], g), maxpool2_adjoint(acts[i - 1], e)


def region_masks(H, W):
    """corner / edge / interior pixels of an H x W image (what a failure message names separately)"""
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    by, bx = (yy == 0) | (yy == H - 1), (xx == 0) | (xx == W - 1)
    return {"corner": by & bx, "edge": (by | bx) & ~(by & bx), "interior": ~(by | bx)}
