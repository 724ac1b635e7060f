"""The twin of the beat tracker and segmentation kernels (csrc/segment.hip), in plain numpy: for each of its 6 entry points the result
written from the formula in include/maua_hip.h and the kernels' header comments - float64 where values are computed, a float32
restatement where the operation order is the contract (segment_reduce's sequential mean, the distances of recurrence_affinity, the
reduction order of soft_kmeans), integers where the output is an index - and the bounds of the families that are not exact.  The
inputs of tests/test_segment_host.py and tests/test_gpu_segment_kernels.py are generated here.  The host test holds this file against
scipy.signal.convolve, torch.median, oracle/segment.py and the pad / roll / median / roll / crop written literally, proves the
preconditions of the exact families and shows that the comparisons reject off-by-one mutants (the `mutant=` arguments).

v = 2^-24 (half a unit in the last place of float32), u = 2^-53."""
import numpy as np

V = 2.0 ** -24
U = 2.0 ** -53
TINY = float(np.finfo(np.float32).tiny)


def f32(a):
    return np.asarray(a, dtype=np.float32)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def measured_dev(fn32, fn64, args, relative=True):
    """the project's convention for a device library function: the float32 CPU function against float64 over the case's own
    arguments; 4 x the largest deviation is what a bound may allow"""
    a32 = [f32(a) for a in args]
    with np.errstate(all="ignore"):
        got = f64(fn32(*a32))
        want = fn64(*[f64(a) for a in a32])
    ok = np.isfinite(want) & np.isfinite(got) & (np.abs(want) >= TINY)
    err = np.abs(got - want)[ok]
    if relative:
        err = err / np.abs(want[ok])
    return float(err.max()) if err.size else 0.0


def lower_median(x, axis, mutant=None):
    """torch.median: the lower of the two middle values of an even count"""
    s = np.sort(x, axis=axis)
    n = s.shape[axis]
    return np.take(s, n // 2 if mutant == "upper" else (n - 1) // 2, axis=axis)


def reflect_index(i, n, mutant=None):
    """F.pad(mode="reflect"): no edge repeat"""
    i = np.asarray(i)
    if mutant == "edge_repeat":
        return np.where(i < 0, -i - 1, np.where(i >= n, 2 * n - 1 - i, i))
    return np.where(i < 0, -i, np.where(i >= n, 2 * (n - 1) - i, i))


# ----------------------------------------------------------------------------------------------------------------- beat tracker
BEAT_PERIODS = (1, 2, 7, 2047)
BEAT_KINDS = ("random", "zeros", "constant", "clicks")
BEAT_MAX_PERIOD = 2047                                  # 2 period + 2 <= 4096, the ring of cumulative scores


def beat_T(period):
    return sorted({1, 2, period, 5000})


def beat_kinds(T, period):
    """every kind, but for the constant envelope over 5000 frames at period 2047: on its plateau the best predecessor is the top of
    a smooth curve sampled on the integers, and every other frame has two candidates within 1e-13 of each other - a third of the
    frames would sit below the margin that decides which links may be compared (tests/test_segment_host.py holds the others to 1 %)"""
    return tuple(k for k in BEAT_KINDS if not (k == "constant" and period == 2047 and T == 5000))


def beat_tables(period, tightness):
    """(smoothing window [2 period + 1], predecessor offsets, their log-time penalties) as librosa and the library's host code compute
    them: every operation but exp and log is a single IEEE operation on the same operands on both sides"""
    a = np.arange(-period, period + 1) * 32.0 / period
    gw = np.exp(-0.5 * (a * a))
    half = int(np.rint(period / 2.0))                   # round half to even, like numpy
    offsets = np.arange(-2 * period, -half + 1)
    with np.errstate(divide="ignore"):
        lg = np.log(-offsets.astype(np.float64) / period)   # period 1: the offset 0 gives log(0) = -inf, a candidate that never wins
        txwt = -tightness * (lg * lg)
    return gw, offsets, txwt


def beat_localscore(env, period):
    """(localscore, bound): scipy.signal.convolve(env, window, "same") in float64.  Bound: the window's exp on both sides within one
    ulp of the true value (4 u between them), a product and at most 2 period + 1 additions: (2 period + 6) u sum |env| |window|"""
    env = f64(env)
    gw = beat_tables(period, 1.0)[0]
    T = env.size
    ls = np.convolve(env, gw, "full")[period:period + T]
    mag = np.convolve(np.abs(env), gw, "full")[period:period + T]
    return ls, (2 * period + 6) * U * mag


def beat_dp(localscore, period, tightness, mutant=None):
    """The dynamic program on a given localscore -> dict(cumscore, backlink, err, safe).  Frame i scores its predecessors
    i + offsets with txwt + cumscore[prev] (txwt alone before time 0), takes the first maximum, links to it; frames before the first
    one whose localscore reaches 1 % of the maximum link to -1.

    err[i] bounds |cumscore - this| for an implementation whose log is within one ulp: a candidate carries its predecessor's err, 12 u
    |txwt| (the two logs 4 u apart, squared, times the tightness) and u of itself for the sum; the maximum of candidates that each
    moved by at most e moves by at most e; + u |cumscore| for the last sum.  The two sums are single IEEE additions: on operands
    that carry no error they give the same bits on both sides, so their u is charged only where an error arrives.  safe[i]: the best
    candidate leads the second best by more than twice the largest candidate error, so no such implementation can link elsewhere -
    or no candidate carries any error at all (every txwt a zero: BEAT_TIE_TIGHTNESS), and then the candidates are the same bits and
    the link, an exact tie included, is decided by the rule "first maximum" alone."""
    ls = f64(localscore)
    T = ls.size
    _, offsets, txwt = beat_tables(period, tightness)
    fin = np.isfinite(txwt)
    d_tx = np.where(fin, 12 * U * np.abs(np.where(fin, txwt, 0.0)), 0.0)
    cum, err = np.zeros(T), np.zeros(T)
    back = np.zeros(T, np.int64)
    safe = np.zeros(T, bool)
    small = 0.01 * ls.max()
    first = True
    for i in range(T):
        prev = offsets + i
        ok = (prev >= 0) & (prev < i)
        cand = txwt.copy()
        cand[ok] += cum[prev[ok]]
        ce = d_tx.copy()
        ce[ok] += err[prev[ok]]
        ce = ce + np.where(ce > 0, U * np.abs(np.where(fin, cand, 0.0)), 0.0)
        j = int(np.argmax(cand)) if mutant != "last_max" else cand.size - 1 - int(np.argmax(cand[::-1]))
        if mutant == "j+1":
            j = min(j + 1, cand.size - 1)
        best = cand[j]
        rest = np.delete(cand, j)
        second = rest.max() if rest.size else -np.inf
        ec = ce[fin].max()
        safe[i] = best - second > 2 * ec or ec == 0
        cum[i] = ls[i] + best
        err[i] = ec + U * abs(cum[i]) if ec > 0 else 0.0
        if first and (ls[i] <= small if mutant == "le" else ls[i] < small):
            back[i] = -1
            safe[i] = True                                  # (decided by the localscore alone)
        else:
            back[i] = prev[j]
            first = False
    return dict(cumscore=cum, backlink=back, err=err, safe=safe)


# The smallest positive double: -tightness * log(.)^2 rounds to -0 for every predecessor (log(.)^2 <= log(2)^2 < 1/2), on any host.
# The candidates are then the cumulative scores themselves and tie exactly wherever those are equal: the tie rule shows.
BEAT_TIE_TIGHTNESS = 5e-324
BEAT_TIE_KINDS = ("zeros", "plateau", "steps")


def beat_tie_T(period):
    return 5000 if period == 2047 else 300


def beat_input(T, period, kind, seed):
    """onset envelopes divided by their standard deviation, as float32.  For the tie cases: 'zeros'; 'plateau', one click at the
    start and silence after it (the localscore is exactly 0 from frame period + 1 on and the cumulative score stays at its maximum:
    every frame of a window ties); 'steps', a click every 3 period + 1 frames (plateaus of rising height)"""
    rng = np.random.default_rng(seed)
    if kind in ("plateau", "steps"):
        e = np.zeros(T, np.float32)
        e[::T if kind == "plateau" else 3 * period + 1] = 1.5
        return e
    if kind == "zeros":
        return np.zeros(T, np.float32)
    if kind == "constant":
        return np.full(T, 1.25, np.float32)
    if kind == "clicks":
        e = np.zeros(T)
        e[period // 2::max(period, 1)] = 1.0
        e = e + 0.01 * rng.uniform(size=T)
    else:
        e = np.abs(rng.standard_normal(T)) * (0.2 + (np.arange(T) % max(period, 2) == 0))
    sd = e.std(ddof=1) if T > 1 else 1.0
    return f32(e / (sd if sd > 0 else 1.0))


# ----------------------------------------------------------------------------------------------------------------- segment_reduce
REDUCE_L = (1, 2, 3, 64, 65)
REDUCE_C = (1, 63, 64, 65)


def segment_reduce(x, bounds, mode, mutant=None):
    """out[s][c] over frames [bounds[s], bounds[s + 1]): the lower median (mode 0) or the mean as the sequential float32 sum divided
    by the float32 count (mode 1); an empty segment gives NaN"""
    x = f32(x)
    out = np.full((len(bounds) - 1, x.shape[1]), np.nan, np.float32)
    for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
        if mutant == "hi+1":
            hi = min(hi + 1, x.shape[0])
        if mutant == "lo+1":
            lo = lo + 1
        if hi <= lo:
            continue
        seg = x[lo:hi]
        if mode == 0:
            out[s] = lower_median(seg, 0, mutant)
        else:
            acc = np.zeros(x.shape[1], np.float32)
            for row in seg:
                acc = acc + row
            out[s] = acc / np.float32(hi - lo)
    return out


def reduce_input(C, kind, seed):
    """(x [T][C], bounds): segments of every length in REDUCE_L, an empty one between them, ends on the first and last frame"""
    lens = [1, 2, 0, 3, 64, 65, 0, 2]
    bounds = np.concatenate(([0], np.cumsum(lens))).astype(np.int32)
    T = int(bounds[-1])
    rng = np.random.default_rng(seed)
    if kind == "ties":
        x = rng.integers(-2, 3, size=(T, C)).astype(np.float32)
    elif kind == "integers":
        x = rng.integers(-1000, 1001, size=(T, C)).astype(np.float32)       # sums stay exact: the mean is one division
    else:
        x = f32(rng.standard_normal((T, C)))
    return x, bounds


# ----------------------------------------------------------------------------------------------------------------- recurrence
REC_N = (1, 4, 257)
REC_WIDTH = (0, 1, 3)
REC_MAX_N = 16384


def recurrence_affinity(data, k, width, exp_dev=0.0, mutant=None):
    """data [n][d] float32 -> dict(rec, bound, kept, arg, bw).  Column j keeps its k nearest rows: distances sqrt(sum (x - y)^2 + 1e-8)
    in float32, |i - j| < width set to 0, zeros replaced by 1e20, ranked by (value, row); symmetrised by the minimum; bandwidth = lower
    median of the row maxima (a zero median replaced by the largest, or 1); rec = exp(-d / bandwidth), values >= 1 (kept nothing) 0.
    (k = n keeps the 1e20 entries as well: the bandwidth becomes 1e20, every real distance's exponential rounds to 1 and is zeroed,
    and the matrix is exp(-1) inside the excluded band - the reference's own behaviour.)
    With integer features every distance is the correctly rounded root of an exact integer, so the kept set and the bandwidth are
    exact; a value carries the quotient's rounding through the exponential (v |arg|) and expf's allowance exp_dev (relative), plus
    the smallest normal number for results that leave the normal range"""
    data = f32(data)
    n = data.shape[0]
    diff = data[:, None, :] - data[None, :, :]
    acc = np.zeros((n, n), np.float32)
    for c in range(data.shape[1]):                          # sequential, like the kernel (exact for integers anyway)
        acc = acc + diff[:, :, c] * diff[:, :, c]
    dist = np.sqrt(acc + np.float32(1e-8))
    off = np.arange(n)[:, None] - np.arange(n)[None, :]
    band = (off >= -width) & (off <= width) if mutant == "width+1" else (off > -width) & (off < width)
    dist = np.where(band, np.float32(0), dist)
    dist = np.where(dist == 0, dist + np.float32(1e20), dist).astype(np.float32)
    rows = np.arange(n)[:, None]
    if mutant == "last_first":                              # ties: higher row first
        order = np.lexsort((-rows.repeat(n, 1), dist), axis=0)
    else:
        order = np.argsort(dist, axis=0, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, rows.repeat(n, 1), axis=0)
    kk = k + {"k+1": 1, "k-1": -1}.get(mutant, 0)
    kept = np.where(rank < kk, dist, np.float32(0))
    sym = np.minimum(kept, kept.T)
    rowmax = sym.max(1)
    bw = lower_median(rowmax, 0, mutant)
    fallback = not bw > 0
    if fallback:
        bw = rowmax.max() if rowmax.max() > 0 else np.float32(1)
    arg = f64(sym) / -float(bw)
    with np.errstate(under="ignore"):
        rec = np.exp(arg)
    # an exponential that rounds to 1 in float32 counts as "kept nothing" too (segment.py:57): certainly so above -2^-26, certainly
    # not below -2^-24; the inputs keep clear of the band between (`ambiguous`, asserted 0 by both test files)
    is_kept = (sym > 0) & (arg <= -2.0 ** -24)
    ambiguous = int(((sym > 0) & (arg > -2.0 ** -24) & (arg < -2.0 ** -26)).sum())
    rec = np.where(is_kept, rec, 0.0)
    bound = np.where(is_kept, rec * (2 * V * np.abs(arg) + exp_dev + V) + TINY, 0.0)
    return dict(rec=rec, bound=bound, kept=is_kept, arg=arg[is_kept], bw=float(bw), fallback=fallback, ambiguous=ambiguous)


def recurrence_input(n, kind, seed):
    """integer features (squared distances exact, far below 2^24): 'random'; 'duplicates' (every row three times: ties, lower row
    first); 'constant' (every distance the same: most rows keep no neighbour, the bandwidth's median is 0)"""
    rng = np.random.default_rng(seed)
    d = 5
    if kind == "constant":
        return np.full((n, d), 3.0, np.float32)
    x = rng.integers(-20, 21, size=(n, d)).astype(np.float32)
    if kind == "duplicates":
        x = x[np.arange(n) // 3 * 3 % n]
    return x


# ----------------------------------------------------------------------------------------------------------------- median filters
def timelag_median(rec, mutant=None):
    """out[r][c] = median over dc in -3 .. 3 of P[(r - c + c') mod 2 n][c'], c' = reflect(c + dc), P = rec over n rows of zeros"""
    rec = f32(rec)
    n = rec.shape[0]
    P = np.concatenate((rec, np.zeros_like(rec)), 0)
    r, c = np.arange(n)[:, None, None], np.arange(n)[None, :, None]
    cc = reflect_index(c + np.arange(-3, 4)[None, None, :], n, mutant)
    shift = r - c + cc + (1 if mutant == "row+1" else 0)
    vals = rec[shift % n, cc] if mutant == "mod_n" else P[shift % (2 * n), cc]      # (mod n: the roll wraps into the data, not the zeros)
    return np.sort(vals, axis=2)[:, :, 3 + (1 if mutant == "upper" else 0)]


def timelag_literal(rec):
    """segment.py:75-83 as it is written: zero-pad the rows to 2 n, roll column i up by i, median of 7 along the columns with reflect
    padding, roll back, crop"""
    rec = f32(rec)
    n = rec.shape[0]
    P = np.concatenate((rec, np.zeros_like(rec)), 0)
    lag = np.stack([np.roll(P[:, i], -i) for i in range(n)], 1)
    pad = np.pad(lag, ((0, 0), (3, 3)), mode="reflect")
    med = np.median(np.lib.stride_tricks.sliding_window_view(pad, 7, axis=1), axis=-1)
    return np.stack([np.roll(med[:, i], i) for i in range(n)], 1)[:n].astype(np.float32)


def median_filter_rows(x, k, mutant=None):
    """out[r][c] = median over t < k of x[reflect(r + t - k / 2)][c] (k odd)"""
    x = f32(x)
    n = x.shape[0]
    idx = reflect_index(np.arange(n)[:, None] + np.arange(k)[None, :] - k // 2 + (1 if mutant == "row+1" else 0), n, mutant)
    w = x[np.clip(idx, 0, n - 1)]                           # [n][k][m]
    return np.sort(w, axis=1)[:, min((k - 1) // 2 + (1 if mutant == "upper" else 0), k - 1)]


def affinity_like(n, seed):
    """a sparse non-negative matrix with ties and zeros, like a recurrence matrix"""
    rng = np.random.default_rng(seed)
    return f32(rng.integers(0, 4, size=(n, n)) / 4.0 * (rng.uniform(size=(n, n)) < 0.6))


# ----------------------------------------------------------------------------------------------------------------- soft k-means
KM_K = (1, 2, 16)
KM_N = (1, 255, 257)
KM_ITERS = (0, 1, 10)


def _block_sum32(per_thread):
    """the kernel's fixed-order reduction of one value per thread [256][...]: xor shuffles over the 64 lanes of each wave, then the
    four waves in order"""
    v = f32(per_thread).reshape((4, 64) + per_thread.shape[1:])
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lanes ^ o]
    return ((v[0, 0] + v[1, 0]) + v[2, 0]) + v[3, 0]


def soft_kmeans(data, mu0, iters, temp, dtype=np.float64):
    """(r [n][k], mu [k][k]): `iters` updates mu = (r^T data) / sum r with r = softmax(temp data mu^T), then the final r.  float64: the
    formula.  float32: the kernel's own order - rows dealt to 256 threads, each summing its rows in turn, the block sum above,
    mu = (1 / den) num - with numpy's float32 exp and unfused products"""
    data, mu = np.asarray(data, dtype=dtype), np.asarray(mu0, dtype=dtype).copy()
    n, k = data.shape
    t = dtype(temp)

    def resp(mu):
        z = np.zeros((n, k), dtype)
        for c in range(k):
            z = z + data[:, c:c + 1] * mu[None, :, c]
        z = t * z
        e = np.exp(z - z.max(1, keepdims=True))
        den = np.zeros(n, dtype)
        for j in range(k):
            den = den + e[:, j]
        return e / den[:, None]

    for _ in range(iters):
        r = resp(mu)
        if dtype == np.float64:
            mu = (r.T @ data) / r.sum(0)[:, None]
            continue
        pad = (-n) % 256
        rp, dp = np.concatenate((r, np.zeros((pad, k), dtype))), np.concatenate((data, np.zeros((pad, k), dtype)))
        num, den = np.zeros((256, k, k), dtype), np.zeros((256, k), dtype)
        for s in range(0, n + pad, 256):
            num = num + rp[s:s + 256, :, None] * dp[s:s + 256, None, :]
            den = den + rp[s:s + 256]
        mu = (dtype(1) / _block_sum32(den))[:, None] * _block_sum32(num)
    return resp(mu), mu


def kmeans_input(n, k, seed):
    """unit-norm rows around k directions, centres started on rows of the data"""
    rng = np.random.default_rng(seed)
    dirs = rng.standard_normal((k, k))
    x = dirs[rng.integers(0, k, size=n)] + 0.3 * rng.standard_normal((n, k))
    x = f32(x / np.linalg.norm(x, axis=1, keepdims=True))
    return x, x[rng.integers(0, n, size=k)].copy()
