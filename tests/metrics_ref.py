"""numpy restatement of the GAN evaluation metrics (frechet_distance with its Newton-Schulz sqrtm, kernel_distance, prdc): the twin the
device kernels are compared with.  float64 by default; ``dtype=np.longdouble`` runs the same arithmetic wider, which is how the tests'
tolerance for the Frechet distance is measured (the twin's own sensitivity to rounding).  Besides the values it returns what the
reference keeps to itself: the error of every Newton-Schulz iteration, the subsets' three sums, the integer counts behind prdc and the
smallest relative margin |dist - radius| / radius of any comparison."""
import numpy as np


def sqrtm(matrix, num_iters=100, dtype=np.float64):
    """-> (S, [error per iteration run], iterations).  Stops once error <= 1e-5 or error > the previous one; S is that iteration's."""
    m = np.asarray(matrix, dtype=dtype)
    dim = m.shape[0]
    norm = np.sqrt((m * m).sum())
    Y, eye, Z = m / norm, np.eye(dim, dtype=dtype), np.eye(dim, dtype=dtype)
    errors, prev, S = [], 1_000_000, None
    for _ in range(num_iters):
        T = dtype(0.5) * (dtype(3.0) * eye - Z @ Y)
        Y, Z = Y @ T, T @ Z
        S = Y * np.sqrt(norm)
        R = m - S @ S
        error = np.sqrt((R * R).sum()) / norm
        errors.append(error)
        if abs(error) <= 1e-5 or error > prev:
            break
        prev = error
    return S, errors, len(errors)


def moments(feats, dtype=np.float64):
    x = np.asarray(feats).astype(dtype)
    mean = x.sum(0) / dtype(x.shape[0])
    xc = x - mean
    return mean, xc.T @ xc / dtype(x.shape[0] - 1)


def frechet_info(feats1, feats2, eps=1e-6, dtype=np.float64, num_iters=100):
    mu1, s1 = moments(feats1, dtype)
    mu2, s2 = moments(feats2, dtype)
    S, errors, iters = sqrtm(s1 @ s2, num_iters, dtype)
    retried = not np.isfinite(S).all()
    if retried:
        off = np.eye(s1.shape[0], dtype=dtype) * dtype(eps)
        S, errors, iters = sqrtm((s1 + off) @ (s2 + off), num_iters, dtype)
    diff = mu1 - mu2
    tr1, tr2 = np.trace(s1), np.trace(s2)
    return {"distance": diff @ diff + tr1 + tr2 - 2 * np.trace(S), "errors": errors, "iterations": iters, "retried": retried,
            "scale": tr1 + tr2, "S": S}


def frechet_distance(feats1, feats2, eps=1e-6):
    return float(frechet_info(feats1, feats2, eps)["distance"])


def kernel_info(feats1, feats2, indices, dtype=np.float64):
    """indices [S, 2, m]: rows of feats2 (x), rows of feats1 (y).  -> kid, sums [S, 3] = (a.sum(), a.diag().sum(), b.sum()) and abs_sums,
    the same sums over the absolute terms (what a rounding bound on a sum scales with)."""
    f1, f2 = np.asarray(feats1).astype(dtype), np.asarray(feats2).astype(dtype)
    n, (S, _, m) = dtype(f1.shape[1]), indices.shape
    sums, abs_sums, t = np.zeros((S, 3), dtype), np.zeros((S, 3), dtype), dtype(0)
    for s in range(S):
        x, y = f2[indices[s, 0]], f1[indices[s, 1]]
        pxx, pyy, pxy = (x @ x.T / n + 1) ** 3, (y @ y.T / n + 1) ** 3, (x @ y.T / n + 1) ** 3
        a = pxx + pyy
        sums[s] = a.sum(), np.trace(a), pxy.sum()
        abs_sums[s] = np.abs(pxx).sum() + np.abs(pyy).sum(), np.abs(np.diag(pxx)).sum() + np.abs(np.diag(pyy)).sum(), np.abs(pxy).sum()
        t += (sums[s, 0] - sums[s, 1]) / (m - 1) - sums[s, 2] * 2 / m
    return {"kid": t / S / m, "sums": sums, "abs_sums": abs_sums}


def pairwise_distances(x, y=None):
    x = np.asarray(x).astype(np.float64)
    y = x if y is None else np.asarray(y).astype(np.float64)
    dist = ((x ** 2).sum(1)[:, None] + (y ** 2).sum(1)[None, :]) - 2.0 * (x @ y.T)
    dist[dist != dist] = 0
    return np.clip(dist, 0.0, np.inf)


def nearest_neighbor_distances(feats, nearest_k):
    return np.sort(pairwise_distances(feats), axis=-1)[:, nearest_k]      # the (k + 1)-th smallest, the self distance included


def _margin(dist, radius):
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(dist - radius) / radius
    rel = rel[np.isfinite(rel)]
    return float(rel.min()) if rel.size else np.inf


def prdc_info(real, fake, nearest_k=5):
    r_real, r_fake = nearest_neighbor_distances(real, nearest_k), nearest_neighbor_distances(fake, nearest_k)
    d = pairwise_distances(real, fake)
    in_real = d < r_real[:, None]
    counts = (int(in_real.any(0).sum()), int((d < r_fake[None, :]).any(1).sum()), int(in_real.sum()), int((d.min(1) < r_real).sum()))
    margin = min(_margin(d, r_real[:, None]), _margin(d, r_fake[None, :]))
    return {"counts": counts, "r_real": r_real, "r_fake": r_fake, "margin": margin, "N": d.shape[0], "M": d.shape[1], "nearest_k": nearest_k}


def prdc_from_counts(counts, N, M, nearest_k):
    p, r, dn, c = (np.float32(v) for v in counts)
    return (float(p / np.float32(M)), float(r / np.float32(N)), float(dn / np.float32(M) / np.float32(nearest_k)), float(c / np.float32(N)))


def prdc(real, fake, nearest_k=5):
    info = prdc_info(real, fake, nearest_k)
    return prdc_from_counts(info["counts"], info["N"], info["M"], nearest_k)


# ---- the inputs the tests build from seeds (the fixture holds only what the reference computed) ------------------------------------------
def gaussian_pair(seed, n1, n2, d):
    """A correlated Gaussian set and a two-component mixture, float32."""
    g = np.random.default_rng(seed)
    mix = g.standard_normal((d, d)) / np.sqrt(d)
    f1 = g.standard_normal((n1, d)) @ (np.eye(d) + 0.5 * mix)
    comp = g.random(n2) < 0.5
    f2 = np.where(comp[:, None], g.standard_normal((n2, d)) * 1.2 + 0.3, g.standard_normal((n2, d)) @ (np.eye(d) + 0.3 * mix.T) - 0.2)
    return f1.astype(np.float32), f2.astype(np.float32)


def lattice_pair(seed, n, m, d, lo=-8, hi=8, duplicates=0):
    """Integer features: every distance is an exact integer in any arithmetic.  duplicates: that many rows of each set repeat another."""
    g = np.random.default_rng(seed)
    a, b = g.integers(lo, hi + 1, (n, d)).astype(np.float32), g.integers(lo, hi + 1, (m, d)).astype(np.float32)
    for j in range(duplicates):
        a[n - 1 - j], b[m - 1 - j] = a[j], b[j]
    return a, b


def indefinite_matrix(seed=7, d=70):
    """A symmetric matrix with one negative eigenvalue: the Newton-Schulz iteration diverges on it, so sqrtm stops by its guard."""
    g = np.random.default_rng(seed)
    q, _ = np.linalg.qr(g.standard_normal((d, d)))
    lam = np.linspace(0.2, 2.0, d)
    lam[3] = -0.5
    return (q * lam) @ q.T


def singular_product(seed=61, n=40, d=70):
    """sigma1 @ sigma2 of two sets with fewer rows than dimensions (both covariances singular), float64."""
    f1, f2 = gaussian_pair(seed, n, n, d)
    return moments(f1)[1] @ moments(f2)[1]


def frechet_sensitivity(pairs):
    """eta: the largest relative difference, over the pairs, between the twin's distance in float64 and in np.longdouble, relative to
    tr sigma1 + tr sigma2.  The tests allow the device 100 eta."""
    eta = 0.0
    for f1, f2 in pairs:
        a, b = frechet_info(f1, f2), frechet_info(f1, f2, dtype=np.longdouble)
        eta = max(eta, float(abs(np.longdouble(a["distance"]) - b["distance"]) / b["scale"]))
    return eta


def sqrtm_sensitivity(matrix):
    """The same for a square root: |S_f64 - S_longdouble|_F / |S_longdouble|_F."""
    a, b = sqrtm(matrix)[0], sqrtm(matrix, dtype=np.longdouble)[0]
    return float(np.sqrt(((a - b) ** 2).sum()) / np.sqrt((b * b).sum()))
