"""numpy restatement of csrc/svd_f64.hip (one-sided Jacobi SVD, the shifted eigh) and of maua_latent_add_directions, the matrices the
decomposition tests run on, and the figures they are held to.  Not a test.

The restatement follows the header's algorithm word for word - tournament order, dgesvj's stop rule, the rotation formulas, the stable
descending sort, the sign rule - but not the device's summation order inside a dot product: it is held to LAPACK by the same bounds as
the device (tests/test_decomposition_host.py), not to the device's bits.  A round's pairs are disjoint, so a round is one vectorised
step over the pairs."""
import numpy as np
import torch

EPS = 2.0 ** -52
MAX_SWEEPS = 30
F32, F64 = np.float32, np.float64


# ------------------------------------------------------------------------------------------------------------------ the schedule
def schedule(n, rnd):
    """the pairs of round ``rnd`` (0 .. N - 2) of a sweep over n columns, N = n rounded up to even, pairs with the padding index dropped"""
    N = n + (n & 1)
    player = lambda k: 0 if k == 0 else 1 + (k - 1 + rnd) % (N - 1)
    pairs = [(player(i), player(N - 1 - i)) for i in range(N // 2)]
    return [(p, q) for p, q in pairs if p < n and q < n]


def rounds(n):
    N = n + (n & 1)
    return N - 1


# ------------------------------------------------------------------------------------------------------------------ the solver
def cosine_of_tangent(t):
    """c = 1 / sqrt(1 + t^2) rounded once, as the device's compensated evaluation delivers it: formed in extended precision and rounded
    to float64.  (The plain float64 expression is biased upwards by a quarter eps for small t - see csrc/svd_f64.hip - and every column
    norm then creeps up by ~23 eps over a 64-column run.  Where numpy's longdouble is no wider than float64 this falls back to that.)"""
    t = np.asarray(t, dtype=np.longdouble)
    return np.asarray(1.0 / np.sqrt(1.0 + t * t), dtype=F64)


def jacobi(A, max_sweeps=MAX_SWEEPS):
    """-> At [n, m] (rotated columns as rows), Vt [n, n] (row j = v_j), sweeps, rotations of the last sweep"""
    A = np.asarray(A, dtype=F64)
    m, n = A.shape
    assert m >= n >= 1
    At, Vt = np.ascontiguousarray(A.T), np.eye(n)
    tol = np.sqrt(float(m)) * EPS
    table = [np.array(schedule(n, r), dtype=np.int64).reshape(-1, 2) for r in range(rounds(n))]
    sweeps = rotated = 0
    for sweeps in range(1, max_sweeps + 1):
        rotated = 0
        for pairs in table:
            if not len(pairs):
                continue
            p, q = pairs[:, 0], pairs[:, 1]
            ap, aq = At[p], At[q]
            alpha, beta, gamma = (ap * ap).sum(1), (aq * aq).sum(1), (ap * aq).sum(1)
            go = (alpha != 0) & (beta != 0) & (np.abs(gamma) > tol * (np.sqrt(alpha) * np.sqrt(beta)))
            if not go.any():
                continue
            p, q, ap, aq, alpha, beta, gamma = p[go], q[go], ap[go], aq[go], alpha[go], beta[go], gamma[go]
            zeta = (beta - alpha) / (2.0 * gamma)
            t = np.where(zeta < 0, -1.0, 1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
            c = cosine_of_tangent(t)
            s = c * t
            c, s = c[:, None], s[:, None]
            At[p], At[q] = c * ap - s * aq, s * ap + c * aq
            vp, vq = Vt[p], Vt[q]
            Vt[p], Vt[q] = c * vp - s * vq, s * vp + c * vq
            rotated += int(go.sum())
        if rotated == 0:
            break
    return At, Vt, sweeps, rotated


def finish(At, Vt, ascending=False):
    """sigma, the stable descending order (``ascending``: read backwards), the signs -> S, U [m, n], V [n, n]"""
    sigma = np.sqrt((At * At).sum(1))
    order = np.argsort(-sigma, kind="stable")
    if ascending:
        order = order[::-1]
    at = np.argmax(np.abs(Vt), axis=1)            # the first maximum: the lowest index on a tie
    sign = np.where(Vt[np.arange(len(Vt)), at] < 0, -1.0, 1.0)
    S = sigma[order]
    V = (sign[:, None] * Vt)[order].T
    with np.errstate(divide="ignore", invalid="ignore"):
        U = np.where(sigma[:, None] > 0, sign[:, None] * At / sigma[:, None], 0.0)[order].T
    return U, S, V


def svd(A, max_sweeps=MAX_SWEEPS):
    """-> U, S, V, sweeps, rotations of the last sweep; A = U diag(S) V^T"""
    At, Vt, sweeps, rotated = jacobi(A, max_sweeps)
    U, S, V = finish(At, Vt)
    return U, S, V, sweeps, rotated


def gershgorin(S):
    return float(np.abs(S).sum(1).max())


def eigh(S, max_sweeps=MAX_SWEEPS):
    """-> w ascending, Q, sweeps, rotations of the last sweep"""
    S = np.asarray(S, dtype=F64)
    c = gershgorin(S)
    At, Vt, sweeps, rotated = jacobi(S + c * np.eye(len(S)), max_sweeps)
    _, sig, Q = finish(At, Vt, ascending=True)
    return sig - c, Q, sweeps, rotated


# ------------------------------------------------------------------------------------------------------------------ the matrices
GAUSSIAN = [(1, 1), (2, 2), (3, 3), (5, 3), (17, 16), (64, 64), (65, 33), (130, 17), (200, 96), (300, 255), (512, 512), (1500, 128)]
SAME_BITS = ["gauss_17x16", "gauss_64x64", "gauss_65x33"]


def gaussian(m, n, seed=None):
    g = torch.Generator().manual_seed(1000 * m + n if seed is None else seed)
    return torch.randn(m, n, generator=g, dtype=torch.float64).numpy()


def matrices():
    """name -> float64 [m, n], m >= n: the list every solver test runs on (inputs drawn by a CPU torch.Generator)"""
    out = {f"gauss_{m}x{n}": gaussian(m, n) for m, n in GAUSSIAN}
    a = gaussian(65, 33).copy()
    a[:, 7] = a[:, 3]
    a[:, 20] = 0.0
    out["dup_zero_65x33"] = a
    out["identity_64"] = np.eye(64)
    out["diag_33"] = np.diag(np.arange(33.0, 0.0, -1.0))
    i = np.arange(64.0)
    out["hilbert_64"] = 1.0 / (i[:, None] + i[None, :] + 1.0)
    out["graded_130x17"] = gaussian(130, 17) * np.logspace(0, -12, 17)[None, :]
    return out


ONE_SWEEP = ["identity_64", "diag_33"]
ZERO_COLUMN = "dup_zero_65x33"


# ------------------------------------------------------------------------------------------------------------------ the figures
def svd_figures(A, U, S, V, sweeps):
    """Every checked quantity as a fraction of its bound (<= 1 passes), against numpy.linalg.svd (LAPACK) of the same matrix:
      sigma     max|S - S_ref|                                   / (4 max(m, n) eps S_ref[0])
      utu       max off-diagonal |U^T U| over S_i > max(m,n) eps S_0  / (2 sqrt(m) eps)
      vtv       |V^T V - I|_max                                  / (sweeps n eps)
      residual  |A - U diag(S) V^T|_F / |A|_F                    / (sweeps n eps)"""
    m, n = A.shape
    S_ref = np.linalg.svd(A, compute_uv=False)
    big = max(m, n)
    out = {"sigma": float(np.abs(S - S_ref).max() / (4 * big * EPS * S_ref[0]))}
    keep = S > big * EPS * S[0]
    Uk = U[:, keep]
    G = Uk.T @ Uk
    off = G - np.diag(np.diag(G))
    out["utu"] = float(np.abs(off).max() / (2 * np.sqrt(m) * EPS)) if off.size else 0.0
    out["vtv"] = float(np.abs(V.T @ V - np.eye(n)).max() / (sweeps * n * EPS))
    out["residual"] = float(np.linalg.norm(A - (U * S[None, :]) @ V.T) / np.linalg.norm(A) / (sweeps * n * EPS))
    return out


def sign_rule_holds(V):
    at = np.argmax(np.abs(V), axis=0)
    return bool((V[at, np.arange(V.shape[1])] > 0).all())


def eigh_matrices():
    """name -> symmetric float64 matrix: +-lambda pairs at n = 32, a 90 x 90 normalised graph Laplacian built as segment.sym_laplacian
    builds one (I - D^-1/2 A D^-1/2 of a symmetric non-negative affinity), a 3 x 3 covariance"""
    g = torch.Generator().manual_seed(77)
    Q, _ = np.linalg.qr(torch.randn(32, 32, generator=g, dtype=torch.float64).numpy())
    lam = np.concatenate([np.linspace(1, 2, 16), -np.linspace(1, 2, 16)])
    pm = (Q * lam[None, :]) @ Q.T
    aff = torch.rand(90, 90, generator=g, dtype=torch.float64).numpy()
    aff = (aff + aff.T) / 2
    np.fill_diagonal(aff, 0.0)
    d = aff.sum(1)
    lap = np.eye(90) - aff / np.sqrt(d[:, None] * d[None, :])
    x = torch.randn(50, 3, generator=g, dtype=torch.float64).numpy()
    return {"plus_minus_32": (pm + pm.T) / 2, "laplacian_90": (lap + lap.T) / 2, "cov_3": np.cov(x.T)}


def eigh_figures(S, w, Q, sweeps):
    """as svd_figures, against numpy.linalg.eigh:
      values    max|w - w_ref|          / (4 n eps (|S|_inf + c))
      residual  |S Q - Q diag(w)|_max   / (sweeps n eps (|S|_inf + c))
      qtq       |Q^T Q - I|_max         / (sweeps n eps)
    and whether w ascends"""
    n = len(S)
    c = gershgorin(S)
    scale = np.abs(S).sum(1).max() + c
    w_ref = np.linalg.eigh(S)[0]
    return {"values": float(np.abs(w - w_ref).max() / (4 * n * EPS * scale)),
            "residual": float(np.abs(S @ Q - Q * w[None, :]).max() / (sweeps * n * EPS * scale)),
            "qtq": float(np.abs(Q.T @ Q - np.eye(n)).max() / (sweeps * n * EPS)),
            "ascending": bool((np.diff(w) >= 0).all())}


# ------------------------------------------------------------------------------------------------------------------ latent directions
def fma32(a, b, c):
    """fmaf on float32 arrays, exactly: the product is exact in float64; the float64 sum is rounded TO ODD (TwoSum tells whether it was
    inexact and on which side the true value lies), and a round-to-odd float64 rounds to float32 as the exact value does."""
    p = a.astype(F64) * b.astype(F64)
    c = np.broadcast_to(c.astype(F64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((err != 0) & even, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(F32)


def add_directions(ws, dirs, coeffs, lo, hi):
    """maua_latent_add_directions in float32: rows lo <= l < hi get ws + sum_j coeffs[t, j] dirs[j], one fmaf per term, j ascending"""
    ws, dirs, coeffs = (np.asarray(x, dtype=F32) for x in (ws, dirs, coeffs))
    out = ws.copy()
    if hi > lo:
        acc = ws[:, lo:hi].copy()
        for j in range(dirs.shape[0]):
            acc = fma32(np.broadcast_to(coeffs[:, j, None, None], acc.shape), np.broadcast_to(dirs[j][None, None, :], acc.shape), acc)
        out[:, lo:hi] = acc
    return out
