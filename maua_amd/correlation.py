"""Matrix correlations on the device (drop-in for maua/audiovisual/audioreactive/selfsupervised/features/correlation.py:353-382).

X [T, Fx] and Y [T, Fy] are feature matrices over the same T frames.  pearson, concordance, autocorrcorr, rv, rv2 and r1 come out of
maua_correlation (csrc/video_features.hip) as a 0-dim device tensor: the library reduces every one of them to second moments over the time
axis, accumulated in float64, so the reference's T x T matrices are never formed and the host does no arithmetic on the value.

Not built (each raises ``NotImplementedError`` by name): spearman (torchsort), smi and r3 (an SVD), svcca / pwcca / lcka / op (anatome),
the adjusted RV coefficients and Coxhead's.
"""
import torch

from . import _lib as L

METRICS = tuple(L.CORR_METRICS)
SQUARE_ONLY = ("pearson", "concordance", "r1")   # need Fx == Fy (column pairs / a trace of X Y^T)


def check_metric(name, T, Fx, Fy):
    """maua_correlation's refusals for such a call, without a device (maua_correlation_check): raises MauaHipError with its own message."""
    if name not in L.CORR_METRICS:
        raise ValueError(f"unknown correlation metric {name!r}: the metrics are {list(METRICS)}")
    one = 256
    nbytes = L.lib().maua_correlation_workspace(int(T), int(Fx), int(Fy))
    L.check(L.lib().maua_correlation_check(one, one, int(T), int(Fx), int(Fy), L.CORR_METRICS[name], one, max(nbytes, 1 << 40), one))


def correlation(name, X, Y):
    if name not in L.CORR_METRICS:
        raise ValueError(f"unknown correlation metric {name!r}: the metrics are {list(METRICS)}")
    X, Y = L.dev_tensor(X, torch.float32), L.dev_tensor(Y, torch.float32)
    if X.dim() != 2 or Y.dim() != 2 or X.shape[0] != Y.shape[0]:
        raise ValueError(f"{name}: X and Y must be [T, Fx] and [T, Fy] over the same T, got {tuple(X.shape)} and {tuple(Y.shape)}")
    T, Fx, Fy = int(X.shape[0]), int(X.shape[1]), int(Y.shape[1])
    check_metric(name, T, Fx, Fy)   # before anything is allocated or launched
    nbytes = L.lib().maua_correlation_workspace(T, Fx, Fy)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=X.device)
    out = torch.empty((), dtype=torch.float32, device=X.device)
    L.check(L.lib().maua_correlation(L.ctx(X.device), L.ptr(X), L.ptr(Y), T, Fx, Fy, L.CORR_METRICS[name], L.ptr(ws), nbytes, L.ptr(out)))
    return out


def pearson(X, Y):
    return correlation("pearson", X, Y)


def concordance(X, Y):
    return correlation("concordance", X, Y)


def autocorrcorr(X, Y):
    return correlation("autocorrcorr", X, Y)


def rv(X, Y):
    return correlation("rv", X, Y)


def rv2(X, Y):
    return correlation("rv2", X, Y)


def r1(X, Y):
    return correlation("r1", X, Y)


def _unbuilt(name, why):
    def fn(*args, **kwargs):
        raise NotImplementedError(f"{name} is not built: {why}; the metrics that are built are {list(METRICS)}")
    fn.__name__ = name
    fn.__doc__ = f"Not built: {why}"
    return fn


_SORT = "it ranks with torchsort.soft_rank (correlation.py:59-62), which is not part of this build"
_SVD = "it needs a singular value decomposition (correlation.py:187-302), and the library has none"
_ANATOME = "it is a distance of the anatome package (correlation.py:389-402), which is not part of this build"
_RVADJ = ("the adjusted RV coefficients (correlation.py:124-179) are not reduced to the library's moments; _rvadj_maye also fails in the "
          "reference itself when Fx != Fy")
_COXHEAD = "Coxhead's coefficients (correlation.py:325-350) need anatome's CCA or a pseudo-inverse of a T x T matrix"
UNBUILT = {"spearman": _SORT, "smi": _SVD, "r3": _SVD, "svcca": _ANATOME, "pwcca": _ANATOME, "lcka": _ANATOME, "op": _ANATOME,
           "_rvadj_maye": _RVADJ, "_rvadj_ghaziri": _RVADJ, "_coxhead": _COXHEAD, "_coxhead2": _COXHEAD}
spearman = _unbuilt("spearman", _SORT)
smi = _unbuilt("smi", _SVD)
r3 = _unbuilt("r3", _SVD)
svcca = _unbuilt("svcca", _ANATOME)
pwcca = _unbuilt("pwcca", _ANATOME)
lcka = _unbuilt("lcka", _ANATOME)
op = _unbuilt("op", _ANATOME)
_rvadj_maye = _unbuilt("_rvadj_maye", _RVADJ)
_rvadj_ghaziri = _unbuilt("_rvadj_ghaziri", _RVADJ)
_coxhead = _unbuilt("_coxhead", _COXHEAD)
_coxhead2 = _unbuilt("_coxhead2", _COXHEAD)
