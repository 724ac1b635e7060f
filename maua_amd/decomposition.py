"""Latent directions of a StyleGAN2 generator - closed-form factorisation (SeFa) and GANSpace - on the library's own float64 Jacobi SVD
(drop-in for maua/GAN/decomposition/sefa.py: ``cff`` :16-27, ``apply_sefa`` :5-13).

``svd``, ``svdvals`` and ``eigh`` are the solver as Python calls (csrc/svd_f64.hip: one-sided Jacobi in float64, no vendor solver and no
torch.linalg); they take float32 or float64 tensors from any device, compute in float64 on the GPU and return the input's dtype on the
GPU.  There is no CPU path: without a device they raise ``MauaHipError``.

``cff`` / ``sefa`` factorise the stacked style-affine weights of the convolution layers, ``ganspace`` takes the principal axes of mapped
latents (mean and covariance by ``metrics.moments``, then ``eigh``).  Both return ``Directions``, whose ``apply`` moves a [T, num_ws,
w_dim] latent sequence along the directions with per-frame coefficients (``maua_latent_add_directions``) - the audio-reactive hook is
``maua_amd.latent.direction_modulate``.

Accuracy is norm-wise (|S - S_exact| = O(max(m, n) eps |A|)); small singular values carry no relative claim, and ``eigh``'s eigenvalues
are accurate to O(n eps (|S| + Gershgorin bound)) absolutely.  A zero singular value gets a zero column of U.  Singular vectors are
signed so that the largest-magnitude component of every v_i is positive: the output is a function of the matrix alone.
"""
import argparse
import ctypes as C
from pathlib import Path

import numpy as np
import torch

from . import _lib as L

PATHS = {"auto": 0, "resident": 1, "rounds": 2}     # maua_svd_f64's path argument
MAX_SWEEPS = 30


def _workspace(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device), int(nbytes)


def _path(path):
    return PATHS[path] if isinstance(path, str) else int(path)


def svd_check(m, n, path=0, max_sweeps=0, ws_bytes=None, lda=None):
    """maua_svd_f64's refusals for such a call, without a device (maua_svd_f64_check): raises MauaHipError with its own message."""
    lib, one = L.lib(), C.c_void_p(256)
    need = lib.maua_svd_f64_workspace_bytes(int(m), int(n))
    L.check(lib.maua_svd_f64_check(one, int(m), int(n), int(n if lda is None else lda), 1, _path(path), int(max_sweeps), one,
                                   need if ws_bytes is None else int(ws_bytes), one, one, one))


def svd_info(A, want_u=True, path=0, max_sweeps=0):
    """The decomposition of a 2-D tensor with m >= n, with its record: a dict of U [m, n] (None without ``want_u``), S [n] descending,
    V [n, n] (float64 device tensors, A = U diag(S) V^T), ``sweeps`` and ``last_rotations`` (0 when it converged)."""
    L.require_device()
    a = L.dev_tensor(A, torch.float64)
    if a.dim() != 2:
        raise ValueError(f"svd: the matrix must be 2-D, got {tuple(a.shape)}")
    m, n = map(int, a.shape)
    lib = L.lib()
    L.check(lib.maua_svd_f64_check(C.c_void_p(256), m, n, n, int(want_u), _path(path), int(max_sweeps), C.c_void_p(256), 1 << 60, C.c_void_p(256),
                                   C.c_void_p(256), C.c_void_p(256)))
    ws, nbytes = _workspace(lib.maua_svd_f64_workspace_bytes(m, n), a.device)
    s = torch.empty(n, dtype=torch.float64, device=a.device)
    u = torch.empty((m, n), dtype=torch.float64, device=a.device) if want_u else None
    v = torch.empty((n, n), dtype=torch.float64, device=a.device)
    sweeps, rotations = C.c_int(), C.c_int()
    L.check(lib.maua_svd_f64(L.ctx(a.device), L.ptr(a), m, n, n, int(want_u), _path(path), int(max_sweeps), L.ptr(ws), nbytes, L.ptr(s), L.ptr(u),
                             L.ptr(v), C.byref(sweeps), C.byref(rotations)))
    return {"U": u, "S": s, "V": v, "sweeps": sweeps.value, "last_rotations": rotations.value}


def svd(A, some=True, path=0):
    """``torch.svd``'s convention: (U [m, k], S [k] descending, V [n, k]), k = min(m, n), A = U diag(S) V^T, in A's dtype.  A wide
    matrix is decomposed through its transpose.  ``some=False`` (the full square U) is not built."""
    if not some:
        raise NotImplementedError("svd(some=False) is not built: the Jacobi solver yields the reduced factors only (U [m, min(m, n)])")
    A = torch.as_tensor(A)
    dtype = A.dtype if A.dtype in (torch.float32, torch.float64) else torch.float32
    if A.dim() == 2 and A.shape[0] < A.shape[1]:
        r = svd_info(A.T, True, path)
        U, V = r["V"], r["U"]
    else:
        r = svd_info(A, True, path)
        U, V = r["U"], r["V"]
    return U.to(dtype), r["S"].to(dtype), V.to(dtype)


def svdvals(A, path=0):
    """the singular values alone, descending, in A's dtype"""
    A = torch.as_tensor(A)
    dtype = A.dtype if A.dtype in (torch.float32, torch.float64) else torch.float32
    r = svd_info(A.T if A.dim() == 2 and A.shape[0] < A.shape[1] else A, False, path)
    return r["S"].to(dtype)


def eigh_info(S, path=0, max_sweeps=0):
    """``eigh`` with its record: a dict of w [n] ascending, Q [n, n] (float64 device tensors), ``sweeps`` and ``last_rotations``."""
    L.require_device()
    s = L.dev_tensor(S, torch.float64)
    if s.dim() != 2 or s.shape[0] != s.shape[1]:
        raise ValueError(f"eigh: the matrix must be square, got {tuple(s.shape)}")
    n = int(s.shape[0])
    lib = L.lib()
    L.check(lib.maua_eigh_f64_check(C.c_void_p(256), n, n, _path(path), int(max_sweeps), C.c_void_p(256), 1 << 60, C.c_void_p(256), C.c_void_p(256)))
    ws, nbytes = _workspace(lib.maua_eigh_f64_workspace_bytes(n), s.device)
    w = torch.empty(n, dtype=torch.float64, device=s.device)
    q = torch.empty((n, n), dtype=torch.float64, device=s.device)
    sweeps, rotations = C.c_int(), C.c_int()
    L.check(lib.maua_eigh_f64(L.ctx(s.device), L.ptr(s), n, n, _path(path), int(max_sweeps), L.ptr(ws), nbytes, L.ptr(w), L.ptr(q),
                              C.byref(sweeps), C.byref(rotations)))
    return {"w": w, "Q": q, "sweeps": sweeps.value, "last_rotations": rotations.value}


def eigh(S, path=0):
    """``torch.linalg.eigh``'s convention for a symmetric matrix (only assumed): (w ascending, Q with the eigenvectors in its columns), in
    S's dtype.  Eigenvalue accuracy is absolute, O(n eps (|S| + c)) with c the Gershgorin bound the solver shifts by, not relative."""
    S = torch.as_tensor(S)
    dtype = S.dtype if S.dtype in (torch.float32, torch.float64) else torch.float32
    r = eigh_info(S, path)
    return r["w"].to(dtype), r["Q"].to(dtype)


# ---------------------------------------------------------------------------------------------------------------- the weights
def _synthesis_state(G):
    """the synthesis network's parameters under this project's keys (``bs.{i}.conv{0,1}.affine.weight``) from a StyleGAN2, a
    StyleGAN2Synthesizer, a SynthesisNetwork or a state dict - this project's keys (with or without a ``synthesis.`` prefix) or
    rosinality's (``*.conv.modulation.weight``, bare or under ``g_ema``), translated by maua_amd.load's key map"""
    if isinstance(G, dict):
        sd = G.get("g_ema", G) if isinstance(G.get("g_ema", None), dict) else G
        if any(".modulation." in k for k in sd):
            from .load import rosinality_to_nvidia
            sd = rosinality_to_nvidia({"g_ema": sd}, for_inference=True)[0]
        return {k[len("synthesis."):] if k.startswith("synthesis.") else k: v for k, v in sd.items()}
    for attr in ("synthesizer", "G_synth", "synthesis"):
        if hasattr(G, attr):
            return _synthesis_state(getattr(G, attr))
    if hasattr(G, "state_dict"):
        return _synthesis_state(G.state_dict())
    raise TypeError(f"cff: expected a StyleGAN2, a synthesizer, a SynthesisNetwork or a state dict, got {type(G).__name__}")


def affine_weights(G, layers=None, include_torgb=False):
    """[(key, weight [C_in, w_dim])] of the style-affine layers in execution order: block 0's conv1, then conv0, conv1 of every later
    block (``layers``: indices into that list of convolution layers, e.g. range(0, 6)); with ``include_torgb`` every block's toRGB
    affine follows its conv1.  sefa.py:18 drops ``to_rgbs`` the same way (its test lets the 4 x 4 block's ``to_rgb1`` through - an
    accident of the key's spelling that is not copied)."""
    sd = _synthesis_state(G)
    convs, i = [], 0
    while f"bs.{i}.conv1.affine.weight" in sd:
        for name in ("conv0", "conv1", "torgb"):
            key = f"bs.{i}.{name}.affine.weight"
            if key in sd and (name != "torgb" or include_torgb):
                convs.append((key, name == "torgb"))
        i += 1
    if not convs:
        raise KeyError("cff: no style-affine weights (bs.{i}.conv{0,1}.affine.weight or *.conv.modulation.weight) in this state")
    if layers is not None:
        conv_keys = [k for k, rgb in convs if not rgb]
        chosen = {conv_keys[int(l)] for l in layers}
        blocks = {k.split(".")[1] for k in chosen}
        convs = [(k, rgb) for k, rgb in convs if (k in chosen) or (rgb and k.split(".")[1] in blocks)]
    return [(k, torch.as_tensor(sd[k]).detach()) for k, _ in convs]


def stacked_weight(G, layers=None, include_torgb=False):
    """W [sum C_in, w_dim]: sefa.py:24's ``torch.cat(weight_mat, 0)``"""
    return torch.cat([w.float().cpu() for _, w in affine_weights(G, layers, include_torgb)], 0)


def cff(G, layers=None, include_torgb=False):
    """sefa.py:16-27: the closed-form factorisation -> eigvec [w_dim, w_dim] = ``torch.svd(W).V``, column i the direction of the i-th
    largest singular value (float32, on the device)."""
    return svd(stacked_weight(G, layers, include_torgb))[2]


# ---------------------------------------------------------------------------------------------------------------- directions
class Directions:
    """``vectors`` [k, w_dim] (row j = direction j), ``values`` [k] (sefa: singular values; ganspace: standard deviations), ``mean``
    [w_dim] or None, ``method`` and ``source`` (what they were computed from)."""

    def __init__(self, vectors, values, mean=None, method="sefa", source=None):
        self.vectors, self.values = torch.as_tensor(vectors).float(), torch.as_tensor(values).float()
        self.mean = None if mean is None else torch.as_tensor(mean).float()
        self.method, self.source = str(method), dict(source or {})

    def __len__(self):
        return int(self.vectors.shape[0])

    def apply(self, ws, coeffs, ws_layers=None):
        """ws [T, num_ws, w_dim] moved along the directions: rows lo <= l < hi of frame t get ``+ sum_j coeffs[t, j] vectors[j]``
        (``ws_layers`` = (lo, hi); None = all rows); the other rows are copied.  -> a new float32 device tensor."""
        return add_directions(ws, self.vectors, coeffs, ws_layers)

    def save(self, path):
        arrays = {"vectors": self.vectors.cpu().numpy(), "values": self.values.cpu().numpy(), "method": np.array(self.method)}
        if self.mean is not None:
            arrays["mean"] = self.mean.cpu().numpy()
        for k, v in self.source.items():
            arrays[f"source_{k}"] = np.array(v)
        np.savez(path, **arrays)
        return path


def load(path):
    """a Directions from ``Directions.save``'s .npz (host tensors)"""
    with np.load(path) as f:
        source = {k[len("source_"):]: f[k].tolist() for k in f.files if k.startswith("source_")}
        return Directions(torch.from_numpy(f["vectors"]), torch.from_numpy(f["values"]), torch.from_numpy(f["mean"]) if "mean" in f.files else None,
                          str(f["method"]), source)


def add_directions(ws, vectors, coeffs, ws_layers=None):
    """maua_latent_add_directions: ws [T, num_ws, C], vectors [k, C], coeffs [T, k] -> [T, num_ws, C] float32 on the device"""
    L.require_device()
    ws = L.dev_tensor(torch.as_tensor(ws), torch.float32)
    if ws.dim() != 3:
        raise ValueError(f"add_directions: ws must be [T, num_ws, w_dim], got {tuple(ws.shape)}")
    T, num_ws, Cn = map(int, ws.shape)
    vectors = L.dev_tensor(torch.as_tensor(vectors), torch.float32).reshape(-1, Cn)
    k = int(vectors.shape[0])
    coeffs = L.dev_tensor(torch.as_tensor(coeffs), torch.float32)
    if tuple(coeffs.shape) != (T, k):
        raise ValueError(f"add_directions: coeffs must be [T, k] = [{T}, {k}], got {tuple(coeffs.shape)}")
    lo, hi = (0, num_ws) if ws_layers is None else (int(ws_layers[0]), int(ws_layers[1]))
    out = torch.empty_like(ws)
    L.check(L.lib().maua_latent_add_directions(L.ctx(ws.device), L.ptr(ws), L.ptr(vectors), L.ptr(coeffs), T, num_ws, Cn, k, lo, hi, L.ptr(out)))
    return out


def sefa(G, num_semantic_axis=8, layers=None, include_torgb=False):
    """The first ``num_semantic_axis`` directions of ``cff`` with their singular values -> Directions."""
    W = stacked_weight(G, layers, include_torgb)
    if W.shape[0] < W.shape[1]:
        raise ValueError(f"sefa: the stacked weight is {tuple(W.shape)}: fewer rows than w_dim leaves directions undetermined")
    r = svd_info(W, want_u=False)
    k = min(int(num_semantic_axis), int(W.shape[1]))
    return Directions(r["V"][:, :k].T.contiguous(), r["S"][:k], None, "sefa",
                      dict(layers="all" if layers is None else [int(l) for l in layers], include_torgb=bool(include_torgb),
                           rows=int(W.shape[0]), sweeps=r["sweeps"]))


def ganspace_moments(G, n_samples, seed, truncation=1.0, batch=1024):
    """w [n_samples, w_dim] = the mapper on z drawn by np.random.RandomState(seed), then (mean, cov) in float64 by metrics.moments"""
    from .metrics import moments
    G_map = G.mapper.G_map if hasattr(G, "mapper") else G
    z = torch.from_numpy(np.random.RandomState(seed).randn(int(n_samples), G_map.z_dim)).float()
    w = torch.cat([G_map.forward(z[i:i + batch].cuda(), None, truncation_psi=truncation)[:, 0].float() for i in range(0, int(n_samples), batch)])
    return w, moments(w)


def ganspace(G, n_samples=10_000, seed=0, truncation=1.0, batch=1024, num_axes=None):
    """GANSpace (Haerkoenen et al. 2020): the principal axes of mapped latents, by descending variance -> Directions whose ``values`` are
    the standard deviations along them and whose ``mean`` is the latents' mean."""
    _, (mean, cov) = ganspace_moments(G, n_samples, seed, truncation, batch)
    r = eigh_info(cov)
    k = int(cov.shape[0]) if num_axes is None else min(int(num_axes), int(cov.shape[0]))
    var = r["w"].flip(0)[:k]
    vectors = r["Q"].flip(1)[:, :k].T.contiguous()
    return Directions(vectors, var.clamp_min(0).sqrt(), mean, "ganspace",
                      dict(n_samples=int(n_samples), seed=int(seed), truncation=float(truncation), sweeps=r["sweeps"]))


def apply_sefa(G, w, num_semantic_axis=8, maximum_variations=3.0, num_cols=7, layers=None, ws_layers=None, directions=None):
    """sefa.py:5-13's image canvas -> [num_semantic_axis * num_cols, 3, H, W] in [-1, 1], row-major: row j walks from w to
    w + maximum_variations v_j in num_cols equal steps (column 0 is w itself in every row).

    The signature is adapted: the reference's version reads a StudioGAN generator's ``linear0`` and interpolates with a ``utils.misc``
    module that is not in its tree, so it cannot run there.  Here ``G`` is a StyleGAN2, ``w`` one latent ([w_dim], or [num_ws, w_dim]),
    the directions are ``sefa(G, num_semantic_axis, layers)`` (or ``directions``), the walk is applied to rows ``ws_layers`` of w+ and
    the canvas is rendered by G's synthesizer."""
    d = sefa(G, num_semantic_axis, layers) if directions is None else directions
    k, num_ws = len(d), G.synthesizer.num_ws
    w = L.dev_tensor(torch.as_tensor(w), torch.float32)
    w = w[None].expand(num_ws, -1) if w.dim() == 1 else w.reshape(num_ws, -1)
    steps = torch.linspace(0.0, float(maximum_variations), int(num_cols))
    coeffs = torch.zeros(k * int(num_cols), k)
    for j in range(k):
        coeffs[j * int(num_cols):(j + 1) * int(num_cols), j] = steps
    ws = d.apply(w[None].expand(k * int(num_cols), -1, -1).contiguous(), coeffs, ws_layers)
    # one row of the canvas per call: every row's first image is then rendered at the same place of the same batch
    return torch.cat([G.synthesizer(latents=ws[i:i + int(num_cols)]).float() for i in range(0, len(ws), int(num_cols))])


# ---------------------------------------------------------------------------------------------------------------- command line
def parse_layers(text):
    """'0-5' -> range(0, 6) (both ends included, as the SeFa paper writes its layer ranges); '0,2,4' -> those; None / 'all' -> None"""
    if text in (None, "all"):
        return None
    out = []
    for part in text.split(","):
        lo, _, hi = part.partition("-")
        out += list(range(int(lo), int(hi or lo) + 1))
    return out


def parser():
    p = argparse.ArgumentParser(prog="python -m maua_amd.decomposition", description="latent directions of a StyleGAN2 generator (SeFa / GANSpace)")
    p.add_argument("--model_file", required=True, help="checkpoint ('None': a random-init network)")
    p.add_argument("--method", choices=["sefa", "ganspace"], default="sefa")
    p.add_argument("--num_axes", type=int, default=8)
    p.add_argument("--out", required=True, help="the directions' .npz")
    p.add_argument("--layers", default=None, help="sefa: convolution layers to factorise, e.g. 0-5 (default: all)")
    p.add_argument("--n_samples", type=int, default=10_000, help="ganspace: latents to sample")
    p.add_argument("--seed", type=int, default=0, help="ganspace: seed of the sampled z")
    p.add_argument("--truncation", type=float, default=1.0)
    p.add_argument("--grid", default=None, help="also write the image grid (one row per direction) to this PNG")
    p.add_argument("--seeds", default="1", help="grid: seeds of the latents to walk from, e.g. 1,2 (one grid block each)")
    p.add_argument("--max_variation", type=float, default=3.0)
    p.add_argument("--num_cols", type=int, default=7)
    p.add_argument("--out_size", default=None, help="width,height of the output: e.g. 512,512 (default: the network's own)")
    return p


def main(argv=None):
    args = parser().parse_args(argv)
    from .stylegan2 import StyleGAN2
    out_size = None if args.out_size is None else tuple(int(s) for s in args.out_size.split(","))
    G = StyleGAN2(None if args.model_file == "None" else args.model_file, inference=False, output_size=out_size)
    if args.method == "sefa":
        d = sefa(G, args.num_axes, parse_layers(args.layers))
    else:
        d = ganspace(G, args.n_samples, args.seed, args.truncation, num_axes=args.num_axes)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    d.save(args.out)
    if args.grid is not None:
        from .image import save_image
        from .sampling import tile_grid
        rows = []
        for w in G.get_w_latents(args.seeds, truncation=args.truncation):
            rows.append(apply_sefa(G, w, maximum_variations=args.max_variation, num_cols=args.num_cols, directions=d).cpu())
        save_image(tile_grid(torch.cat(rows), args.num_cols), args.grid)     # every cell is filled: num_axes rows of num_cols per seed
    return d


if __name__ == "__main__":
    main()
