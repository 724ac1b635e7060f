"""On the device: the float64 Jacobi SVD / eigh of csrc/svd_f64.hip, the latent-direction kernel, and the decomposition module on top.

The solver is held to numpy.linalg.svd / eigh (LAPACK, float64, CPU) of the same matrix by tests/decomp_ref.py's figures, each a
fraction of its bound (<= 1 passes):
  sigma     max|S - S_ref| <= 4 max(m, n) eps S_ref[0]            both solvers are backward stable to O(n eps |A|); Weyl
  utu       off-diagonal max of U^T U over S_i > max(m,n) eps S_0 <= 2 sqrt(m) eps      the stop rule guarantees sqrt(m) eps
  vtv       |V^T V - I|_max <= sweeps n eps                        a column passes through <= (n - 1) sweeps rotations of a few eps
  residual  |A - U diag(S) V^T|_F / |A|_F <= sweeps n eps
with `sweeps` as the call reported it, on every path that accepts the matrix (path 1: the workgroup-resident one, up to (m + n) n
doubles in 159 KiB; path 2: one launch per round).  Both paths and every rerun must return the same bits.

Measured on an MI355X (identical on both paths wherever both run; DESIGN.md section 5l holds the same table):

  matrix                     paths  sweeps  sigma  utu    vtv    residual
  gauss_1x1                  1, 2   1       0      0      0      0
  gauss_2x2                  1, 2   2       0.109  0.319  0.125  0.225
  gauss_3x3                  1, 2   4       0.071  0.148  0.250  0.076
  gauss_5x3                  1, 2   5       0.098  0.058  0.200  0.074
  gauss_17x16                1, 2   7       0.024  0.452  0.067  0.042
  gauss_64x64                1, 2   11      0.027  0.491  0.018  0.015
  gauss_65x33                1, 2   8       0.016  0.495  0.040  0.028
  gauss_130x17               1, 2   7       0.007  0.320  0.046  0.040
  gauss_200x96               2      10      0.012  0.493  0.016  0.014
  gauss_300x255              2      12      0.018  0.503  0.012  0.008
  gauss_512x512              2      14      0.009  0.503  0.006  0.005
  gauss_1500x128             2      10      0.001  0.499  0.021  0.012
  dup_zero_65x33             1, 2   9       0.013  0.489  0.030  0.025
  identity_64, diag_33       1, 2   1       0      0      0      0
  hilbert_64                 1, 2   24      0.006  0.415  0.010  0.005
  graded_130x17              1, 2   5       0.005  0.383  0.035  0.037
  eigh (values, residual, qtq): plus_minus_32 0.020 0.006 0.028 (9 sweeps); laplacian_90 0.031 0.004 0.029 (10); cov_3 0.038 0.046 0.133 (5)

The CPU restatement on the same matrices (tests/test_decomposition_host.py prints its fractions) stays below 0.2 / 0.51 / 0.25 / 0.34.
With the plain float64 `1 / sqrt(1 + t^2)` the vtv and residual columns were about five times larger and ganspace's sum of variances
missed the trace by 1.5 x its bound (csrc/svd_f64.hip, cosine_of_tangent, says why).

maua_latent_add_directions is held TO THE BIT to decomp_ref.add_directions (one exact float32 fused multiply-add per term)."""
import ctypes as C
import functools
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import cabi_guard as G  # noqa: E402
import decomp_ref as R  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from maua_amd import decomposition as D  # noqa: E402
from maua_amd import latent as LT  # noqa: E402

pytestmark = pytest.mark.gpu
EPS = R.EPS
MATRICES = R.matrices()


def paths_of(m, n):
    """the paths whose _check accepts the matrix"""
    out = []
    for path in (1, 2):
        try:
            D.svd_check(m, n, path=path)
            out.append(path)
        except L.MauaHipError:
            pass
    return out


@functools.lru_cache(maxsize=None)
def solved(name, path):
    r = D.svd_info(torch.from_numpy(MATRICES[name]), want_u=True, path=path)
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()}


# ------------------------------------------------------------------------------------------------------------------ the solver
@pytest.mark.parametrize("name", list(MATRICES))
def test_svd_against_lapack(name):
    A = MATRICES[name]
    m, n = A.shape
    paths = paths_of(m, n)
    assert 2 in paths and ((1 in paths) == ((m + m % 2 + n + n % 2) * n * 8 + 128 <= 159 * 1024))
    for path in paths:
        r = solved(name, path)
        assert r["last_rotations"] == 0 and 1 <= r["sweeps"] <= 30
        figures = R.svd_figures(A, r["U"], r["S"], r["V"], r["sweeps"])
        print(f"{name} path {path}: sweeps {r['sweeps']} " + " ".join(f"{k} {v:.3f}" for k, v in figures.items()))
        assert all(v <= 1.0 for v in figures.values()), (name, path, figures)
        assert (np.diff(r["S"]) <= 0).all() and R.sign_rule_holds(r["V"])
        if name in R.ONE_SWEEP:
            assert r["sweeps"] == 1
        if name == R.ZERO_COLUMN:
            assert r["S"][-1] == 0.0 and not r["U"][:, -1].any(), "a zero column: sigma = 0 exactly and a zero u"


@pytest.mark.parametrize("name", R.SAME_BITS + ["gauss_200x96"])
def test_same_bits_across_reruns_and_paths(name):
    A = torch.from_numpy(MATRICES[name])
    runs = {}
    for path in paths_of(*A.shape):
        first = solved(name, path)
        again = D.svd_info(A, want_u=True, path=path)
        for k in ("U", "S", "V"):
            assert np.array_equal(first[k], again[k].cpu().numpy()), f"{name} path {path}: a rerun changed {k}"
        assert again["sweeps"] == first["sweeps"]
        runs[path] = first
    if name in R.SAME_BITS:
        assert set(runs) == {1, 2}
        for k in ("U", "S", "V"):
            assert np.array_equal(runs[1][k], runs[2][k]), f"{name}: paths 1 and 2 differ in {k}"
        assert runs[1]["sweeps"] == runs[2]["sweeps"]


def test_svd_c_abi_guards_lda_and_no_u():
    """the C entry on guarded buffers: a leading dimension wider than n, u untouched without want_u, the workspace's guards intact"""
    A = R.gaussian(37, 10, seed=5)
    wide = np.full((37, 13), np.nan)
    wide[:, :10] = A
    lib = L.lib()
    need = lib.maua_svd_f64_workspace_bytes(37, 10)
    a, ws = G.inp(wide, torch.float64), G.Buf(need // 8 + 32, torch.float64)
    ws_ptr = C.c_void_p((ws.ptr.value + 255) & ~255)
    s, u, v = G.Buf(10, torch.float64), G.Buf(370, torch.float64), G.Buf(100, torch.float64)
    sweeps, rot = C.c_int(), C.c_int()
    G.call("maua_svd_f64", a.ptr, 37, 10, 13, 1, 2, 0, ws_ptr, need, s.ptr, u.ptr, v.ptr, C.byref(sweeps), C.byref(rot))
    for b, what in ((s, "s"), (u, "u"), (v, "v")):
        b.check(what)
    ws.check("workspace", nan_ok=True, written=False)
    figures = R.svd_figures(A, u.get().reshape(37, 10), s.get(), v.get().reshape(10, 10), sweeps.value)
    assert rot.value == 0 and all(f <= 1.0 for f in figures.values()), figures
    u2, s2, v2 = G.Buf(370, torch.float64), G.Buf(10, torch.float64), G.Buf(100, torch.float64)
    G.call("maua_svd_f64", a.ptr, 37, 10, 13, 0, 2, 0, ws_ptr, need, s2.ptr, u2.ptr, v2.ptr, None, None)
    assert u2.untouched() and np.array_equal(s2.get(), s.get()) and np.array_equal(v2.get(), v.get())
    G.refused("maua_svd_f64", a.ptr, 37, 10, 13, 1, 1, 0, ws_ptr, need - 8, s.ptr, u.ptr, v.ptr, None, None)
    # the sweep cap: an error, the count it reached and the rotations of the last sweep, outputs written
    s3, v3 = G.Buf(10, torch.float64), G.Buf(100, torch.float64)
    rc = lib.maua_svd_f64(L.ctx(), a.ptr, 37, 10, 13, 0, 2, 1, ws_ptr, need, s3.ptr, None, v3.ptr, C.byref(sweeps), C.byref(rot))
    torch.cuda.synchronize()
    assert rc != 0 and b"no sweep without rotations within 1 sweeps" in lib.maua_last_error() and sweeps.value == 1 and rot.value > 0
    s3.check("s after the cap")


def test_wide_and_float32_through_the_python_layer():
    g = torch.Generator().manual_seed(11)
    A = torch.randn(12, 40, generator=g)
    U, S, V = D.svd(A)
    assert U.dtype == S.dtype == V.dtype == torch.float32 and U.shape == (12, 12) and S.shape == (12,) and V.shape == (40, 12)
    S_ref = np.linalg.svd(A.double().numpy(), compute_uv=False)
    assert np.abs(S.double().cpu().numpy() - S_ref).max() <= 2.0 ** -23 * S_ref[0] * 2      # float32 output: its own rounding
    back = (U.double() * S.double()[None]) @ V.double().T
    assert float((back.cpu() - A.double()).norm() / A.double().norm()) <= 4 * 2.0 ** -24 * np.sqrt(12)
    assert torch.equal(D.svdvals(A), S) and torch.equal(D.svdvals(A.T), S)
    assert D.svd(A.double())[1].dtype == torch.float64


# ------------------------------------------------------------------------------------------------------------------ eigh
@pytest.mark.parametrize("name", list(R.eigh_matrices()))
def test_eigh_against_lapack(name):
    S = R.eigh_matrices()[name]
    for path in paths_of(len(S), len(S)):
        r = D.eigh_info(torch.from_numpy(S), path=path)
        w, Q = r["w"].cpu().numpy(), r["Q"].cpu().numpy()
        figures = R.eigh_figures(S, w, Q, r["sweeps"])
        print(f"{name} path {path}: sweeps {r['sweeps']} {figures}")
        assert r["last_rotations"] == 0 and figures.pop("ascending") and all(v <= 1.0 for v in figures.values()), (name, path, figures)
        assert R.sign_rule_holds(Q)
    w32, Q32 = D.eigh(torch.from_numpy(S).float())
    assert w32.dtype == Q32.dtype == torch.float32 and Q32.shape == S.shape


# ------------------------------------------------------------------------------------------------------------------ cff
W_DIM = 64


def small_net(seed=0):
    from maua_amd.stylegan2 import SynthesisNetwork
    return SynthesisNetwork(W_DIM, 32, 3, channel_base=1024, channel_max=48, dtype=torch.float32, generator=torch.Generator().manual_seed(seed))


def test_cff_planted_spectrum_matches_torch_svd():
    """W = U0 diag(s) V0^T with s_i = 2 - i / w_dim split over the layers: every direction is determined with gap 1 / w_dim, so every
    column of cff(G) equals torch.svd(W.double()).V's up to sign within 64 eps s0 w_dim (perturbation 64 eps s0 over the gap)."""
    net = small_net()
    sd = net.state_dict()
    keys = [k for k, _ in D.affine_weights(net)]
    rows = sum(sd[k].shape[0] for k in keys)
    g = torch.Generator().manual_seed(21)
    U0 = torch.linalg.qr(torch.randn(rows, W_DIM, generator=g, dtype=torch.float64))[0]
    V0 = torch.linalg.qr(torch.randn(W_DIM, W_DIM, generator=g, dtype=torch.float64))[0]
    s = 2.0 - torch.arange(W_DIM, dtype=torch.float64) / W_DIM
    W = ((U0 * s[None]) @ V0.T).float()
    at = 0
    for k in keys:
        sd[k] = W[at:at + sd[k].shape[0]].clone()
        at += sd[k].shape[0]
    net.load_state_dict(sd)
    assert torch.equal(D.stacked_weight(net), W)
    want = torch.svd(W.double()).V
    got = D.svd_info(D.stacked_weight(net), want_u=False)["V"].cpu()      # cff's own call, before the cast to float32
    sign = torch.sign((got * want).sum(0))
    err = (got * sign[None] - want).abs().max(0).values
    assert float(err.max()) <= 64 * EPS * float(s[0]) * W_DIM, err
    eig = D.cff(net).cpu()
    assert eig.dtype == torch.float32 and eig.shape == (W_DIM, W_DIM) and torch.equal(eig, got.float())


def test_cff_random_init_residuals():
    net = small_net(3)
    W = D.stacked_weight(net).double()
    r = D.svd_info(W, want_u=True)
    U, S, V = (r[k].cpu() for k in ("U", "S", "V"))
    bound = r["sweeps"] * W.shape[1] * EPS * float(S[0])
    assert float((W @ V - U * S[None]).norm(dim=0).max()) <= bound and float((W.T @ U - V * S[None]).norm(dim=0).max()) <= bound
    S_ref = np.linalg.svd(W.numpy(), compute_uv=False)
    assert np.abs(S.numpy() - S_ref).max() <= 4 * max(W.shape) * EPS * S_ref[0]
    d = D.sefa(net, 5, layers=range(0, 3))
    assert d.vectors.shape == (5, W_DIM) and d.values.shape == (5,) and d.method == "sefa" and d.source["layers"] == [0, 1, 2]


# ------------------------------------------------------------------------------------------------------------------ ganspace
def test_ganspace_moments_trace_orthonormal_and_rerun():
    from maua_amd import metrics
    from maua_amd.stylegan2 import MappingNetwork
    G_map = MappingNetwork(W_DIM, 0, W_DIM, 8, num_layers=2, generator=torch.Generator().manual_seed(4))
    d = D.ganspace(G_map, n_samples=2048, seed=9)
    w, (mean, cov) = D.ganspace_moments(G_map, 2048, 9)
    m2, c2 = metrics.moments(w)
    assert torch.equal(mean, m2) and torch.equal(cov, c2) and torch.equal(d.mean.cpu(), mean.float().cpu())
    trace = float(cov.diagonal().sum())
    r = D.eigh_info(cov)
    assert abs(float(r["w"].sum()) - trace) <= 4 * W_DIM * EPS * trace
    assert torch.equal(d.values.cpu(), r["w"].flip(0).clamp_min(0).sqrt().float().cpu()) and bool((d.values[:-1] >= d.values[1:]).all())
    Q = r["Q"].cpu()
    assert float((Q.T @ Q - torch.eye(W_DIM, dtype=torch.float64)).abs().max()) <= r["sweeps"] * W_DIM * EPS
    assert torch.equal(d.vectors.cpu(), Q.flip(1).T.float())
    again = D.ganspace(G_map, n_samples=2048, seed=9)
    assert torch.equal(again.vectors, d.vectors) and torch.equal(again.values, d.values) and torch.equal(again.mean, d.mean)
    assert d.method == "ganspace" and d.source["n_samples"] == 2048 and d.source["seed"] == 9


# ------------------------------------------------------------------------------------------------------------------ the latent kernel
@pytest.mark.parametrize("T,num_ws,Cn,k,lo,hi", [(3, 6, 512, 1, 0, 6), (3, 6, 512, 5, 0, 6), (3, 6, 512, 1, 2, 4), (3, 6, 512, 5, 2, 4),
                                                 (3, 6, 512, 5, 3, 3), (3, 6, 512, 5, 4, 2), (3, 6, 96, 5, 1, 5), (2, 5, 30, 3, 0, 4),
                                                 (3, 6, 512, 0, 0, 6)])
def test_add_directions_to_the_bit(T, num_ws, Cn, k, lo, hi):
    g = np.random.RandomState(100 * Cn + 10 * k + lo)
    ws, dirs, coeffs = (g.randn(*shape).astype(np.float32) for shape in ((T, num_ws, Cn), (max(k, 1), Cn), (T, max(k, 1))))
    dirs, coeffs = dirs[:k], coeffs[:, :k]
    want = R.add_directions(ws, dirs, coeffs, lo, hi)
    a, d, c, out = G.inp(ws), G.inp(dirs), G.inp(coeffs), G.Buf(ws.size)
    G.call("maua_latent_add_directions", a.ptr, d.ptr, c.ptr, T, num_ws, Cn, k, lo, hi, out.ptr)
    out.check("out")
    got = out.get().reshape(ws.shape)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    outside = [l for l in range(num_ws) if not lo <= l < hi]
    assert np.array_equal(got[:, outside].view(np.uint32), ws[:, outside].view(np.uint32)), "rows outside the range keep their bits"
    if k and hi > lo:
        assert not np.array_equal(got[:, lo:hi], ws[:, lo:hi])
    # the Python layers call the same kernel
    dd = D.Directions(torch.from_numpy(dirs.reshape(k, Cn)), torch.ones(k))
    assert np.array_equal(dd.apply(torch.from_numpy(ws), torch.from_numpy(coeffs), (lo, hi)).cpu().numpy(), want)
    assert np.array_equal(LT.direction_modulate(torch.from_numpy(ws), dd, torch.from_numpy(coeffs), (lo, hi)).cpu().numpy(), want)


def test_add_directions_refusals_and_defaults():
    one = G.Buf(64)
    G.refused("maua_latent_add_directions", one.ptr, one.ptr, one.ptr, 1, 2, 32, 1, 0, 3, one.ptr)
    G.refused("maua_latent_add_directions", one.ptr, None, one.ptr, 1, 2, 32, 1, 0, 2, one.ptr)
    assert one.untouched()
    ws, v, e = torch.randn(4, 6, 32), torch.randn(1, 32), torch.rand(4)
    full = LT.direction_modulate(ws, v, e)                       # one direction, a [T] envelope, all rows
    assert np.array_equal(full.cpu().numpy(), R.add_directions(ws.numpy(), v.numpy(), e.numpy()[:, None], 0, 6))
    low = LT.direction_modulate(ws, v, e, "low")                # LAYER_SLICES by name, clipped to num_ws
    assert torch.equal(low, full)


# ------------------------------------------------------------------------------------------------------------------ end to end
def test_cli_grid_and_modulated_render(tmp_path):
    from PIL import Image
    d = D.main(["--model_file", "None", "--method", "sefa", "--num_axes", "4", "--out", str(tmp_path / "d.npz"), "--grid", str(tmp_path / "g.png"),
                "--out_size", "32,32", "--num_cols", "5"])
    back = D.load(tmp_path / "d.npz")
    assert torch.equal(back.vectors, d.vectors.cpu()) and back.vectors.shape == (4, 512) and back.method == "sefa"
    grid = np.asarray(Image.open(tmp_path / "g.png"))
    assert grid.shape == (4 * 32, 5 * 32, 3), "num_axes rows of num_cols tiles"
    tiles = grid.reshape(4, 32, 5, 32, 3).transpose(0, 2, 1, 3, 4)
    for row in range(1, 4):
        assert np.array_equal(tiles[row, 0], tiles[0, 0]), "column 0 of every row is the unmoved latent's image"
    assert any(not np.array_equal(tiles[row, 4], tiles[row, 0]) for row in range(4)), "the walk changes the image"
    from maua_amd.stylegan2 import StyleGAN2
    Gn = StyleGAN2(None, output_size=(32, 32))
    ws = Gn.get_w_latents("1,2,3")
    moved = LT.direction_modulate(ws, back, torch.rand(3, 4) * 3, "low")
    img = Gn.synthesizer(latents=moved)
    assert img.shape == (3, 3, 32, 32) and bool(torch.isfinite(img.float()).all())
