"""The float64 matrix-core GEMM and the GAN evaluation metrics on it (csrc/gemm_f64.hip, maua_amd/metrics.py) on the device, against numpy,
the twin (tests/metrics_ref.py) and what the reference's own functions returned (tests/golden/g41_metrics.npz).

Tolerances, each derived or measured on the CPU (tests/test_metrics_host.py proves the conditions they rest on):
  * maua_gemm_f64: integer inputs of magnitude <= 2^20 are bit-equal to numpy (every partial sum is exact, whatever the order); Gaussian
    inputs lie within (K + 2) 2^-52 (|alpha| |A| |B| + |beta C|) element by element; two runs are bit-identical.
  * moments: 4 N 2^-53 times the sum of the absolute terms of each element.
  * Newton-Schulz: the iteration count equals the twin's and every error lies within 64 d 2^-53 (absolute) of the twin's.
  * Frechet distance: within tol (tr sigma1 + tr sigma2) of the reference's value, tol = 100 eta, eta = 2.4e-16 being the twin's own
    float64-to-longdouble difference over the three pairs (tol = 2.4e-14; it is recomputed here and must stay <= 1e-9).  The square roots
    of the singular product (d 70 from 40 rows; it converges in 17 iterations) and of the indefinite matrix (which stops by the divergence
    guard after 5) are held to 100 times the twin's own sensitivity on that matrix, 2.7e-12 and 7.3e-16 of |S|_F: the iteration amplifies
    a rounding of the singular product by four orders of magnitude, so the distances' tol cannot be met there by the twin itself.
  * KID: each of the three per-subset sums within (d + 8) 2^-52 of the sum of its absolute terms; the KID within what follows from that.
  * PRDC: radii within 1e-12 (relative) of the twin's - d <= 70 products at 2^-53 each on a difference of sums no smaller than 1e-3 of
    its terms - and the counts EQUAL, since no comparison lies within 1e-9 of its radius; on the integer lattices everything is exact.
"""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import metrics_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "g41_metrics.npz"
PAIRS = ("a", "b", "c")
U = 2.0 ** -53


@pytest.fixture(scope="module")
def M():
    from maua_amd import metrics
    return metrics


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def tol(fx):
    eta = MR.frechet_sensitivity([(fx[f"{t}_f1"], fx[f"{t}_f2"]) for t in PAIRS])
    assert 0 < 100 * eta <= 1e-9
    return 100 * eta


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- maua_gemm_f64 -----------------------------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1), (16, 16, 4), (17, 15, 5), (70, 70, 70), (33, 130, 257), (257, 150, 20)]      # the last: the 128 x 128 tile


def gemm_case(M, shape, ta, tb, alpha, beta, integer, seed):
    m, n, k = shape
    g = np.random.default_rng(seed)
    draw = (lambda *s: g.integers(-2 ** 20, 2 ** 20 + 1, s).astype(np.float64)) if integer else (lambda *s: g.standard_normal(s))
    pad_a, pad_b, pad_c = 3, 2, 5      # every leading dimension wider than its row
    a_st = draw(*((k, m + pad_a) if ta else (m, k + pad_a)))
    b_st = draw(*((n, k + pad_b) if tb else (k, n + pad_b)))
    c0 = 2.0 * draw(m, n + pad_c)      # even integers: beta = 0.5 stays exact
    opa = a_st[:, :m].T if ta else a_st[:, :k]
    opb = b_st[:, :k].T if tb else b_st[:, :n]
    want = alpha * (opa @ opb) + (beta * c0[:, :n] if beta else 0.0)
    out = dev(c0)
    M.gemm_f64(dev(a_st), dev(b_st), ta, tb, alpha, beta, out=out, M=m, N=n, K=k)
    got = out.cpu().numpy()
    assert np.array_equal(got[:, n:], c0[:, n:]), "columns beyond N were written"
    bound = (k + 2) * 2.0 ** -52 * (abs(alpha) * (np.abs(opa) @ np.abs(opb)) + np.abs(beta * c0[:, :n]))
    return got[:, :n], want, bound, (a_st, b_st, c0)


@pytest.mark.parametrize("shape", GEMM_SHAPES)
@pytest.mark.parametrize("alpha, beta", [(1.0, 0.0), (-2.0, 0.5)])
def test_gemm_f64(M, shape, alpha, beta):
    for ta in (False, True):
        for tb in (False, True):
            got, want, _, _ = gemm_case(M, shape, ta, tb, alpha, beta, True, 1)
            assert np.array_equal(got, want), ("integer inputs", shape, ta, tb, float(np.abs(got - want).max()))
            got, want, bound, (a_st, b_st, c0) = gemm_case(M, shape, ta, tb, alpha, beta, False, 2)
            worst = float((np.abs(got - want) / bound).max())
            print(f"gemm_f64 {shape} ta={int(ta)} tb={int(tb)} alpha={alpha} beta={beta}: worst error / bound = {worst:.3f}")
            assert worst <= 1.0, (shape, ta, tb)
            again = dev(c0)
            M.gemm_f64(dev(a_st), dev(b_st), ta, tb, alpha, beta, out=again, M=shape[0], N=shape[1], K=shape[2])
            assert np.array_equal(again.cpu().numpy()[:, :shape[1]], got), "two runs differ"


def test_gemm_f64_nan_in_beta_zero_output_is_not_read(M):
    a, b = dev(np.ones((5, 7))), dev(np.ones((7, 3)))
    out = torch.full((5, 3), float("nan"), dtype=torch.float64, device="cuda")
    assert np.array_equal(M.gemm_f64(a, b, out=out).cpu().numpy(), np.full((5, 3), 7.0))


# ---- moments -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, d", [(2, 1), (64, 16), (200, 70)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_moments(M, n, d, dtype):
    x = (np.random.default_rng(n + d).standard_normal((n, d)) * 1.5 + 0.7).astype(dtype)
    mean, cov = (t.cpu().numpy() for t in M.moments(dev(x)))
    w = x.astype(np.float64)
    wm = w.mean(0)
    xc = w - wm
    assert (np.abs(mean - wm) <= 4 * n * U * np.abs(w).sum(0) / n).all()
    want = xc.T @ xc / (n - 1)
    bound = 4 * n * U * (np.abs(xc).T @ np.abs(xc)) / (n - 1)
    print(f"moments ({n}, {d}) {np.dtype(dtype).name}: worst cov error / bound = {float((np.abs(cov - want) / np.maximum(bound, 1e-300)).max()):.3f}")
    assert (np.abs(cov - want) <= bound).all()


# ---- Newton-Schulz and the Frechet distance --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", PAIRS)
def test_frechet_on_the_fixture(M, fx, tol, tag):
    f1, f2 = fx[f"{tag}_f1"], fx[f"{tag}_f2"]
    twin = MR.frechet_info(f1, f2)
    got = M.frechet_info(dev(f1), dev(f2))
    d = f1.shape[1]
    assert got["iterations"] == twin["iterations"] and not got["retried"]
    err = np.abs(np.array(got["errors"]) - np.array(twin["errors"], dtype=np.float64))
    rel = abs(got["distance"] - float(fx[f"{tag}_frechet"])) / float(twin["scale"])
    print(f"frechet {tag}: iterations {got['iterations']}, worst error difference {err.max():.3e} (bound {64 * d * U:.3e}), "
          f"distance off by {rel:.3e} of the traces (tol {tol:.3e})")
    assert (err <= 64 * d * U).all()
    assert rel <= tol
    assert M.frechet_distance(dev(f1), dev(f2)) == got["distance"]                       # bit-identical rerun, the plain name
    assert abs(M.frechet_distance(dev(f1).double(), dev(f2).double()) - got["distance"]) == 0.0      # float64 features: the same values


@pytest.mark.parametrize("name, stop, guard", [("singular_product", 17, False), ("indefinite_matrix", 5, True)])
def test_sqrtm_on_hard_matrices(M, name, stop, guard):
    matrix = getattr(MR, name)()
    S_twin, e_twin, it_twin = MR.sqrtm(matrix)
    allow = 100 * MR.sqrtm_sensitivity(matrix)
    assert it_twin == stop and allow <= 1e-9
    S, errors, iters = M.sqrtm_info(dev(matrix))
    S = S.cpu().numpy()
    off = float(np.sqrt(((S - S_twin) ** 2).sum()) / np.sqrt((S_twin ** 2).sum()))
    print(f"sqrtm {name}: iterations {iters}, last errors {errors[-2:]}, |S - twin|_F / |S|_F = {off:.3e} (allowed {allow:.3e})")
    assert iters == it_twin and np.isfinite(S).all()
    assert (errors[-1] > errors[-2]) == guard      # the S of the iteration that stopped, the diverged one included
    assert off <= allow
    assert M.sqrtm(dev(matrix).float(), num_iters=3).dtype == torch.float32 and M.sqrtm_info(dev(matrix), num_iters=3)[2] == 3


# ---- KID ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "c"])
def test_kernel_distance(M, fx, tag):
    f1, f2, idx = fx[f"{tag}_f1"], fx[f"{tag}_f2"], fx[f"{tag}_kid_idx"]
    S, _, m = idx.shape
    d = f1.shape[1]
    twin = MR.kernel_info(f1, f2, idx)
    np.random.seed(int(fx[f"{tag}_kid_seed"]))
    got = M.kernel_info(dev(f1), dev(f2), num_subsets=S, max_subset_size=m)
    assert np.array_equal(got["indices"], idx)
    bound = (d + 8) * 2.0 ** -52 * twin["abs_sums"]
    print(f"kid {tag}: worst sum error / bound = {float((np.abs(got['sums'] - twin['sums']) / bound).max()):.3f}")
    assert (np.abs(got["sums"] - twin["sums"]) <= bound).all()
    kid_bound = ((bound[:, 0] + bound[:, 1]) / (m - 1) + bound[:, 2] * 2 / m).sum() / S / m
    assert abs(got["kid"] - float(fx[f"{tag}_kid"])) <= kid_bound
    np.random.seed(int(fx[f"{tag}_kid_seed"]))
    assert M.kernel_distance(dev(f1), dev(f2), num_subsets=S, max_subset_size=m) == got["kid"]      # bit-identical rerun
    with pytest.raises(ValueError, match="indices"):
        M.kernel_info(dev(f1), dev(f2), indices=np.full((1, 2, 4), len(f1) + len(f2)))


# ---- PRDC --------------------------------------------------------------------------------------------------------------------------------
def prdc_against_twin(M, real, fake, k):
    twin = MR.prdc_info(real, fake, k)
    got = M.prdc_info(dev(real), dev(fake), k)
    for name in ("r_real", "r_fake"):
        r, want = got[name].cpu().numpy(), twin[name]
        assert (np.abs(r - want) <= 1e-12 * want).all(), (name, float(np.abs(r - want).max()))
    assert got["counts"] == twin["counts"], (got["counts"], twin["counts"])
    again = M.prdc_info(dev(real), dev(fake), k)
    assert again["counts"] == got["counts"] and torch.equal(again["r_real"], got["r_real"]) and torch.equal(again["r_fake"], got["r_fake"])
    return got, twin


@pytest.mark.parametrize("tag", ["lat", "dup"])
def test_prdc_on_the_lattices_is_exact(M, fx, tag):
    real, fake, k = fx[f"{tag}_real"].astype(np.float32), fx[f"{tag}_fake"].astype(np.float32), int(fx[f"{tag}_k"])
    got, twin = prdc_against_twin(M, real, fake, k)
    assert got["counts"] == tuple(fx[f"{tag}_counts"]) == M.prdc_counts(dev(real), dev(fake), k)
    assert M.prdc(dev(real), dev(fake), nearest_k=k) == tuple(fx[f"{tag}_prdc"])
    assert np.array_equal(got["r_real"].cpu().numpy(), twin["r_real"]) and np.array_equal(got["r_fake"].cpu().numpy(), twin["r_fake"])
    assert np.array_equal(M.pairwise_distances(dev(real), dev(fake)).cpu().numpy(), MR.pairwise_distances(real, fake))
    assert np.array_equal(M.pairwise_distances(dev(real)).cpu().numpy(), MR.pairwise_distances(real))
    assert np.array_equal(M.nearest_neighbor_distances(dev(real), k).cpu().numpy(), twin["r_real"])
    if tag == "dup":
        assert int((got["r_real"] == 0).sum()) == 6      # a twin point at distance 0: radius 0 for k = 1, and nothing is < 0


@pytest.mark.parametrize("tag", PAIRS)
def test_prdc_on_the_fixture(M, fx, tag):
    f1, f2 = fx[f"{tag}_f1"], fx[f"{tag}_f2"]
    for row, k in zip(fx[f"{tag}_prdc"], (1, 3, 5)):
        prdc_against_twin(M, f1, f2, k)
        assert M.prdc(dev(f1), dev(f2), nearest_k=k) == tuple(row)


@pytest.mark.parametrize("n, m, d, k", [(5, 7, 8, 3), (129, 130, 16, 5), (257, 70, 16, 5), (16, 17, 4, 15)])
def test_prdc_edges(M, n, m, d, k):
    """N = k + 2: the smallest set with a radius that is not the maximum; 129 and 257: one past a tile, and more than one column block"""
    real, fake = MR.gaussian_pair(n + m, n, m, d)
    assert MR.prdc_info(real, fake, k)["margin"] > 1e-9
    got, twin = prdc_against_twin(M, real, fake, k)
    assert M.prdc(dev(real), dev(fake), k) == MR.prdc_from_counts(twin["counts"], n, m, k)


def test_prdc_refusals(M):
    x = torch.zeros(20, 4, device="cuda")
    with pytest.raises(ValueError, match="nearest_k=16"):
        M.prdc(x, x, nearest_k=16)
    with pytest.raises(ValueError, match="nearest_k=0"):
        M.nearest_neighbor_distances(x, 0)
    from maua_amd._lib import MauaHipError
    with pytest.raises(MauaHipError, match="nearest_k \\+ 1 rows"):
        M.prdc(x[:3], x, nearest_k=3)
    with pytest.raises(NotImplementedError, match="symsqrtm"):
        M.symsqrtm(torch.eye(3, device="cuda"))


# ---- compute() end to end ------------------------------------------------------------------------------------------------------------------
def pool_extractor(batch):
    return torch.nn.functional.adaptive_avg_pool2d(batch.float(), 4).flatten(1)      # [B, 3, 16, 16] -> [B, 48]


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    from PIL import Image
    from maua_amd import load as ML
    root = tmp_path_factory.mktemp("metrics")
    (root / "real").mkdir()
    g = np.random.default_rng(5)
    for i in range(64):
        Image.fromarray(g.integers(0, 256, (16, 16, 3), dtype=np.uint8)).save(root / "real" / f"{i:03d}.png")
    torch.save(ML.synthetic_rosinality_checkpoint(), root / "ros.pt")
    return root


def test_compute_end_to_end(M, dataset, tol):
    from maua_amd.load import load_network
    G = load_network(str(dataset / "ros.pt"))
    gen = torch.Generator(device="cuda").manual_seed(3)

    def fake_samples():
        return G(z=torch.randn((16, 512), device="cuda", generator=gen), c=None)

    kw = dict(n_samples=64, extractor=(pool_extractor, 16), batch_size=16, num_workers=0, verbose=False, return_features=True,
              cache_dir=str(dataset / "cache"))
    np.random.seed(11)
    res, real, fake = M.compute(str(dataset / "real"), fake_samples, **kw)
    name = "pool_extractor"
    assert list(res) == [f"Frechet {name} Distance", f"Kernel {name} Distance", f"Precision ({name})", f"Recall ({name})",
                         f"Density ({name})", f"Coverage ({name})"]
    assert real.is_cuda and fake.is_cuda and tuple(real.shape) == tuple(fake.shape) == (64, 48) and real.dtype == torch.float32
    r, f = real.cpu().numpy(), fake.cpu().numpy()
    twin = MR.frechet_info(r, f)
    assert abs(res[f"Frechet {name} Distance"] - float(twin["distance"])) <= tol * float(twin["scale"])
    np.random.seed(11)
    idx = M.draw_subsets(64, 64)
    kt = MR.kernel_info(r, f, idx)
    b = (48 + 8) * 2.0 ** -52 * kt["abs_sums"]
    assert abs(res[f"Kernel {name} Distance"] - float(kt["kid"])) <= ((b[:, 0] + b[:, 1]) / 63 + b[:, 2] * 2 / 64).sum() / 100 / 64
    pi = MR.prdc_info(r, f, 5)
    assert pi["margin"] > 1e-9
    assert tuple(res[k] for k in list(res)[2:]) == MR.prdc_from_counts(pi["counts"], 64, 64, 5)
    cache = dataset / "cache" / f"real_real_{name}_features.npz"
    assert cache.exists()
    res2, real2, _ = M.compute(str(dataset / "real"), fake_samples, **kw)
    assert torch.equal(real2, real) and list(res2) == list(res)      # the cache file's features, no folder read
    assert set(M.compute(str(dataset / "real"), fake_samples, metrics=["prdc"], **{**kw, "return_features": False})) == set(list(res)[2:])


def test_command_line(dataset):
    cmd = [sys.executable, "-m", "maua.GAN.metrics.compute", "--data_dir", str(dataset / "real"), "--checkpoint", str(dataset / "ros.pt"),
           "--extractor", "CLIP:ViT-B/32", "--allow_random_init", "--n_samples", "32", "--batch_size", "16", "--num_workers", "0"]
    out = subprocess.run(cmd, cwd=dataset, env={**__import__("os").environ, "PYTHONPATH": str(ROOT)}, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout[out.stdout.index("{"):])
    ex = "CLIP:ViT-B/32"
    assert set(res) == {f"Frechet {ex} Distance", f"Kernel {ex} Distance", f"Precision ({ex})", f"Recall ({ex})", f"Density ({ex})",
                        f"Coverage ({ex})"}
    assert all(np.isfinite(v) for v in res.values())
