"""The GAN evaluation metrics without a device: the numpy twin (tests/metrics_ref.py) against what the reference's own functions returned
(tests/golden/g41_metrics.npz), the conditions under which that fixture pins a device implementation without ambiguity, the host layer's
names, signatures and refusals, and the command line's defaults.

The fixture's inputs are chosen so that the reference alone decides every discrete outcome:
  * no Newton-Schulz error lies within 1 % of the 1e-5 threshold and no ratio e_k / e_(k-1) within 1 % of 1 before the stop, so the
    iteration count cannot turn on a rounding;
  * every |dist - radius| / radius of every prdc comparison is above 1e-9 (the smallest is 1.4e-6), while the device's radii are held to
    1e-12: the counts carry no tolerance.
The Frechet tolerance of the device tests is measured here: eta, the twin's own float64-to-longdouble difference relative to
tr sigma1 + tr sigma2, is 2.4e-16 over the three pairs, so tol = 100 eta = 2.4e-14 (required: <= 1e-9).  The square roots of the singular
product and of the indefinite matrix (the divergence guard) move by 2.7e-12 and 7.3e-16 of |S|_F; each is allowed 100 times its own."""
import inspect
import json
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import metrics_ref as MR  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from maua_amd import metrics as M  # noqa: E402

GOLDEN = Path(__file__).resolve().parent / "golden" / "g41_metrics.npz"
PAIRS = {"a": (41, 96, 96, 24), "b": (42, 200, 180, 70), "c": (43, 64, 80, 16)}
KS = (1, 3, 5)


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def sigs(fx):
    return json.loads(str(fx["signatures"]))


def test_fixture_inputs_are_the_seeded_pairs(fx):
    for tag, (seed, n1, n2, d) in PAIRS.items():
        f1, f2 = MR.gaussian_pair(seed, n1, n2, d)
        assert np.array_equal(f1, fx[f"{tag}_f1"]) and np.array_equal(f2, fx[f"{tag}_f2"]) and f1.dtype == np.float32
    for tag, seed, dup in (("lat", 51, 0), ("dup", 52, 3)):
        real, fake = MR.lattice_pair(seed, 80, 72, 32, duplicates=dup)
        assert np.array_equal(real, fx[f"{tag}_real"]) and np.array_equal(fake, fx[f"{tag}_fake"]) and np.abs(real).max() <= 8
    assert GOLDEN.stat().st_size < 300 * 1024


@pytest.mark.parametrize("tag", sorted(PAIRS))
def test_twin_frechet_and_unambiguous_iteration(fx, tag):
    info = MR.frechet_info(fx[f"{tag}_f1"], fx[f"{tag}_f2"])
    e = np.array(info["errors"], dtype=np.float64)
    assert not info["retried"] and info["iterations"] == len(e) < 100 and e[-1] <= 1e-5
    assert (np.abs(e / 1e-5 - 1) > 0.01).all(), e
    assert (np.abs(e[1:] / e[:-1] - 1) > 0.01).all() and (e[1:] < e[:-1]).all(), e
    assert abs(info["distance"] - float(fx[f"{tag}_frechet"])) <= 1e-14 * info["scale"]


def test_frechet_tolerance_is_the_twins_own_sensitivity(fx):
    eta = MR.frechet_sensitivity([(fx[f"{t}_f1"], fx[f"{t}_f2"]) for t in sorted(PAIRS)])
    assert 0 < 100 * eta <= 1e-9 and eta < 1e-15, eta
    for matrix, stop, guard in ((MR.singular_product(), 17, False), (MR.indefinite_matrix(), 5, True)):
        S, errors, iters = MR.sqrtm(matrix)
        assert iters == stop == MR.sqrtm(matrix, dtype=np.longdouble)[2] and np.isfinite(S).all()
        assert (errors[-1] > errors[-2]) == guard and (guard or errors[-1] <= 1e-5)
        assert (np.abs(np.array(errors, dtype=np.float64) / 1e-5 - 1) > 0.01).all()
        assert 0 < 100 * MR.sqrtm_sensitivity(matrix) <= 1e-9


@pytest.mark.parametrize("tag", sorted(PAIRS))
def test_twin_kernel_distance(fx, tag):
    f1, f2, idx = fx[f"{tag}_f1"], fx[f"{tag}_f2"], fx[f"{tag}_kid_idx"]
    S, two, m = idx.shape
    assert two == 2 and m == min(len(f1), len(f2), m) and idx[:, 0].max() < len(f2) and idx[:, 1].max() < len(f1)
    np.random.seed(int(fx[f"{tag}_kid_seed"]))
    assert np.array_equal(M.draw_subsets(len(f1), len(f2), S, m), idx)      # the host layer draws the reference's subsets
    info = MR.kernel_info(f1, f2, idx)
    d = f1.shape[1]
    bound = ((d + 8) * 2.0 ** -52 * (info["abs_sums"][:, 0] + info["abs_sums"][:, 1]) / (m - 1) + (d + 8) * 2.0 ** -52 * info["abs_sums"][:, 2] * 2 / m)
    assert abs(info["kid"] - float(fx[f"{tag}_kid"])) <= bound.sum() / S / m
    if tag == "c":
        assert all(sorted(idx[s, 1]) == list(range(64)) for s in range(S))      # m = N1: every row of feats1 is drawn


@pytest.mark.parametrize("tag", sorted(PAIRS))
def test_twin_prdc_and_margins(fx, tag):
    f1, f2 = fx[f"{tag}_f1"], fx[f"{tag}_f2"]
    for row, k in zip(fx[f"{tag}_prdc"], KS):
        info = MR.prdc_info(f1, f2, k)
        assert info["margin"] > 1e-9, (k, info["margin"])
        assert MR.prdc_from_counts(info["counts"], len(f1), len(f2), k) == tuple(row)


def test_twin_prdc_on_the_lattices(fx):
    for tag in ("lat", "dup"):
        real, fake, k = fx[f"{tag}_real"].astype(np.float32), fx[f"{tag}_fake"].astype(np.float32), int(fx[f"{tag}_k"])
        info = MR.prdc_info(real, fake, k)
        assert info["counts"] == tuple(fx[f"{tag}_counts"]) and MR.prdc(real, fake, k) == tuple(fx[f"{tag}_prdc"])
        d = MR.pairwise_distances(real, fake)
        assert np.array_equal(d, np.round(d))      # exact integers
    assert (MR.prdc_info(fx["dup_real"].astype(np.float32), fx["dup_fake"].astype(np.float32), 1)["r_real"] == 0).sum() == 6


def _signature(fn):
    p = inspect.signature(fn).parameters
    return list(p), {k: v.default for k, v in p.items() if v.default is not inspect.Parameter.empty}


@pytest.mark.parametrize("ref, fn", [("frechet.sqrtm", M.sqrtm), ("frechet.symsqrtm", M.symsqrtm), ("frechet.frechet_distance", M.frechet_distance),
                                     ("kernel.kernel_distance", M.kernel_distance), ("prdc.pairwise_distances", M.pairwise_distances),
                                     ("prdc.nearest_neighbor_distances", M.nearest_neighbor_distances), ("prdc.prdc", M.prdc)])
def test_signatures_follow_the_reference(sigs, ref, fn):
    args, defaults = _signature(fn)
    assert args == sigs[ref]["args"] and defaults == sigs[ref]["defaults"]


def test_compute_signature_and_flags(sigs):
    args, defaults = _signature(M.compute)
    ref = sigs["compute.compute"]
    n = len(ref["args"])
    assert args[:n] == ref["args"] and args[n] == "return_features" and defaults["return_features"] is False
    for k in ("n_samples", "extractor", "batch_size", "ignore_cache", "verbose"):
        assert defaults[k] == ref["defaults"][k], k
    assert list(defaults["metrics"]) == ref["defaults"]["metrics"]
    assert M.default_num_workers() == min(8, torch.multiprocessing.cpu_count())
    p = M.parser()
    ns = p.parse_args(["--data_dir", "d", "--checkpoint", "c"])
    flags = sigs["compute.flags"]
    assert {a.option_strings[0] for a in p._actions if a.option_strings and a.dest != "help"} == set(flags) | {"--allow_random_init"}
    for flag, spec in flags.items():
        if flag in ("--num_workers", "--device"):      # defaults the reference computes from the machine
            continue
        assert getattr(ns, flag[2:]) == (False if spec.get("action") == "store_true" else spec.get("default", {"--data_dir": "d", "--checkpoint": "c"}.get(flag)))
    assert ns.num_workers == M.default_num_workers() and ns.allow_random_init is False
    assert p.parse_args(["--data_dir", "d", "--checkpoint", "c", "--extractor", "CLIP:ViT-B/32", "--allow_random_init"]).allow_random_init
    with pytest.raises(SystemExit):
        p.parse_args(["--checkpoint", "c"])


def test_reexports_resolve():
    import maua.GAN.metrics as pkg
    import maua.GAN.metrics.compute as c
    import maua.GAN.metrics.frechet as f
    import maua.GAN.metrics.kernel as k
    import maua.GAN.metrics.prdc as p
    assert f.frechet_distance is M.frechet_distance and f.sqrtm is M.sqrtm and f.symsqrtm is M.symsqrtm
    assert k.kernel_distance is M.kernel_distance
    assert p.prdc is M.prdc and p.pairwise_distances is M.pairwise_distances and p.nearest_neighbor_distances is M.nearest_neighbor_distances
    assert c.compute is M.compute and c.FolderImages is M.FolderImages and c.resize_clean is M.resize_clean and c.main is M.main
    assert (pkg.frechet_distance, pkg.kernel_distance, pkg.compute, pkg.prdc) == (M.frechet_distance, M.kernel_distance, c, p)


def test_unbuilt_parts_raise_by_name():
    with pytest.raises(NotImplementedError, match="symsqrtm"):
        M.symsqrtm(torch.eye(3))
    for name in ("SwAV", "Inception"):
        with pytest.raises(NotImplementedError, match=name):
            M.get_extractor(name)
    with pytest.raises(ValueError, match="resnet9000"):
        M.get_extractor("resnet9000")
    for k in (0, 16, 2.5):
        with pytest.raises(ValueError, match=f"nearest_k={k}"):
            M._check_k("prdc", k)
    fn = lambda x: x  # noqa: E731
    assert M.get_extractor(fn)[:2] == (fn, None) and M.get_extractor((fn, 16))[:2] == (fn, 16)


def test_resize_clean_is_the_host_bilinear():
    x = np.arange(8 * 8 * 3, dtype=np.uint8).reshape(8, 8, 3)
    assert np.array_equal(M.resize_clean(x, 8), x.astype(np.float32) / 255.0)      # same size: the identity
    y = M.resize_clean(x, 4)
    assert y.shape == (4, 4, 3) and y.dtype == np.float32 and 0 <= y.min() and y.max() <= 1


def test_no_cpu_path(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    x = torch.zeros(8, 4)
    for call in (lambda: M.frechet_distance(x, x), lambda: M.kernel_distance(x, x), lambda: M.prdc(x, x, 1), lambda: M.sqrtm(torch.eye(4)),
                 lambda: M.pairwise_distances(x), lambda: M.nearest_neighbor_distances(x, 1), lambda: M.moments(x),
                 lambda: M.gemm_f64(torch.eye(2), torch.eye(2)), lambda: M.compute([], lambda: x, extractor=lambda b: b)):
        with pytest.raises(L.MauaHipError, match="no HIP device"):
            call()


def test_library_refusals_without_a_device():
    from maua_amd.build import build
    build()
    lib = L.lib()
    one = 256
    assert lib.maua_gemm_f64(None, 0, 0, 1, 1, 1, 1.0, one, 1, one, 1, 0.0, one, 1) == -1 and b"ctx is NULL" in lib.maua_last_error()
    assert lib.maua_prdc(one, one, 8, one, 8, 4, 0, 16, one, 1 << 30, one, one, one) == -1
    assert lib.maua_last_error() == b"maua_prdc: nearest_k must be 1 .. 15"
    assert lib.maua_prdc(one, one, 3, one, 8, 4, 0, 3, one, 1 << 30, one, one, one) == -1 and b"nearest_k + 1 rows" in lib.maua_last_error()
    assert lib.maua_knn_radii(one, one, 8, 4, 0, 0, one, 1 << 30, one) == -1 and b"maua_knn_radii: nearest_k must be 1 .. 15" == lib.maua_last_error()
    assert lib.maua_gemm_f64(one, 0, 0, 4, 4, 4, 1.0, one, 3, one, 4, 0.0, one, 4) == -1 and b"leading dimension" in lib.maua_last_error()
    assert lib.maua_gemm_f64(one, 0, 0, 0, 4, 4, 1.0, one, 4, one, 4, 0.0, one, 4) == -1
    assert lib.maua_metrics_moments(one, one, 0, 1, 4, one, 1 << 30, one, one) == -1 and b"N - 1" in lib.maua_last_error()
    assert lib.maua_sqrtm_newton_schulz(one, one, 4, 0, one, 1 << 30, one, None, None) == -1 and b"num_iters" in lib.maua_last_error()
    assert lib.maua_sqrtm_newton_schulz(one, one, 4, 5, one, 16, one, None, None) == -1 and b"workspace" in lib.maua_last_error()
    assert lib.maua_kernel_distance(one, one, 8, one, 8, 4, 0, one, 2, 9, one, 1 << 30, one, one, one) == -1 and b"subset size" in lib.maua_last_error()
    # six [d][d] matrices, the reduction's 128 partials and 8 scalars, each rounded up to 256 bytes
    assert lib.maua_sqrtm_workspace(70) == 6 * ((70 * 70 * 8 + 255) // 256 * 256) + 1024 + 256
    assert lib.maua_metrics_moments_workspace(200, 70) == (200 * 70 * 8 + 255) // 256 * 256
    assert lib.maua_prdc_workspace(0, 4, 4) == 0 and lib.maua_frechet_workspace(1, 4, 4) == 0 and lib.maua_kernel_distance_workspace(1, 4) == 0
