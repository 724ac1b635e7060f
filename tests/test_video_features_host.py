"""CPU-only side of tests/test_gpu_video_features.py: the restatements of tests/video_features_ref.py against the reference's recorded
results (tests/golden/g39_video_features.npz), against torch.histc and against each other, the error bounds the GPU test relies on, and
the Python layer that needs no device (refusals by their text, the names that raise, the absdiff assembly, the score command line)."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import video_features_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def g39():
    z = np.load(ROOT / "tests" / "golden" / "g39_video_features.npz")
    g = {k: z[k] for k in z.files}
    g["chw"] = np.ascontiguousarray(g["clip"].transpose(0, 3, 1, 2))
    g["video"] = R.u8_to_float(g["chw"])
    return g


def test_fixture_is_what_the_issue_describes(g39):
    clip = g39["clip"]
    assert clip.shape == (7, 37, 53, 3) and clip.dtype == np.uint8
    assert sum(bool((f == f[0, 0]).all()) for f in clip) == 1   # one constant frame
    assert (ROOT / "tests" / "golden" / "g39_video_features.npz").stat().st_size < 100 * 1024
    assert g39["X"].shape == (50, 7) and g39["Y"].shape == (50, 7) and g39["Z"].shape == (50, 5)


def test_golden_histograms_exact(g39):
    """The float32 restatement reproduces the reference's recorded histograms bit for bit (constant frame included: min == max)."""
    _, hist = R.features_f32(g39["video"], 32)
    for c, name in enumerate(("redogram", "greenogram", "blueogram")):
        assert np.array_equal(hist[:, c].numpy(), g39[name]), name
    assert np.array_equal(hist[:, :3].reshape(7, 96).numpy(), g39["rgb_hist"])
    counts, _ = R.features_f32(g39["video"], 32)
    assert int(counts.sum()) == 7 * 6 * 37 * 53
    assert bool((counts[:, :3] > 0).all(dim=2).sum() >= 12)   # the gradient frames leave no R / G / B bin empty


def test_golden_scalars_against_float64(g39):
    """The recorded variance, absdiff and metrics are float32 results of the reference's own summation.  Measured on this fixture, the
    reference's departure from the float64 restatement is at most 5.9e-8 relative (variance), 8.5e-8 relative (absdiff) and 7.6e-8 absolute
    (the nine metric values); the bars are 4 x that: 2.4e-7, 3.4e-7 and 3.1e-7."""
    v = g39["video"]
    var = R.variance_f64(v).numpy()
    rel = np.abs(g39["visual_variance"][:, 0] - var) / var
    print("variance departure", rel.max())
    assert rel.max() <= 2.4e-7
    ad = R.absdiff_from_diff(R.diff_f64(v))[:, 0].numpy()
    rel = np.abs(g39["absdiff"][:, 0] - ad) / ad
    print("absdiff departure", rel.max())
    assert rel.max() <= 3.4e-7
    X, Y, Z = (torch.from_numpy(g39[k]) for k in "XYZ")
    for tag, B, names in (("XY", Y, R.METRICS), ("XZ", Z, R.RECT_METRICS)):
        for m in names:
            dep = abs(float(g39[f"{m}_{tag}"]) - R.corr_full(m, X, B))
            print(m, tag, "departure", dep)
            assert dep <= 3.1e-7, (m, tag)


def test_uint8_exact_forms_are_the_float64_restatement(g39):
    """The integer forms the GPU test compares uint8 results with are the float64 restatement of k / 255 without its rounding error."""
    x = torch.from_numpy(g39["chw"]).double() / 255
    assert np.allclose(R.variance_u8_exact(g39["chw"]), R.variance_f64(x).numpy(), rtol=1e-12, atol=1e-15)
    assert np.allclose(R.diff_u8_exact(g39["chw"]), R.diff_f64(x).numpy(), rtol=1e-12, atol=1e-12)
    const = np.full((1, 3, 2, 3), 77, dtype=np.uint8)
    assert R.variance_u8_exact(const) == [0.0]


def test_reduced_form_equals_full_form(g39):
    X, Y, Z = (torch.from_numpy(g39[k]) for k in "XYZ")
    for B, names in ((Y, R.METRICS), (Z, R.RECT_METRICS)):
        for m in names:
            assert abs(R.corr_full(m, X, B) - R.corr_reduced(m, X, B)) <= 1e-12, m


CORR_CASES = [(3, 4, 4, 1), (3, 5, 3, 2), (257, 6, 6, 3), (257, 9, 4, 4)]   # (T, Fx, Fy, seed): shared with the GPU test


@pytest.mark.parametrize("T,Fx,Fy,seed", CORR_CASES)
def test_reduced_form_meets_the_gpu_bar(T, Fx, Fy, seed):
    """Before the GPU test relies on it: on its own inputs the float64 moment form is within a small share of the 4 x 2^-23 bar of the
    reference's form (T = 3: the smallest strict upper triangle; T = 257: 4 slabs of 64 rows and a ragged one)."""
    X, Y = R.corr_inputs(T, Fx, Fy, seed)
    for m in (R.METRICS if Fx == Fy else R.RECT_METRICS):
        full, red = R.corr_full(m, X, Y), R.corr_reduced(m, X, Y)
        assert math.isfinite(full) and abs(full - red) <= R.CORR_BAR / 64, (m, full, red)


def test_lower_median():
    for n in (1, 2, 5, 6):
        v = torch.randn(n, generator=torch.Generator().manual_seed(n))
        assert float(R._lower_median(v)) == float(v.median())


def test_bin_rule_against_histc():
    """The restated bin rule against torch.histc: k / 255 lattices with random ranges, continuous values, min == max."""
    g = torch.Generator().manual_seed(7)
    for trial in range(120):
        bins = int(torch.randint(1, 257, (1,), generator=g))
        lo, hi = sorted(int(k) for k in torch.randint(0, 256, (2,), generator=g))
        n = int(torch.randint(1, 400, (1,), generator=g))
        k = torch.randint(lo, hi + 1, (n,), generator=g).numpy()
        x = torch.from_numpy(R.LUT255[k])
        assert torch.equal(R.histc_counts_f32(x, bins), torch.histc(x, bins=bins).long()), (trial, bins, lo, hi)
    for trial in range(60):
        bins = int(torch.randint(1, 257, (1,), generator=g))
        x = torch.rand(int(torch.randint(1, 3000, (1,), generator=g)), generator=g) * 7 - 3
        assert torch.equal(R.histc_counts_f32(x, bins), torch.histc(x, bins=bins).long()), (trial, bins)
    for value in (0.0, 1.0, 90 / 255, 6.2831855):
        x = torch.full((17,), value, dtype=torch.float32)
        for bins in (1, 32, 255, 256):
            c = R.histc_counts_f32(x, bins)
            assert torch.equal(c, torch.histc(x, bins=bins).long())
            assert int(c[bins // 2]) == 17


def test_hsv_restatement_matches_published_form(g39):
    """rgb_to_hsv_f32 (ties written out) equals the published max / gather form on the CPU, on the clip and on every kind of tie; the hue of a
    pixel with r the maximum and b > g is negative before the remainder and lands in [0, 2 pi)."""
    ties = torch.tensor([[.5, .5, .2], [.5, .2, .5], [.2, .5, .5], [.3, .3, .3], [0., 0., 0.], [1., 1., 1.], [.9, .1, .4]]).T.reshape(1, 3, 7, 1)
    for video in (g39["video"], ties):
        a, b = R.rgb_to_hsv_f32(video), R.rgb_to_hsv_published(video)
        for u, w in zip(a, b):
            assert torch.equal(u, w)
    h, s, v = R.rgb_to_hsv_f32(ties)
    assert float(h[0, 6, 0]) > math.pi and float(h.min()) >= 0 and float(h.max()) < 2 * math.pi + 1e-6
    assert float(s[0, 3, 0]) == 0 and float(s[0, 4, 0]) == 0 and float(h[0, 3, 0]) == 0


def test_float32_sum_bounds_hold_for_the_device_order():
    """The bounds the GPU test applies to float32 input (video_features_ref: any-order float64 sums) hold for the frame pass's own order and
    for three others, against exactly rounded sums (math.fsum), on the GPU test's float32 shapes."""
    g = torch.Generator().manual_seed(11)
    for (H, W) in ((2, 3), (37, 53), (301, 203)):
        a, b = torch.rand(3, H, W, generator=g), torch.rand(3, H, W, generator=g)
        x = a.double().reshape(-1).numpy()
        d = (a - b).abs().double().reshape(-1).numpy()
        n = x.size
        s1x, s2x, dx = math.fsum(x), math.fsum(x * x), math.fsum(d)
        var_exact = (s2x - s1x * s1x / n) / (n - 1)
        perm = np.random.default_rng(3).permutation(n)
        orders = {"device": R.device_order_sum, "sequential": lambda v: float(np.cumsum(v)[-1]), "pairwise": lambda v: float(np.sum(v)),
                  "permuted": lambda v: float(np.cumsum(v[perm])[-1])}
        for name, fn in orders.items():
            S1, S2, D = fn(x), fn(x * x), fn(d)
            var = np.float32((S2 - S1 * S1 / n) / (n - 1))
            assert abs(float(var) - var_exact) <= R.variance_bound_f32(n, s2x, var_exact), (name, H, W)
            assert abs(float(np.float32(D)) - dx) <= R.diff_bound_f32(n, dx), (name, H, W)
        # the bounds are not loose by more than the float32 rounding they contain: they stay within 2 float32 ulps of the value
        assert R.variance_bound_f32(n, s2x, var_exact) <= 2 * 2.0 ** -23 * var_exact
        assert R.diff_bound_f32(n, dx) <= 2 * 2.0 ** -23 * dx


# ---- the Python layer without a device ---------------------------------------------------------------------------------------------------
def test_new_symbols_declared():
    from maua_amd import _lib as L
    names = L.declared_symbols()
    for s in ("maua_vfeat_create", "maua_vfeat_destroy", "maua_vfeat_reset", "maua_vfeat_check", "maua_vfeat_push", "maua_correlation",
              "maua_correlation_check", "maua_correlation_workspace"):
        assert s in names


def test_absdiff_assembly():
    from maua_amd.video_features import assemble_absdiff
    diff = torch.tensor([0., 3., 5., 2.])
    assert torch.equal(assemble_absdiff(diff), torch.tensor([[3.], [5.], [2.], [2.]]))
    with pytest.raises(ValueError, match="at least two frames"):
        assemble_absdiff(torch.tensor([0.]))


def test_vfeat_refusals_by_text():
    from maua_amd import _lib as L
    from maua_amd.video_features import check_push
    check_push(37, 53, 32, 4, 0, 3)
    check_push(1, 1, 1, 1, 2, 1)
    check_push(4096, 4096, 256, 8, 1, 0)
    for args, text in (((37, 53, 32, 4, 3, 1), "layout must be 0"), ((37, 53, 32, 4, -1, 1), "layout must be 0"),
                       ((37, 53, 0, 4, 0, 1), "bins must be 1 .. 256"), ((37, 53, 257, 4, 0, 1), "bins must be 1 .. 256"),
                       ((37, 53, 32, 4, 0, 5), "exceeds max_batch"), ((37, 53, 32, 4, 0, -1), "exceeds max_batch"),
                       ((0, 53, 32, 4, 0, 1), "between 1 and 2^24 pixels"), ((4097, 4096, 32, 4, 0, 1), "between 1 and 2^24 pixels"),
                       ((37, 53, 32, 0, 0, 0), "max_batch must be")):
        with pytest.raises(L.MauaHipError) as e:
            check_push(*args)
        assert text in str(e.value), (args, str(e.value))


def test_layout_of():
    from maua_amd.video_features import layout_of
    assert layout_of(torch.zeros(2, 5, 7, 3, dtype=torch.uint8), 5, 7) == 0
    assert layout_of(torch.zeros(2, 3, 5, 7, dtype=torch.uint8), 5, 7) == 1
    assert layout_of(torch.zeros(2, 3, 5, 7), 5, 7) == 2
    for bad in (torch.zeros(2, 3, 5, 8), torch.zeros(2, 5, 7, 3), torch.zeros(2, 3, 5, 7, dtype=torch.float64)):
        with pytest.raises(ValueError, match="VideoAnalyzer: frames"):
            layout_of(bad, 5, 7)


def test_correlation_refusals_by_text():
    from maua_amd import _lib as L
    from maua_amd import correlation as CR
    for m in CR.METRICS:
        CR.check_metric(m, 50, 7, 7)
    for m in ("rv", "rv2", "autocorrcorr"):
        CR.check_metric(m, 50, 7, 5)
    for m in CR.SQUARE_ONLY:
        with pytest.raises(L.MauaHipError, match="need Fx == Fy"):
            CR.check_metric(m, 50, 7, 5)
    with pytest.raises(L.MauaHipError, match="T must be 2"):
        CR.check_metric("rv", 1, 4, 4)
    with pytest.raises(L.MauaHipError, match="autocorrcorr needs T >= 3"):
        CR.check_metric("autocorrcorr", 2, 4, 4)
    with pytest.raises(L.MauaHipError, match="at most 1024"):
        CR.check_metric("rv", 50, 1000, 25)
    with pytest.raises(ValueError, match="unknown correlation metric"):
        CR.check_metric("kendall", 50, 4, 4)
    lib = L.lib()
    assert lib.maua_correlation_workspace(50, 7, 5) > 0 and lib.maua_correlation_workspace(50, 7, 5) % 256 == 0
    assert lib.maua_correlation_check(256, 256, 50, 7, 5, 3, 256, 16, 256) != 0 and b"workspace" in lib.maua_last_error()
    assert lib.maua_correlation_check(256, 256, 50, 7, 5, 9, 256, 1 << 30, 256) != 0 and b"unknown metric" in lib.maua_last_error()


def test_names_that_raise():
    from maua_amd import correlation as CR
    from maua_amd import video_features as VF
    import maua.audiovisual.audioreactive.selfsupervised.features.correlation as DC
    import maua.audiovisual.audioreactive.selfsupervised.features.video as DV
    x = torch.zeros(4, 3, 5, 5)
    for name in ("fft", "video_spectrogram", "low_freq_rms", "mid_freq_rms", "high_freq_rms", "adaptive_freq_rms", "video_spectral_onsets"):
        with pytest.raises(NotImplementedError, match=rf"^{name} is not built: .*cv2\.linearPolar"):
            getattr(DV, name)(x)
    for name in ("optical_flow_cpu", "directogram", "video_flow_onsets"):
        with pytest.raises(NotImplementedError, match=rf"^{name} is not built: .*winsize=25"):
            getattr(DV, name)(x)
    for name, dep in (("spearman", "torchsort"), ("smi", "singular value"), ("r3", "singular value"), ("svcca", "anatome"), ("pwcca", "anatome"),
                      ("lcka", "anatome"), ("op", "anatome"), ("_rvadj_maye", "adjusted RV"), ("_rvadj_ghaziri", "adjusted RV"),
                      ("_coxhead", "Coxhead"), ("_coxhead2", "Coxhead")):
        with pytest.raises(NotImplementedError, match=rf"^{name} is not built: .*{dep}"):
            getattr(DC, name)(x, x)
    assert set(VF.UNBUILT) | {"redogram", "greenogram", "blueogram", "rgb_hist", "huestogram", "saturogram", "valueogram", "hsv_hist",
                              "visual_variance", "absdiff"} <= set(dir(DV))
    assert set(CR.UNBUILT) | set(CR.METRICS) <= set(dir(DC))


def test_score_cli_arguments():
    from maua_amd.audiovisual import score as S
    a = S.parse_args(["--audio_file", "clip.wav", "--frames", "frames.npy", "--fps", "30"])
    assert (a.audio_file, a.frames, a.fps, a.metrics, a.bins) == ("clip.wav", "frames.npy", 30.0, ["rv2", "autocorrcorr"], 32)
    a = S.parse_args(["--audio_file", "a.wav", "--frames", "f.npy", "--metrics", "rv", "pearson", "--bins", "16", "--batch_size", "4"])
    assert (a.metrics, a.bins, a.batch_size) == (["rv", "pearson"], 16, 4)
    with pytest.raises(SystemExit):
        S.parse_args(["--frames", "f.npy"])
    with pytest.raises(SystemExit):
        S.parse_args(["--audio_file", "a.wav", "--frames", "f.npy", "--metrics", "smi"])
    with pytest.raises(ValueError, match="unknown metric"):
        S.audiovisual_score({"a": torch.zeros(4, 2)}, {"v": torch.zeros(4, 2)}, metrics=("smi",))
    with pytest.raises(ValueError, match="frames must be uint8"):
        S.score_frames("a.wav", np.zeros((4, 5, 5, 3), dtype=np.uint8))


def test_render_loop_signatures_keep_their_defaults():
    import inspect
    from maua_amd.audiovisual.render.ffmpeg import FFMPEG
    from maua_amd.audiovisual.sample import generate
    assert inspect.signature(FFMPEG.__call__).parameters["analyzer"].default is None
    assert inspect.signature(generate).parameters["analyze"].default is False
