"""The per-frame visual features and the matrix correlations on the device (csrc/video_features.hip) against tests/video_features_ref.py.

Counts and histograms are compared to the bit with the float32 restatement, the uint8 variance and difference within 2 float32 ulps of
the exact integer form, the float32-input ones within the bounds derived in video_features_ref (proved on the CPU in
tests/test_video_features_host.py), every correlation within 4 x 2^-23 of the float64 restatement of the reference's own form.  Every
output lies between guard regions that must be intact afterwards."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import video_features_ref as R  # noqa: E402
from test_video_features_host import CORR_CASES  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
G = 512   # guard elements on either side of every output
LAYOUTS = ("u8_hwc", "u8_chw", "f32_chw")


class Guarded:
    """A device buffer of ``shape`` between guard regions filled, like the body, with a sentinel bit pattern."""

    def __init__(self, shape, dtype):
        self.n = int(np.prod(shape))
        self.sent = torch.tensor(0x7FC0BEEF if dtype == torch.float32 else 0x5EAD5EAD, dtype=torch.int32)
        self.raw = torch.empty(self.n + 2 * G, dtype=torch.int32, device="cuda").fill_(int(self.sent))
        self.t = self.raw[G:G + self.n].view(dtype).reshape(shape)

    def check(self, what):
        raw = self.raw.cpu()
        assert bool((raw[:G] == self.sent).all()) and bool((raw[G + self.n:] == self.sent).all()), f"{what}: a guard region was written"
        assert not bool((raw[G:G + self.n] == self.sent).any()), f"{what}: an element was left unwritten"
        return self.t.cpu()


def as_layout(chw_u8, layout):
    """uint8 [T, 3, H, W] (numpy) -> the device tensor of that layout; float32 frames hold the bytes' values k / 255."""
    if layout == "u8_hwc":
        return torch.from_numpy(np.ascontiguousarray(chw_u8.transpose(0, 2, 3, 1))).cuda()
    if layout == "u8_chw":
        return torch.from_numpy(np.ascontiguousarray(chw_u8)).cuda()
    return R.u8_to_float(chw_u8).cuda()


def run_stream(frames, H, W, bins, batches, max_batch=None, analyzer=None):
    """Push ``frames`` [T, ...] in the given batch sizes through guarded outputs -> (counts i32 [T, 6, bins], hist f32, variance [T], diff [T])."""
    from maua_amd.video_features import VideoAnalyzer
    an = analyzer if analyzer is not None else VideoAnalyzer(H, W, bins=bins, max_batch=max_batch or max(batches))
    outs, i = [], 0
    for b in batches:
        hist, counts = Guarded((b, 6, bins), torch.float32), Guarded((b, 6, bins), torch.int32)
        var, diff = Guarded((b,), torch.float32), Guarded((b,), torch.float32)
        an.push_raw(frames[i:i + b].contiguous(), hist.t, counts.t, var.t, diff.t)
        torch.cuda.synchronize()
        outs.append((counts.check("counts"), hist.check("hist"), var.check("variance"), diff.check("diff")))
        i += b
    assert i == frames.shape[0]
    if analyzer is None:
        an.close()
    return tuple(torch.cat([o[k] for o in outs]) for k in range(4))


def ulps32(a, ref):
    """|a - ref| in units of float32(ref)'s spacing."""
    ref = np.asarray(ref, dtype=np.float64)
    spacing = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    return np.abs(np.asarray(a, dtype=np.float64) - ref) / spacing


def assert_bits(counts, hist, ref_counts, ref_hist):
    assert torch.equal(counts.long(), ref_counts), "bin counts differ from the float32 restatement"
    assert torch.equal(hist.view(torch.int32), ref_hist.view(torch.int32)), "hist differs from the float32 restatement in its bits"


def assert_u8_scalars(var, diff, chw_u8, first_diff=0.0):
    ev, ed = np.array(R.variance_u8_exact(chw_u8)), np.array(R.diff_u8_exact(chw_u8))
    ed[0] = first_diff
    uv, ud = ulps32(var.numpy(), ev), ulps32(diff.numpy(), ed)
    print("variance ulps", uv.max(), "diff ulps", ud.max())
    assert uv.max() <= 2 and ud.max() <= 2


def assert_f32_scalars(var, diff, video):
    """video: the float32 frames [T, 3, H, W] on the host."""
    n = video[0].numel()
    rv, rd = R.variance_f64(video).numpy(), R.diff_f64(video).numpy()
    s2 = (video.double() ** 2).flatten(1).sum(1).numpy()
    for t in range(video.shape[0]):
        ev, ed = abs(float(var[t]) - rv[t]), abs(float(diff[t]) - rd[t])
        print("frame", t, "variance error", ev, "bound", R.variance_bound_f32(n, s2[t], rv[t]), "diff error", ed, "bound", R.diff_bound_f32(n, rd[t]))
        assert ev <= R.variance_bound_f32(n, s2[t], rv[t]) and ed <= R.diff_bound_f32(n, rd[t])


_cache = {}


def fixture_ref(bins=32):
    if bins not in _cache:
        z = np.load(ROOT / "tests" / "golden" / "g39_video_features.npz")
        chw = np.ascontiguousarray(z["clip"].transpose(0, 3, 1, 2))
        video = R.u8_to_float(chw)
        _cache[bins] = (chw, video) + R.features_f32(video, bins)
    return _cache[bins]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fixture_clip_exact_counts(layout):
    """The fixture clip pushed as 3 + 3 + 1 frames (a carried frame, a ragged last batch) in every layout."""
    chw, video, ref_counts, ref_hist = fixture_ref()
    counts, hist, var, diff = run_stream(as_layout(chw, layout), 37, 53, 32, (3, 3, 1))
    assert_bits(counts, hist, ref_counts, ref_hist)
    if layout == "f32_chw":
        assert_f32_scalars(var, diff, video)
    else:
        assert_u8_scalars(var, diff, chw)


def planted_frame(fill, pixel, H=5, W=7, at=(2, 3)):
    f = np.empty((1, 3, H, W), dtype=np.uint8)
    f[0] = np.array(fill, dtype=np.uint8).reshape(3, 1, 1)
    f[0, :, at[0], at[1]] = pixel
    return f


def run_planted(chw, layout, bins=32):
    H, W = chw.shape[2:]
    ref_counts, ref_hist = R.features_f32(R.u8_to_float(chw), bins)
    counts, hist, _, _ = run_stream(as_layout(chw, layout), H, W, bins, (chw.shape[0],))
    assert_bits(counts, hist, ref_counts, ref_hist)
    return counts[0].long()


PLANT_LAYOUTS = ("u8_hwc", "f32_chw")


@pytest.mark.parametrize("layout", PLANT_LAYOUTS)
def test_planted_negative_hue(layout):
    """r the maximum and b > g: h1 < 0, the remainder must bring it to 5/6 .. 1 of the circle, not leave it negative (C's fmodf)."""
    c = run_planted(planted_frame((100, 100, 100), (200, 50, 120)), layout)
    assert int(c[3, 0]) == 34 and int(c[3, 31]) == 1 and int(c[3].sum()) == 35   # the grey fill has hue 0, the pixel the frame's largest hue


@pytest.mark.parametrize("layout", PLANT_LAYOUTS)
@pytest.mark.parametrize("pixel", [(200, 200, 50), (200, 50, 200), (50, 200, 200)])
def test_planted_tie(layout, pixel):
    """Two channels share the maximum: the first one's hue formula applies."""
    c = run_planted(planted_frame((100, 100, 100), pixel), layout)
    assert int(c[3, 0]) == 34 and int(c[3, 31]) == 1


@pytest.mark.parametrize("layout", PLANT_LAYOUTS)
def test_planted_grey_and_black(layout):
    """A grey pixel (deltac == 0 -> 1, s = 0) and a black one (s = 0 / (0 + 1e-8), v = 0) in a saturated frame."""
    c = run_planted(planted_frame((200, 50, 50), (120, 120, 120)), layout)
    assert int(c[4, 0]) == 1 and int(c[4, 31]) == 34
    c = run_planted(planted_frame((200, 50, 50), (0, 0, 0)), layout)
    assert int(c[4, 0]) == 1 and int(c[5, 0]) == 1 and int(c[5, 31]) == 34


@pytest.mark.parametrize("layout", PLANT_LAYOUTS)
@pytest.mark.parametrize("bins", [1, 32, 256])
def test_planted_maximum_lands_in_last_bin(layout, bins):
    """The frame's maximum itself gives pos == bins and belongs to the last bin."""
    f = planted_frame((10, 20, 30), (255, 20, 30))
    f[0, 0, 0, 0] = 97   # a third value, so that the range is not just its two ends
    c = run_planted(f, layout, bins)
    assert int(c[0, bins - 1]) == (1 if bins > 1 else 35) and int(c[0].sum()) == 35


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("bins", [1, 32, 256])
def test_constant_frame(layout, bins):
    """min == max: the range widens to [v - 1, v + 1] and everything lands in bin bins // 2; the hue histogram is that of h = 0."""
    f = planted_frame((90, 90, 90), (90, 90, 90))
    c = run_planted(f, layout, bins)
    assert bool((c[:, bins // 2] == 35).all()) and int(c.sum()) == 6 * 35
    f = planted_frame((90, 160, 40), (90, 160, 40))
    c = run_planted(f, layout, bins)
    assert bool((c[:, bins // 2] == 35).all())


SHAPES = [(2, 3), (301, 203)]   # a tail-only frame where N - 1 = 17 is far from N; 15 workgroups of 4096 pixels, the last one ragged (3759)


@pytest.mark.parametrize("H,W", SHAPES)
@pytest.mark.parametrize("bins", [1, 32, 256])
def test_shapes_uint8(H, W, bins):
    g = np.random.default_rng(H * W + bins)
    chw = g.integers(0, 256, (3, 3, H, W), dtype=np.uint8)
    chw[1, :, : H // 2] //= 3   # a frame whose range is not the full one
    ref_counts, ref_hist = R.features_f32(R.u8_to_float(chw), bins)
    for layout in ("u8_hwc", "u8_chw"):
        counts, hist, var, diff = run_stream(as_layout(chw, layout), H, W, bins, (2, 1))
        assert_bits(counts, hist, ref_counts, ref_hist)
        assert_u8_scalars(var, diff, chw)


@pytest.mark.parametrize("H,W", SHAPES + [(37, 53)])
def test_shapes_float32(H, W):
    """Continuous float32 values (off the 1 / 255 lattice): every bin goes through the float path."""
    g = torch.Generator().manual_seed(H * W)
    video = torch.rand(3, 3, H, W, generator=g)
    video[1] = video[1] * 0.5 + 0.25
    ref_counts, ref_hist = R.features_f32(video, 32)
    counts, hist, var, diff = run_stream(video.cuda(), H, W, 32, (1, 2))
    assert_bits(counts, hist, ref_counts, ref_hist)
    assert_f32_scalars(var, diff, video)


def test_stream_state():
    """After reset() the first diff is 0; without one it is against the previous push's last frame; a rerun gives the same bits."""
    from maua_amd.video_features import VideoAnalyzer
    chw, video, _, _ = fixture_ref()
    frames = as_layout(chw, "u8_hwc")
    exact = R.diff_u8_exact(chw)
    an = VideoAnalyzer(37, 53, bins=32, max_batch=4)
    first = run_stream(frames[:4], 37, 53, 32, (4,), analyzer=an)
    assert float(first[3][0]) == 0.0
    second = run_stream(frames[4:], 37, 53, 32, (3,), analyzer=an)
    assert ulps32(float(second[3][0]), exact[4]) <= 2 and exact[4] > 0
    an.reset()
    again = run_stream(frames[4:], 37, 53, 32, (3,), analyzer=an)
    assert float(again[3][0]) == 0.0 and torch.equal(again[3][1:], second[3][1:])
    an.reset()
    rerun = run_stream(frames[:4], 37, 53, 32, (4,), analyzer=an)
    for a, b in zip(first, rerun):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the layout may not change inside a stream
    from maua_amd import _lib as L
    with pytest.raises(L.MauaHipError, match="layout changed inside a stream"):
        an.push(as_layout(chw, "u8_chw")[:1])
    with pytest.raises(L.MauaHipError, match="exceeds max_batch"):
        an.push_raw(frames[:5], *(torch.empty(5 * 6 * 32, device="cuda") for _ in range(4)))
    an.close()


def test_analyzer_features_and_whole_clip_functions():
    """VideoAnalyzer.features() on batches equals the reference-named functions on the whole clip, which equal the restatement."""
    from maua_amd import video_features as VF
    chw, video, ref_counts, ref_hist = fixture_ref()
    an = VF.VideoAnalyzer(37, 53, bins=32, max_batch=3)
    an.push(as_layout(chw, "u8_hwc"))
    f = {k: v.cpu() for k, v in an.features().items()}
    an.close()
    dev = video.cuda()
    assert torch.equal(f["rgb_hist"], ref_hist[:, :3].reshape(7, 96)) and torch.equal(f["rgb_hist"], VF.rgb_hist(dev, 96).cpu())
    assert torch.equal(f["hsv_hist"], ref_hist[:, 3:].reshape(7, 96)) and torch.equal(f["hsv_hist"], VF.hsv_hist(dev, 96).cpu())
    for c, fn in enumerate((VF.redogram, VF.greenogram, VF.blueogram, VF.huestogram, VF.saturogram, VF.valueogram)):
        assert torch.equal(fn(dev).cpu(), ref_hist[:, c])
    exact = np.array(R.diff_u8_exact(chw))
    assert f["absdiff"].shape == (7, 1) and ulps32(f["absdiff"][:, 0].numpy(), np.concatenate((exact[1:], exact[-1:]))).max() <= 2
    assert f["visual_variance"].shape == (7, 1) and ulps32(f["visual_variance"][:, 0].numpy(), R.variance_u8_exact(chw)).max() <= 2
    assert np.allclose(VF.visual_variance(dev).cpu().numpy(), f["visual_variance"].numpy(), rtol=1e-6)
    assert np.allclose(VF.absdiff(dev).cpu().numpy(), f["absdiff"].numpy(), rtol=1e-6)


# ---- correlations ------------------------------------------------------------------------------------------------------------------------
def corr_cases():
    z = np.load(ROOT / "tests" / "golden" / "g39_video_features.npz")
    X, Y, Z = (torch.from_numpy(z[k]) for k in "XYZ")
    cases = [("fixture XY", X, Y), ("fixture XZ", X, Z)]
    for T, Fx, Fy, seed in CORR_CASES:
        cases.append((f"T={T} {Fx}x{Fy}", *R.corr_inputs(T, Fx, Fy, seed)))
    return cases


@pytest.mark.parametrize("case", range(2 + len(CORR_CASES)))
def test_correlations(case):
    from maua_amd import correlation as CR
    name, X, Y = corr_cases()[case]
    xd, yd = X.cuda(), Y.cuda()
    for m in (R.METRICS if X.shape[1] == Y.shape[1] else R.RECT_METRICS):
        got, ref = float(getattr(CR, m)(xd, yd)), R.corr_full(m, X, Y)
        print(name, m, got, ref, abs(got - ref))
        assert abs(got - ref) <= R.CORR_BAR, (name, m)


def test_correlation_rerun_and_refusal():
    from maua_amd import _lib as L
    from maua_amd import correlation as CR
    X, Y = R.corr_inputs(257, 9, 4, 4)
    xd, yd = X.cuda(), Y.cuda()
    for m in R.RECT_METRICS:
        a, b = CR.correlation(m, xd, yd), CR.correlation(m, xd, yd)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for m in ("pearson", "concordance", "r1"):
        with pytest.raises(L.MauaHipError, match="need Fx == Fy"):
            getattr(CR, m)(xd, yd)


# ---- the render loop -----------------------------------------------------------------------------------------------------------------------
def test_render_integration(monkeypatch):
    """A random-init generator at 64^2, 10 frames in batches of 4 through FFMPEG with the writer replaced: the frames handed to the writer are
    byte-identical with and without the analyser, analyzer.features() equals the whole-clip functions on the collected frames, and
    audiovisual_score of them is finite."""
    from maua_amd import video_features as VF
    from maua_amd.audiovisual.render import ffmpeg as FF
    from maua_amd.audiovisual.score import audiovisual_score
    from maua_amd.stylegan2 import SynthesisNetwork

    written = []

    class Writer:
        def __init__(self, *a, **k):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False

        def write(self, u8):
            written.append(u8.cpu().clone())

    class Synth:
        output_size = (64, 64)

        def __init__(self):
            self.net = SynthesisNetwork(64, 64, 3, channel_base=2048, channel_max=128, generator=torch.Generator().manual_seed(0))

        def __call__(self, latents, rgb8_out=None):
            return self.net(latents, rgb8_out=rgb8_out)

    monkeypatch.setattr(FF, "VideoWriter", Writer)
    synth = Synth()
    g = torch.Generator().manual_seed(1)
    a, b = torch.randn(2, 1, synth.net.num_ws, 64, generator=g)
    w = torch.linspace(0, 1, 10).reshape(10, 1, 1)
    latents = (a * (1 - w) + b * w).cuda()
    renderer = FF.FFMPEG("unused.mp4", fps=30, batch_size=4)
    renderer(synth, {"latents": latents})
    plain = torch.cat(written)
    written.clear()
    an = VF.VideoAnalyzer(64, 64, bins=32, max_batch=4)
    renderer(synth, {"latents": latents}, analyzer=an)
    analysed = torch.cat(written)
    assert plain.shape == (10, 64, 64, 3) and torch.equal(plain, analysed) and float(plain.float().std()) > 1
    f = an.features()
    an.close()
    video = analysed.permute(0, 3, 1, 2).contiguous().cuda()
    assert torch.equal(f["rgb_hist"], VF.rgb_hist(video, 96)) and torch.equal(f["hsv_hist"], VF.hsv_hist(video, 96))
    assert torch.equal(f["visual_variance"], VF.visual_variance(video)) and torch.equal(f["absdiff"], VF.absdiff(video))
    with pytest.raises(NotImplementedError, match="world > 1"):
        renderer(synth, {"latents": latents}, world=2, analyzer=an)
    audio = {"ramp": torch.linspace(0, 1, 10).reshape(10, 1).cuda() ** 2 + 0.05 * torch.rand(10, 1, generator=g).cuda(),
             "pair": torch.rand(10, 2, generator=g).cuda()}
    table = audiovisual_score(audio, f)
    assert table["audio"] == ["ramp", "pair", "all"] and table["video"] == ["rgb_hist", "hsv_hist", "visual_variance", "absdiff", "all"]
    for m in ("rv2", "autocorrcorr"):
        assert tuple(table[m].shape) == (3, 5) and bool(torch.isfinite(table[m]).all()), table[m]


def test_generate_analyze(tmp_path):
    """sample.generate(analyze=True): the frames, plus the score table of the clip's audio features against the video features taken batch by
    batch inside the loop (352 frames at 256^2: the sampler's sigma = 80 filter needs more than 320 frames, its noise maps at least this size)."""
    import wave
    from maua_amd.audiovisual.sample import ALLFEATS, generate
    from maua_amd.pipeline import synthetic_audio
    sr = 30720
    pcm = (synthetic_audio(352 * 1024, sr).clamp(-1, 1) * 32767).short().numpy()
    with wave.open(str(tmp_path / "clip352.wav"), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr); w.writeframes(pcm.tobytes())
    _, frames, table = generate(str(tmp_path / "clip352.wav"), None, out_dir=str(tmp_path), analyze=True, seed=5, fps=30, downscale_factor=4,
                                batch_size=32)
    assert tuple(frames.shape) == (352, 256, 256, 3) and float(frames.float().std()) > 1
    assert set(table["audio"]) == set(ALLFEATS) | {"all"} and table["audio"][-1] == "all"
    assert table["video"] == ["rgb_hist", "hsv_hist", "visual_variance", "absdiff", "all"]
    for m in ("rv2", "autocorrcorr"):
        assert tuple(table[m].shape) == (len(ALLFEATS) + 1, 5) and bool(torch.isfinite(table[m]).all()), table[m]
        assert float(table[m].abs().max()) <= 1 + 1e-6
