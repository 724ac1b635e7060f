"""CPU-only checks of the optical-flow video pipeline (maua_amd/flow.py, maua_amd/video_diffusion.py): the new C-ABI symbols, the drop-in
surface against g38 (tests/golden/make_golden_video.py: the reference's own functions), tests/flow_ref.py against g38, the order of
operations of VideoFlowDiffusionProcessor.forward with CPU stand-ins for the device operators, the frame sources, the refusals, and the
restated estimator against a flow known in closed form.  The operators themselves run in tests/test_gpu_video_pipeline.py."""
import ctypes
import inspect
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flow_ref as FR  # noqa: E402

NEW_SYMBOLS = ["maua_flow_warp", "maua_flow_consistency", "maua_flow_resize_bilinear", "maua_flow_compose", "maua_flow_turbo",
               "maua_farneback_levels", "maua_farneback_create", "maua_farneback_destroy", "maua_farneback_pair"]
ROOT = Path(__file__).resolve().parent.parent
SHIFT = (1.5, -0.75)
FB_SIZES = [(80, 96), (45, 70)]          # (rows, cols): five pyramid levels; two levels, odd sizes


@pytest.fixture(scope="module")
def g38(golden):
    g = golden("g38_video_pipeline")
    g["meta"] = json.loads(str(g["meta_json"]))
    return g


_fb_cache = {}


def farneback_references(rows, cols):
    """The known-shift pair of this size and the restatement's flows of it in float32 and float64, both directions (computed once)."""
    key = (rows, cols)
    if key not in _fb_cache:
        a, b = FR.sinusoid_pair(rows, cols)
        _fb_cache[key] = dict(a=a, b=b, ab32=FR.farneback(a, b), ab64=FR.farneback(a, b, torch.float64), ba32=FR.farneback(b, a),
                              ba64=FR.farneback(b, a, torch.float64))
    return _fb_cache[key]


def farneback_bar(rows, cols):
    """The bar of the device estimator's parity test: four times the largest difference between the restatement in float32 and in
    float64 on the same inputs (the match_histogram precedent)."""
    r = farneback_references(rows, cols)
    spread = max(float((r["ab32"].double() - r["ab64"]).abs().max()), float((r["ba32"].double() - r["ba64"]).abs().max()))
    return spread, 4 * spread


def test_new_symbols_are_declared_exported_and_counted():
    from maua_amd import _lib as L
    from maua_amd.build import build
    syms = L.declared_symbols()
    assert all(s in syms for s in NEW_SYMBOLS)
    lib = ctypes.CDLL(str(build()))
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    stated = re.search(r"\*\*(\d+) entry points\*\*", (ROOT / "DESIGN.md").read_text())
    assert stated and int(stated.group(1)) == len(syms), (stated and stated.group(1), len(syms))
    header = (ROOT / "include" / "maua_hip.h").read_text()
    block = header[header.index("optical-flow operators of the video pipeline"):header.index("build-owned counter RNG")]
    for cite in ("flow/lib.py:51-63", "diffusion/video.py:161-162", "flow/consistency.py:78-127", "diffusion/video.py:153-157",
                 "diffusion/video.py:248-277", "diffusion/video.py:221-238", "flow/__init__.py:35-55"):
        assert cite in block, cite
    src = (ROOT / "maua_amd" / "csrc" / "flow.hip").read_text()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.lower()     # gathers only


def test_module_imports_and_reexports():
    import maua.diffusion.video as V
    import maua.flow as MF
    import maua.flow.lib as ML
    import maua_amd.flow as F
    import maua_amd.video_diffusion as VD
    for n in ("VideoFrames", "FramesOnDisk", "initialize_cache_files", "initialize_optical_flow", "VideoFlowDiffusionProcessor", "video_sample",
              "build_parser", "main"):
        assert getattr(V, n) is getattr(VD, n)
    for n in ("get_flow_model", "flow_warp_map", "get_consistency_map", "check_consistency"):
        assert getattr(MF, n) is getattr(F, n)
    for n in ("encode_mflo", "decode_mflo", "flow_warp_map", "get_consistency_map"):
        assert getattr(ML, n) is getattr(F, n)
    assert V.warp is F.warp and "maua.diffusion.video" in __import__("maua").__doc__ and "maua.flow" in __import__("maua").__doc__


def test_signatures_and_flags_match_the_reference(g38):
    import maua_amd.video_diffusion as VD
    immaterial = {"diffusion"}
    for name, args in g38["meta"]["signatures"].items():
        obj = VD.VideoFlowDiffusionProcessor.forward if name == "forward" else getattr(VD, name, None)
        if obj is None:
            import maua_amd.flow as F
            obj = getattr(F, name)
        ours = inspect.signature(obj).parameters
        assert list(ours)[:len(args)] == [a[0] for a in args], (name, list(ours))
        for n, d in args:
            if d is not None and n not in immaterial:
                assert ours[n].default == eval(d), (name, n, d, ours[n].default)
    assert {"forward", "video_sample"} <= set(g38["meta"]["signatures"])
    actions = {a.option_strings[0]: a for a in VD.build_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    ref = g38["meta"]["cli"]
    assert [f for f, _, _ in ref] == list(actions)
    for flag, kw, hlp in ref:
        a = actions[flag]
        assert a.help == hlp, flag
        if "default" in kw:
            assert a.default == eval(kw["default"]), flag
        if kw.get("action") == "'store_true'":
            assert a.default is False and a.nargs == 0
    args = VD.build_parser().parse_args("--size 128,64 --turbo 3 --hist-persist".split())
    assert args.size == (64, 128) and args.turbo == 3 and args.hist_persist


def test_flow_ref_reproduces_the_fixture(g38):
    import maua_amd.flow as F
    for name in ("wm57", "wm129"):
        assert float((FR.flow_warp_map(g38[f"{name}_flow"]) - g38[f"{name}_map"]).abs().max()) <= 1e-6
        assert float((F.flow_warp_map(g38[f"{name}_flow"]) - g38[f"{name}_map"]).abs().max()) <= 1e-6
    populated = dict(boundary=0, missed=0, overshoot=0)
    for name in ("smooth", "edge", "out"):
        fwd, bwd = g38[f"cc_{name}_fwd"], g38[f"cc_{name}_bwd"]
        assert float((FR.check_consistency(fwd, bwd) - g38[f"cc_{name}_map"]).abs().max()) <= 1e-6
        _, masks = FR.consistency_classes(fwd, bwd)
        for k in populated:
            populated[k] += int(masks[k].sum())
        exclude, frac = FR.near_threshold(fwd, bwd)
        assert frac <= float(exclude.float().mean()) <= 0.005, (name, frac)          # the fixture's flows keep clear of the thresholds
    assert all(v > 0 for v in populated.values()) and populated == g38["meta"]["cc_populated"]


def test_mflo_round_trips_are_bit_equal(g38):
    import maua_amd.flow as F
    for name in ("mf_a", "mf_b"):
        enc = F.encode_mflo(g38[f"{name}_flow"].numpy())
        assert enc.dtype == np.uint8 and np.array_equal(enc, g38[f"{name}_enc"].numpy())
        assert np.array_equal(F.decode_mflo(enc), g38[f"{name}_dec"].numpy())


class Stub(torch.nn.Module):
    def __init__(self, log):
        super().__init__()
        self.log = log

    def forward(self, img, prompts, t_start, verbose=True):
        self.log.append(["forward", float(t_start), [type(p).__name__ for p in prompts]])
        return img * 0.75 + 0.125


PIPE_CASES = ["t1", "t3", "t1w2", "t3w2", "t3w2_first", "t1_hist", "t3w2_notrust"]


def cpu_stand_ins(monkeypatch, VD, log, n_frames=5, size=64):
    """The device operators and file sources of maua_amd.video_diffusion replaced by CPU restatements and the fixture's stub sources."""
    frames, flows, cons, first = FR.pipe_inputs(n_frames, size)

    class Frames:
        def __init__(self, filename, height, width, device):
            pass

        def __len__(self):
            return n_frames

        def __getitem__(self, idx):
            return frames[idx].clone()

    class Prompt:
        def __init__(self, *a, path=None, size=None, **k):
            self.img = first.clone()

    def fill(cache, *a, **k):
        for i in range(n_frames):
            cache.flow.items[i], cache.consistency.items[i] = flows[i], cons[i]

    real_insert = VD.FramesOnDisk.insert

    def insert(self, item, idx=None):
        if self.basename.endswith("frame"):
            log.append(["insert", "frame", int(idx if idx is not None else len(self))])
        real_insert(self, item, idx)

    def compose(frame, prev=None, flow=None, consistency=None, cached=None, flow_exaggeration=1.0, consistency_trust=0.75, blend=2.0, fade=1.0,
                noise_injection=0.0, seed=0):
        assert noise_injection == 0.0
        return FR.compose(frame, prev, flow, consistency, cached, flow_exaggeration, consistency_trust, blend, fade, 0.0, None)

    monkeypatch.setattr(VD, "VideoFrames", Frames)
    monkeypatch.setattr(VD, "initialize_optical_flow", fill)
    monkeypatch.setattr(VD.FramesOnDisk, "insert", insert)
    monkeypatch.setattr(VD, "compose", compose)
    monkeypatch.setattr(VD, "turbo_step", lambda p, n, f, e, w, b: FR.turbo(p, n, f, e, w, torch.tensor(b)))
    monkeypatch.setattr(VD, "match_histogram", lambda a, b: (log.append(["match_histogram"]), a * 0.9 + 0.1 * b.mean())[1])
    for cls in ("ContentPrompt", "StylePrompt", "ImagePrompt"):
        monkeypatch.setattr(VD, cls, type(cls, (Prompt,), {}))
    monkeypatch.setattr(VD, "TextPrompt", type("TextPrompt", (), {"__init__": lambda self, text: None}))


@pytest.mark.parametrize("name", PIPE_CASES)
def test_order_of_operations_with_cpu_stand_ins(g38, monkeypatch, name):
    """VideoFlowDiffusionProcessor.forward with CPU stand-ins: the sequence of sampler calls (skip, prompt kinds), histogram matches
    and frame-cache inserts (index), and the frames, are the reference's up to the point where it raises (see the generator)."""
    import maua_amd.video_diffusion as VD
    c = g38["meta"][f"pipe_{name}"]
    log = []
    cpu_stand_ins(monkeypatch, VD, log)
    video = VD.VideoFlowDiffusionProcessor()(diffusion=Stub(log), init="clip.mp4", text="a prompt", style="style.png", size=(64, 64),
                                             noise_injection=0.0, constant_seed=7, device="cpu", flow_exaggeration=1.5, **c["kwargs"])
    assert log == c["log"]
    assert c["raised"] and any(e[0] == "forward" for e in log)
    assert [e[1] for e in log if e[0] == "forward"][:2] == [0.4, 0.7]
    assert list(video.shape) == c["shape"]
    assert float((video[:, :, 1::4, ::4] - g38[f"pipe_{name}"]).abs().max()) <= 2e-5
    assert abs(float(video.double().sum()) - c["sum"]) <= 2e-5 * video.numel()


def test_video_frames_sources(tmp_path):
    from PIL import Image
    import maua_amd.video_diffusion as VD
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (3, 8, 12, 3), dtype=np.uint8)
    d = tmp_path / "clip"
    d.mkdir()
    for i, f in enumerate(u8):
        Image.fromarray(f).save(d / f"f{i:03d}.png")
    want = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(127.5).sub(1)
    np.save(tmp_path / "clip.npy", u8)
    for src in (str(d), str(d / "*.png"), str(tmp_path / "clip.npy"), u8, torch.from_numpy(u8).permute(0, 3, 1, 2)):
        fr = VD.VideoFrames(src, 8, 12, "cpu")
        assert len(fr) == 3 and tuple(fr[1].shape) == (1, 3, 8, 12) and torch.equal(fr[1], want[1:2]) and torch.equal(fr[-1], want[2:3])
    (tmp_path / "notes.txt").write_text("not a video")
    with pytest.raises(RuntimeError, match="directory or glob of image files"):
        VD.VideoFrames(str(tmp_path / "missing.mp4"), 8, 12, "cpu")
    with pytest.raises(ValueError, match="uint8"):
        VD.VideoFrames(np.zeros((2, 8, 12, 3), dtype=np.float32), 8, 12, "cpu")


def test_frames_on_disk_interface(tmp_path):
    import maua_amd.video_diffusion as VD
    c = VD.FramesOnDisk(str(tmp_path / "frame"), "cpu")
    a, b = torch.rand(1, 3, 4, 4), torch.rand(1, 3, 4, 4)
    c.insert(a)
    c.insert(b)
    c.insert(a * 2, 0)
    assert len(c) == 3 and torch.equal(c[0], a * 2) and torch.equal(c[[0, 1]], torch.cat([a * 2, b]))
    assert torch.equal(c.finalize(), torch.cat([a * 2, b]))
    with pytest.raises(IndexError):
        c[5]
    # persist: the reference's files, read back by a new object
    p = VD.FramesOnDisk(str(tmp_path / "flow"), "cpu", persist=True)
    flow = FR.pipe_inputs(1, 64)[1][0] * 0 + torch.stack(torch.meshgrid(torch.linspace(-4, 4, 64), torch.linspace(-3, 3, 64), indexing='ij'), -1)[None]
    p.insert(flow)
    p.finalize()
    q = VD.FramesOnDisk(str(tmp_path / "flow"), "cpu", persist=True)
    assert len(q) == 1 and tuple(q[0].shape) == (1, 64, 64, 2) and float((q[0] - flow).abs().max()) < 0.5      # 8-bit JPEG of the .mflo code
    q.finalize()


def test_unsupported_models_and_processors_raise_by_name():
    import maua_amd.flow as F
    import maua_amd.video_diffusion as VD
    for name in ("raft/raft_8x2_100k_mixed_368x768", "pwc", "unflow", "spynet", "liteflownet", "deepflow2"):
        with pytest.raises(NotImplementedError, match=re.escape(name)):
            F.get_flow_model([name])
    with pytest.raises(NotImplementedError, match="numpy"):
        F.get_consistency_map(torch.zeros(1, 4, 4, 2), torch.zeros(1, 4, 4, 2), "numpy")
    for other in ("stable", "latent", "glide", "glid3xl"):
        with pytest.raises(NotImplementedError, match=other):
            VD.video_sample(other, "clip.mp4")


@pytest.mark.parametrize("rows,cols", FB_SIZES)
def test_restated_estimator_recovers_a_known_flow(rows, cols):
    """tests/flow_ref.py's Farneback on a sum of low-frequency sinusoids and its analytically shifted copy (no interpolation in the
    inputs): away from a 16-pixel border the mean endpoint error stays below half the smaller shift component - a
    flipped sign, swapped axes or a missed 1 / pyr_scale between levels each leave at least 0.75 px.  Also prints the float32 / float64
    spread that sets the device test's bar."""
    r = farneback_references(rows, cols)
    border = 16
    assert FR.pyramid_levels(rows, cols) + 1 == (5 if rows >= 80 else 2)
    for k, shift in (("ab", SHIFT), ("ba", (-SHIFT[0], -SHIFT[1]))):
        for prec in ("32", "64"):
            epe = FR.endpoint_error(r[k + prec], shift, border)
            print(f"farneback restatement {cols}x{rows} {k} float{prec}: mean endpoint error {epe:.4f} px")
            assert epe < 0.375
    spread, bar = farneback_bar(rows, cols)
    print(f"farneback restatement {cols}x{rows}: float32 vs float64 max abs {spread:.3e}, device bar {bar:.3e}")
    assert 0 < spread < 1e-3


def run_noise_case(monkeypatch, constant_seed, **kw):
    """The processor with injected noise and CPU stand-ins that log: every Philox key draw (the real ``torch.randint``), every compose
    call (what it blends and whether it adds noise), ``pre_hook`` and ``match_histogram`` (which, like the library's, draws its own key)."""
    import maua_amd.flow as F
    import maua_amd.video_diffusion as VD
    log = []
    cpu_stand_ins(monkeypatch, VD, log, n_frames=3)

    def draw():
        key = F.draw_noise_key()
        log.append(["key", key])
        return key

    def compose(frame, prev=None, flow=None, consistency=None, cached=None, flow_exaggeration=1.0, consistency_trust=0.75, blend=2.0, fade=1.0,
                noise_injection=0.0, seed=0):
        log.append(["compose", prev is not None, float(noise_injection), seed])
        g = torch.Generator().manual_seed(seed % (2 ** 31))
        return FR.compose(frame, prev, flow, consistency, cached, flow_exaggeration, consistency_trust, blend, fade, noise_injection,
                          torch.randn(frame.shape, generator=g))

    def match(a, b):
        log.append(["match_histogram", int(torch.randint(0, 2 ** 62, ()))])
        return a * 0.9 + 0.1 * b.mean()

    monkeypatch.setattr(VD, "draw_noise_key", draw)
    monkeypatch.setattr(VD, "compose", compose)
    monkeypatch.setattr(VD, "match_histogram", match)
    torch.manual_seed(5)
    video = VD.VideoFlowDiffusionProcessor()(diffusion=Stub(log), init="clip.mp4", size=(64, 64), noise_injection=0.02, constant_seed=constant_seed,
                                             device="cpu", **kw)
    return [e for e in log if e[0] != "insert"], video


def test_noise_is_one_launch_without_hooks_and_a_second_one_behind_them(monkeypatch):
    """Where the noise goes (diffusion/video.py:271-277: pre_hook, hist_persist, noise): with no hook between fade and noise the key is
    drawn and the one composition adds the noise; with ``pre_hook`` or ``hist_persist`` the composition adds none, the hooks run, then the
    key is drawn - after match_histogram's own draw - and a second compose adds the noise alone."""
    log, video = run_noise_case(monkeypatch, None)
    kinds = [e[0] for e in log]
    assert kinds == ["key", "compose", "forward"] * 3 and bool(torch.isfinite(video).all())
    for key, comp in zip(log[0::3], log[1::3]):
        assert comp == ["compose", True, 0.02, key[1]]
    assert len({e[1] for e in log if e[0] == "key"}) == 3                     # a new key per frame ...
    log7, video7 = run_noise_case(monkeypatch, 7)
    assert len({e[1] for e in log7 if e[0] == "key"}) == 1                    # ... and the same one under constant_seed
    assert torch.equal(run_noise_case(monkeypatch, 7)[1], video7)

    hooked = []
    log, _ = run_noise_case(monkeypatch, 7, hist_persist=True, pre_hook=lambda x: (hooked.append(1), x * 0.5)[1])
    per_frame, frame = [], []
    for e in log:
        frame.append(e)
        if e[0] == "forward":
            per_frame.append(frame)
            frame = []
    assert len(per_frame) == 3 and len(hooked) == 3
    assert [e[0] for e in per_frame[0]] == ["compose", "key", "compose", "forward"]                        # f_n == 0: no histogram match yet
    for fr in per_frame[1:]:
        assert [e[0] for e in fr] == ["compose", "match_histogram", "key", "compose", "forward"]
        assert fr[0][1:3] == [True, 0.0] and fr[3] == ["compose", False, 0.02, fr[2][1]]
        assert fr[1][1] != fr[2][1]                                            # two draws of the same generator, in this order
    # hist_persist alone: frame 0 is the one-launch form, later frames the two-launch one
    log, _ = run_noise_case(monkeypatch, 7, hist_persist=True)
    kinds = [e[0] for e in log]
    assert kinds == ["key", "compose", "forward"] + ["compose", "match_histogram", "key", "compose", "forward"] * 2


def test_persist_writes_the_cache_and_leaves_no_thread(monkeypatch, tmp_path):
    import threading
    import maua_amd.video_diffusion as VD
    monkeypatch.chdir(tmp_path)
    log = []
    cpu_stand_ins(monkeypatch, VD, log, n_frames=3)
    video = VD.VideoFlowDiffusionProcessor()(diffusion=Stub(log), init="clip.mp4", size=(64, 64), noise_injection=0.0, device="cpu", persist=True)
    assert tuple(video.shape) == (3, 3, 64, 64)
    assert not [t for t in threading.enumerate() if isinstance(t, VD.WriteThread)]       # frame, flow and consistency writers all ended
    assert sorted(p.name for p in (tmp_path / "workspace" / "clip_video").glob("frame*.jpg")) == ["frame0.jpg", "frame1.jpg", "frame2.jpg"]

    class Boom(Stub):
        def forward(self, *a, **k):
            raise RuntimeError("sampler failed")
    with pytest.raises(RuntimeError, match="sampler failed"):
        VD.VideoFlowDiffusionProcessor()(diffusion=Boom(log), init="clip.mp4", size=(64, 64), device="cpu", persist=True, noise_injection=0.0)
    assert not [t for t in threading.enumerate() if isinstance(t, VD.WriteThread)]


FFMPEG_STAND_IN = '''#!{python}
"""stands in for ffmpeg in the tests: "decodes" a .npy of frames into the PPM stream the frame reader asks for"""
import sys
import numpy as np
args = sys.argv[1:]
src = args[args.index("-i") + 1]
assert args[args.index("-f") + 1] == "image2pipe" and args[args.index("-vcodec") + 1] == "ppm" and args[-1] == "-"
if src.endswith("broken.mp4"):
    sys.stderr.write("moov atom not found")
    sys.exit(1)
for f in np.load(src.replace(".mp4", ".npy")):
    sys.stdout.buffer.write(b"P6\\n%d %d\\n255\\n" % (f.shape[1], f.shape[0]) + f.tobytes())
'''


def test_video_file_through_an_ffmpeg_executable_alone(monkeypatch, tmp_path):
    """The video-file route with a stand-in ``ffmpeg`` on PATH (and nothing else: no ffprobe): the PPM pipe carries the frame size."""
    import os
    import maua_amd.video_diffusion as VD
    bindir = tmp_path / "bin"
    bindir.mkdir()
    exe = bindir / "ffmpeg"
    exe.write_text(FFMPEG_STAND_IN.format(python=sys.executable))
    exe.chmod(0o755)
    monkeypatch.setenv("PATH", str(bindir))
    u8 = np.random.default_rng(1).integers(0, 256, (4, 10, 14, 3), dtype=np.uint8)
    np.save(tmp_path / "clip.npy", u8)
    (tmp_path / "clip.mp4").write_bytes(b"not really a video")
    fr = VD.VideoFrames(str(tmp_path / "clip.mp4"), 10, 14, "cpu")
    assert len(fr) == 4 and torch.equal(fr.data, torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(127.5).sub(1))
    (tmp_path / "broken.mp4").write_bytes(b"x")
    with pytest.raises(RuntimeError, match="moov atom not found"):
        VD.VideoFrames(str(tmp_path / "broken.mp4"), 10, 14, "cpu")
    with pytest.raises(RuntimeError, match="truncated"):
        VD._parse_ppm_stream(b"P6\n4 4\n255\n" + bytes(10), "a test")
    monkeypatch.setenv("PATH", str(tmp_path / "nowhere"))
    with pytest.raises(RuntimeError, match="ffmpeg executable is on PATH"):
        VD.VideoFrames(str(tmp_path / "clip.mp4"), 10, 14, "cpu")


def test_main_maps_the_flags_onto_video_sample(monkeypatch, tmp_path):
    import maua_amd.video_diffusion as VD
    seen, takes = {}, set(inspect.signature(VD.video_sample).parameters)
    monkeypatch.setattr(VD, "video_sample", lambda **kw: (seen.update(kw), torch.zeros(2, 3, 64, 64))[1])
    monkeypatch.setattr(VD, "write_video", lambda video, path, fps, value_range: seen.update(path=path, fps=fps, value_range=value_range, n=video.shape[0]))
    monkeypatch.delenv("MAUA_ALLOW_RANDOM_INIT", raising=False)
    VD.main(["--diffusion", "guided", "--init", "in/clip.mp4", "--text", "a fox", "--size", "128,64", "--turbo", "2", "--fps", "24",
             "--out-dir", str(tmp_path / "out"), "--constant-seed", "3"])
    assert seen["diffusion"] == "guided" and seen["sampler"] == "plms" and seen["size"] == (64, 128) and seen["turbo"] == 2
    assert seen["constant_seed"] == 3 and seen["skip"] == 0.85 and "out_dir" not in seen
    assert "guided_kwargs" not in seen
    assert seen["path"] == f"{tmp_path / 'out'}/guided_clip_a_fox_{seen['path'].split('_')[-1]}" and seen["path"].endswith(".mp4")
    assert seen["fps"] == 24 and seen["value_range"] == (-1, 1) and seen["n"] == 2 and (tmp_path / "out").is_dir()
    # every keyword main passes is one video_sample takes
    assert set(seen) - {"path", "fps", "value_range", "n"} <= takes
    monkeypatch.setenv("MAUA_ALLOW_RANDOM_INIT", "1")
    VD.main(["--diffusion", "guided", "--init", "clip.mp4", "--out-dir", str(tmp_path / "out")])
    assert seen["guided_kwargs"] == dict(allow_random_init=True)
