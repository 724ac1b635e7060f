"""CPU-only checks of the multi-resolution image pipeline (maua_amd/image.py): the new C-ABI symbols, tests/image_pipeline_ref.py and
the host-side tables against g37 (tests/golden/make_golden_image_pipeline.py: the reference's own functions), the drop-in surface
(names, signatures, command line), and the order of operations of MultiResolutionDiffusionProcessor.forward with CPU stand-ins for the
device operators.  The operators themselves run in tests/test_gpu_image_pipeline.py."""
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
import image_pipeline_ref as H  # noqa: E402

NEW_SYMBOLS = ["maua_image_resize", "maua_image_destitch", "maua_image_restitch", "maua_image_sharpen", "maua_image_moments_slices",
               "maua_image_moments", "maua_image_match_apply", "maua_image_perlin"]
ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def g37(golden):
    g = golden("g37_image_pipeline")
    g["meta"] = json.loads(str(g["meta_json"]))
    return g


def test_new_symbols_are_declared_exported_and_counted():
    from maua_amd import _lib as L
    from maua_amd.build import build
    syms = L.declared_symbols()
    assert all(s in syms for s in NEW_SYMBOLS)
    lib = ctypes.CDLL(str(build()))
    assert all(hasattr(lib, s) for s in NEW_SYMBOLS)
    stated = re.search(r"\*\*(\d+) entry points\*\*", (ROOT / "DESIGN.md").read_text())
    assert stated and int(stated.group(1)) == len(syms), (stated and stated.group(1), len(syms))
    # every new entry cites the reference lines it replaces
    header = (ROOT / "include" / "maua_hip.h").read_text()
    block = header[header.index("image operators of the multi-resolution pipeline"):header.index("build-owned counter RNG")]
    for cite in ("diffusion/image.py:66-71", "ops/image.py:15-23", "ops/image.py:26-62", "ops/image.py:70-71", "ops/image.py:105-173",
                 "ops/noise.py:90-132"):
        assert cite in block, cite
    src = (ROOT / "maua_amd" / "csrc" / "image_ops.hip").read_text()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    assert "atomic" not in code.lower()     # gathers only: no atomics of any kind in the new kernels


def test_module_imports_and_reexports():
    import maua.diffusion.image as D
    import maua_amd.image as I
    for n in ("round64", "width_height", "build_output_name", "get_start_steps", "initialize_image", "MultiResolutionDiffusionProcessor",
              "image_sample", "get_diffusion_model"):
        assert getattr(D, n) is (getattr(I, n) if n != "get_diffusion_model" else __import__("maua_amd.diffusion").diffusion.get_diffusion_model)
    assert "out of scope" not in D.__doc__


def test_signatures_match_the_reference(g37):
    import maua_amd.image as I
    immaterial = {"diffusion"}      # annotated with a class of the reference's there
    for name, args in g37["meta"]["signatures"].items():
        obj = I.MultiResolutionDiffusionProcessor.forward if name == "forward" else getattr(I, name)
        ours = inspect.signature(obj).parameters
        names = list(ours)
        assert names[:len(args)] == [a[0] for a in args], (name, names)
        for n, d in args:
            if d is None or n in immaterial:
                continue
            if name == "forward" and n == "schedule":      # the reference's default is a set literal ({(512, 512), 0.5}): a dict here
                assert ours[n].default == {(512, 512): 0.5}
                continue
            assert ours[n].default == eval(d), (name, n, d, ours[n].default)


def test_command_line_flags_and_help(g37):
    import maua_amd.image as I
    actions = {a.option_strings[0]: a for a in I.build_parser()._actions if a.option_strings and a.option_strings[0] != "-h"}
    ref = g37["meta"]["cli"]
    assert [f for f, _, _ in ref] == list(actions)
    for flag, kw, hlp in ref:
        a = actions[flag]
        assert a.help == hlp, flag
        if "default" in kw:
            assert a.default == eval(kw["default"]), flag
        if kw.get("action") == "'store_true'":
            assert a.default is False and a.nargs == 0
        if "nargs" in kw:
            assert a.nargs == eval(kw["nargs"])
    args = I.build_parser().parse_args("--sizes 128,64 256,128 --skips 0 0.6 --stitch --super-res None".split())
    assert args.sizes == [(64, 128), (128, 256)] and args.skips == [0.0, 0.6] and args.stitch and args.super_res == "None"


def test_pure_functions(g37):
    import maua_amd.image as I
    m = g37["meta"]
    assert all(I.round64(x) == y for x, y in m["round64"])
    assert all(list(I.width_height(s)) == v for s, v in m["width_height"])
    assert all(I.build_output_name(unique=False, **kw) == name for kw, name in m["output_names"])
    assert len(I.build_output_name()) == 6

    class D:
        original_num_steps = 1000
        timestep_map = list(range(0, 1000, 20))
    assert np.array_equal(I.get_start_steps(list(g37["start_steps_skips"].numpy()), D()), g37["start_steps"].numpy())


def _cpu_destitch(img, tile_size, overtile=1):
    import maua_amd.image as I
    ys, xs = I.tile_origins(img.shape[2], tile_size, overtile), I.tile_origins(img.shape[3], tile_size, overtile)
    return torch.cat([img[..., y:y + tile_size, x:x + tile_size] for y in ys for x in xs])


def _cpu_restitch(tiled, Hh, Ww, overtile=1):
    """the arithmetic of csrc/image_ops.hip's restitch_kernel from the host tables of maua_amd.image.blend_tables"""
    import maua_amd.image as I
    T = tiled.shape[-1]
    ys, xs, wy, wx = I.blend_tables(Hh, Ww, T, overtile)
    out, norm = torch.zeros(1, 3, Hh, Ww), torch.zeros(1, 3, Hh, Ww)
    i = 0
    for r, y in enumerate(ys):
        for c, x in enumerate(xs):
            w = wy[r].reshape(1, 1, -1, 1) * wx[c].reshape(1, 1, 1, -1)
            out[..., y:y + T, x:x + T] += tiled[i] * w
            norm[..., y:y + T, x:x + T] += w
            i += 1
    return out / norm


def test_tile_tables_against_the_reference(g37):
    import maua_amd.image as I
    for name, rows, cols in (("s23", 2, 3), ("s33", 3, 3)):
        m = g37["meta"][name]
        img, T = g37[f"{name}_img"], m["T"]
        assert len(I.tile_origins(m["H"], T)) == rows and len(I.tile_origins(m["W"], T)) == cols and m["n_tiles"] == rows * cols
        assert torch.equal(_cpu_destitch(img, T), g37[f"{name}_tiles"])
        assert float((_cpu_restitch(g37[f"{name}_rnd"], m["H"], m["W"]) - g37[f"{name}_rnd_out"]).abs().max()) <= 2e-5
        back = _cpu_restitch(g37[f"{name}_tiles"], m["H"], m["W"])
        assert float((back - g37[f"{name}_back"]).abs().max()) <= 2e-5 and float((back - img).abs().max()) <= 2e-5     # partition of unity


def test_helper_against_the_fixture(g37):
    """tests/image_pipeline_ref.py where the reference's code is the source: the perlin image chain (to_pil_image, PIL's autocontrast,
    to_tensor around the reference's perlin_ms) and the resize restatement's basic properties."""
    for name in ("pc", "pg"):
        m = g37["meta"][name]
        assert torch.equal(H.perlin_image(g37[f"{name}_raw"], m["grayscale"]), g37[f"{name}_img"])
    x = torch.rand(1, 3, 20, 24, generator=torch.Generator().manual_seed(1))
    for k in (H.cubic, H.lanczos3):
        assert torch.equal(H.resize(x, out_shape=(20, 24), interp_method=k), x)
        up = H.resize(torch.ones(1, 1, 16, 16), out_shape=(40, 24), interp_method=k)
        assert float((up[..., 8:-8, 6:-6] - 1).abs().max()) < 1e-5            # weights sum to one away from the zero padding
        down = H.resize(torch.ones(1, 1, 64, 64), out_shape=(16, 32), interp_method=k)
        assert float((down[..., 3:-3, 3:-3] - 1).abs().max()) < 1e-5
    assert H.resize_tables(64, 128, H.lanczos3)[1].shape[1] == 6 and H.resize_tables(128, 64, H.lanczos3)[1].shape[1] == 12
    # the product's host tables are the same arithmetic
    import maua_amd.image as I
    for a, b, k, kn in ((64, 128, H.lanczos3, "lanczos3"), (192, 64, H.lanczos3, "lanczos3"), (4096, 64, H.cubic, "cubic"), (37, 53, H.cubic, "cubic")):
        l0, w0 = H.resize_tables(a, b, k)
        l1, w1 = I.resize_tables(a, b, kn)
        assert torch.equal(l0.int(), l1) and torch.equal(w0.float(), w1)
    u8 = (torch.rand(5, 7, 3) * 255).byte().numpy()
    assert torch.equal(H.to_tensor(u8), torch.from_numpy(u8).permute(2, 0, 1).float() / 255)
    s = H.sharpen(x * 2 - 1, 1.0)
    assert float((s - (x * 2 - 1)).abs().max()) < 1e-6                        # strength 1 leaves the image unchanged


def _apply_tables(x, left, w, dim):
    """one 1-D pass from a (left, weights) table, written without the helper's gather: a plain loop over output samples"""
    x = x.movedim(dim, -1)
    out = torch.zeros(*x.shape[:-1], left.shape[0], dtype=x.dtype)
    for o in range(left.shape[0]):
        for k in range(w.shape[1]):
            i = int(left[o]) + k
            if 0 <= i < x.shape[-1]:
                out[..., o] += float(w[o, k]) * x[..., i]
    return out.movedim(-1, dim)


def test_resize_tables_independent_checks():
    """The product's tap tables against things that do not share their text: the oracle's cubic resize (pinned through g33 / g34 by the
    reference's own cutout code), and for both kernels the properties of the published algorithm - a constant and a linear ramp are
    reproduced away from the zero padding, up and down (weights sum to one, first moment = the projected coordinate: half-pixel
    centre alignment, output sample o sits at (o + 0.5) / scale - 0.5), and a same-size resize is the identity."""
    import maua_amd.image as I
    from oracle import clip as OC
    x = torch.rand(1, 3, 24, 40, generator=torch.Generator().manual_seed(2)).double()
    for out in ((36, 64), (12, 20), (24, 17)):
        ours = x
        for dim, o in ((-2, out[0]), (-1, out[1])):
            if ours.shape[dim] != o:
                left, w = I.resize_tables(ours.shape[dim], o, "cubic")
                ours = _apply_tables(ours, left, w.double(), dim)
        assert float((ours - OC.resize(x.float(), out).double()).abs().max()) <= 2e-5, out
    for kernel, support in (("cubic", 4), ("lanczos3", 6)):
        for n_in, n_out in ((40, 100), (100, 40), (64, 128), (128, 64), (37, 53)):
            left, w = I.resize_tables(n_in, n_out, kernel)
            scale = n_out / n_in
            assert w.shape[1] == int(np.ceil(support / min(scale, 1.0) - 1e-7))
            assert float((w.sum(1) - 1).abs().max()) <= 1e-5
            centre = (torch.arange(n_out, dtype=torch.float64) + 0.5) / scale - 0.5              # half-pixel centres
            pos = (left[:, None] + torch.arange(w.shape[1])).double()
            inside = (left >= 0) & (left + w.shape[1] <= n_in)
            assert int(inside.sum()) > n_out // 2
            # in pixels of the input.  Up-scaling with cubic (a first-order exact kernel) reproduces a ramp exactly.  lanczos3 is not
            # first-order exact (its windowed sinc leaves a ripple of ~2e-2 pixel), and shrinking samples the stretched kernel at
            # 1 / scale points per unit, a quadrature and not an identity (~1e-2 pixel).  A wrong alignment convention (corner-
            # instead of centre-aligned grids) would shift every sample by 0.5 * |1 / scale - 1| >= 0.15 pixel at these sizes.
            tol = 1e-5 if kernel == "cubic" and scale > 1 else 0.03
            assert float(((w.double() * pos).sum(1) - centre)[inside].abs().max()) <= tol, (kernel, n_in, n_out)
            ramp = torch.arange(n_in, dtype=torch.float64)[None] * 0.01 + 0.3
            got = _apply_tables(ramp, left, w.double(), -1)[0]
            assert float((got - (centre * 0.01 + 0.3))[inside].abs().max()) <= 2e-5 + 0.01 * tol
        left, w = I.resize_tables(16, 16, kernel)
        eye = _apply_tables(torch.eye(16, dtype=torch.float64), left, w.double(), -1)
        assert float((eye - torch.eye(16)).abs().max()) <= 1e-6


def covariance_condition(x):
    h = x.double().permute(1, 0, 2, 3).reshape(3, -1)
    h = h - h.mean(1, keepdim=True)
    return float(torch.linalg.cond(h @ h.T / h.shape[1]))


def match_histogram_bar(g):
    """The bar of the match_histogram parity test: four times the spread between the reference's own float32 result and the same
    function in float64 on the same inputs and noise (the library reduces in a different order)."""
    spread = float((g["mh_out32"].double() - g["mh_out64"]).abs().max())
    return spread, 4 * spread


def test_match_histogram_fixture_is_well_conditioned(g37):
    for b in range(2):
        assert covariance_condition(g37["mh_target"][b:b + 1] + 1e-3 * g37["mh_noise_t"][b:b + 1]) < 1e4
        assert covariance_condition(g37["mh_source"].mean(0, keepdim=True) + 1e-3 * g37["mh_noise_s"][b:b + 1]) < 1e4
    spread, bar = match_histogram_bar(g37)
    print(f"match_histogram: reference float32 vs float64 spread {spread:.3e}, bar {bar:.3e}")
    assert 0 < spread < 1e-4
    assert torch.equal(g37["mh_identity"], g37["mh_target"])


class Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.image_size, self.device, self.calls = 64, "cpu", []

    def forward(self, img, prompts, t_start, verbose=True):
        self.calls.append(dict(shape=list(img.shape), t_start=float(t_start), prompts=[type(p).__name__ for p in prompts]))
        return img * 0.75 + 0.125


def pre_hook(x):
    return x * 0.5 - 0.1


def post_hook(x):
    return x.flip(-1) * 0.9


def run_pipeline_case(I, g37, name, stub):
    c = g37["meta"][f"pipe_{name}"]
    h, w = c["shape"][2:]
    torch.manual_seed(3704)
    return I.MultiResolutionDiffusionProcessor()(
        diffusion=stub, init="random", text="a prompt", schedule={(64, 64): 0.0, (h, w): 0.5},
        pre_hook=pre_hook if c["hooks"] else None, post_hook=post_hook if c["hooks"] else None, super_res_model=None,
        tile_size=c["tile_size"], stitch=c.get("stitch", True), max_batch=c["max_batch"], verbose=False)


PIPE_CASES = ["tile64", "six_b4", "tile64_hooks", "nostitch"]


@pytest.mark.parametrize("name", PIPE_CASES)
def test_order_of_operations_with_cpu_stand_ins(g37, monkeypatch, name):
    """MultiResolutionDiffusionProcessor.forward with the device operators replaced by CPU restatements: the calls the processor
    receives (shapes, t_start, prompt classes: ContentPrompt dropped while stitching, max_batch splitting) and the result are the
    reference's."""
    import maua_amd.image as I
    monkeypatch.setattr(I, "resize", lambda img, out_shape, interp_method="cubic": H.resize(img, out_shape=out_shape, interp_method=getattr(H, interp_method)))
    monkeypatch.setattr(I, "destitch", lambda img, tile_size: _cpu_destitch(img, tile_size))
    monkeypatch.setattr(I, "restitch", _cpu_restitch)
    monkeypatch.setattr(I, "initialize_image", lambda init, shape: torch.randn((1, 3, *shape)))
    stub = Stub()
    res = run_pipeline_case(I, g37, name, stub)
    c = g37["meta"][f"pipe_{name}"]
    assert stub.calls == c["calls"]
    if name == "six_b4":
        assert [k["shape"][0] for k in stub.calls] == [1, 4, 2] and stub.calls[1]["prompts"] == ["TextPrompt"]
    assert stub.calls[0]["prompts"] == ["ContentPrompt", "TextPrompt"]
    assert list(res.shape) == c["shape"]
    assert float((res[:, :, 1::3, ::3] - g37[f"pipe_{name}"]).abs().max()) <= 2e-5
    assert abs(float(res.double().sum()) - c["sum"]) <= 2e-5 * res.numel()


def test_refusals_name_what_they_refuse():
    import maua_amd.image as I
    with pytest.raises(NotImplementedError, match="SwinIR-M-DFO-GAN"):
        I.image_sample(sizes=[(64, 64)], skips=[0.0])                         # the reference's default super_res, before anything is built
    with pytest.raises(NotImplementedError, match="SwinIR"):
        I.MultiResolutionDiffusionProcessor()(Stub(), "random", schedule={(64, 64): 0.0}, super_res_model="SwinIR-M-DFO-GAN", verbose=False)
    for other in ("stable", "latent", "glide", "glid3xl"):
        with pytest.raises(NotImplementedError, match=other):
            I.image_sample(diffusion=other, super_res=None)
    assert I.check_super_res("None") is None and I.check_super_res(None) is None and I.check_super_res("x4plus") == "x4plus"
    with pytest.raises(NotImplementedError, match='mode="hist"'):
        I.match_histogram(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), mode="hist")
    t = torch.zeros(1, 3, 4, 4)
    assert I.match_histogram(t, t, mode="False") is t
    with pytest.raises(AssertionError, match="equal length"):
        I.image_sample(diffusion=Stub(), super_res=None, sizes=[(64, 64)], skips=[0.0, 0.5])

    class Net:
        channel_mult = (1, 1, 2, 2, 4, 4, 8, 8)          # 8 levels: multiples of 128 only
    stub = Stub()
    stub.model = Net()
    with pytest.raises(ValueError, match="192x64"):
        I.check_sizes(stub, [(128, 128), (64, 192)], 128, False)
    with pytest.raises(ValueError, match="tile size 64"):
        I.check_sizes(stub, [(128, 128), (256, 256)], 64, True)
    I.check_sizes(stub, [(128, 128), (256, 384)], 128, True)
    with pytest.raises(ValueError, match="rounds to nothing"):
        I.MultiResolutionDiffusionProcessor()(Stub(), "random", schedule={(20, 64): 0.0}, verbose=False)
    with pytest.raises(ValueError, match="interp_method"):
        I.resize(torch.zeros(1, 3, 4, 4), (8, 8), interp_method="box")


def test_image_prompt_takes_arrays_as_to_tensor_does(tmp_path):
    from PIL import Image
    from maua_amd.grad import ContentPrompt, ImagePrompt, StylePrompt
    rng = np.random.default_rng(0)
    u8 = rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    want = (H.to_tensor(u8).unsqueeze(0) * 2 - 1).clamp(-1, 1)
    assert torch.equal(ImagePrompt(img=u8).img, want) and tuple(want.shape) == (1, 3, 5, 7)
    assert torch.equal(ImagePrompt(img=Image.fromarray(u8)).img, want)
    f = tmp_path / "p.png"
    Image.fromarray(u8).save(f)
    for cls in (ImagePrompt, StylePrompt, ContentPrompt):
        assert torch.equal(cls(path=str(f)).img, want)
    fl = rng.random((5, 7, 3), dtype=np.float32)
    assert torch.equal(ImagePrompt(img=fl).img, torch.from_numpy(fl).permute(2, 0, 1).unsqueeze(0) * 2 - 1)
    t = torch.rand(2, 3, 4, 4)
    assert torch.equal(ImagePrompt(img=t).img, t * 2 - 1)                   # tensors as before
    assert torch.equal(ImagePrompt(img=t.numpy()).img, t * 2 - 1)           # ... and 4-D arrays, taken as [B, C, H, W] values
    with pytest.raises(Exception, match="path or img"):
        ImagePrompt()


def test_perlin_gradient_draws_follow_the_reference(g37):
    """perlin_gradients draws with the reference's call shapes and order: a seeded generator reproduces the recorded gradients."""
    import maua_amd.image as I
    for name in ("pc", "pg"):
        m = g37["meta"][name]
        torch.manual_seed(3702)
        ours = I.perlin_gradients(list(g37[f"{name}_octaves"].numpy()), m["width"], m["height"], m["grayscale"])
        assert len(ours) == m["n_grads"]
        assert all(torch.equal(o, g37[f"{name}_grad{k:02d}"]) for k, o in enumerate(ours))
