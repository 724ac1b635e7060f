"""The SwAV ResNet-50 extractor without a device: the float64 restatement (tests/swav_ref.py) against what the reference's own network
returned (tests/golden/g42_swav.npz), the BatchNorm fold, the checkpoint loader, the extractor spellings and the shims, and the network
the library builds against the state dict."""
import ctypes
import io
import pickle
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent))
import swav_ref as SR  # noqa: E402

from maua_amd import _lib as L  # noqa: E402
from maua_amd import metrics as M  # noqa: E402
from maua_amd import resnet as R  # noqa: E402
from maua_amd.load import load_state_dict_file  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "g42_swav.npz"


@pytest.fixture(scope="module")
def fx():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def test_restatement_reproduces_the_reference(fx):
    layers = tuple(int(n) for n in fx["layers"])
    sd = SR.make_state_dict(int(fx["seed"]), layers)
    taps, feats = SR.forward(sd, torch.from_numpy(fx["x"]), layers)
    want = torch.from_numpy(fx["feat_f64"])
    assert feats.dtype == torch.float64 and feats.shape == want.shape == (2, 2048)
    assert float((feats - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert [tuple(t.shape[1:]) for t in taps] == [(64, 20, 28), (64, 10, 14), (256, 10, 14), (512, 5, 7), (1024, 3, 4), (2048, 2, 2)]
    assert np.allclose([float(t.abs().max()) for t in taps], fx["tap_max"], rtol=1e-12, atol=0)
    # the reference's own float32 error is what a float32 evaluation of the same operations loses: a few 1e-7 of each tap's largest value
    assert (fx["tap_err"] / fx["tap_max"] < 2e-6).all() and (fx["tap_err"] > 0).all()


def test_weight_checksums(fx):
    layers = tuple(int(n) for n in fx["layers"])
    sums = SR.checksums(SR.make_state_dict(int(fx["seed"]), layers))
    assert sorted(sums) == [str(k) for k in fx["sum_keys"]]
    assert np.array_equal(np.array([sums[k] for k in sorted(sums)]), fx["sums"])
    assert len(sums) == 5 * len(SR.conv_names(layers))


def test_bn_fold_equals_conv_then_bn():
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, 8, 9, 7), generator=g, dtype=torch.float64)
    w = torch.randn((12, 8, 3, 3), generator=g, dtype=torch.float64)
    gamma, var = torch.rand(12, generator=g, dtype=torch.float64) + 0.5, torch.rand(12, generator=g, dtype=torch.float64) + 0.5
    beta, mean = torch.randn(12, generator=g, dtype=torch.float64), torch.randn(12, generator=g, dtype=torch.float64)
    want = F.batch_norm(F.conv2d(x, w, None, 2, 1), mean, var, gamma, beta, False, 0.0, 1e-5)
    s = gamma / torch.sqrt(var + 1e-5)
    got = F.conv2d(x, w * s.reshape(-1, 1, 1, 1), beta - mean * s, 2, 1)
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    wf, bf = R.fold_bn(w, gamma, beta, mean, var)      # the library's fold: the same values, rounded once to float32
    assert wf.dtype == bf.dtype == torch.float32
    assert torch.equal(wf, (w * s.reshape(-1, 1, 1, 1)).float()) and torch.equal(bf, (beta - mean * s).float())


def test_loader_round_trip(tmp_path):
    layers = (1, 1, 1, 1)
    sd = SR.make_state_dict(5, layers)
    saved = {"module." + k: v for k, v in sd.items()}
    saved["module.bn1.num_batches_tracked"] = torch.tensor(3)
    saved["module.projection_head.0.weight"] = torch.zeros(4, 4)
    saved["module.prototypes.weight"] = torch.zeros(4, 4)
    for name, kw in (("zip.pth.tar", {}), ("legacy.pth.tar", {"_use_new_zipfile_serialization": False})):
        torch.save(saved, tmp_path / name, **kw)
        got = R.clean_state_dict(load_state_dict_file(tmp_path / name))
        assert sorted(got) == sorted(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    torch.save({"state_dict": saved}, tmp_path / "wrapped.pth")
    assert sorted(R.clean_state_dict(load_state_dict_file(tmp_path / "wrapped.pth"))) == sorted(sd)
    assert [c for c, _ in R.conv_names(layers)] == [c for c, *_ in SR.conv_names(layers)]


class _Foreign:
    def __reduce__(self):
        return (eval, ("1 + 1",))


def test_loader_refuses_a_foreign_global(tmp_path):
    bare = tmp_path / "bare.pkl"
    bare.write_bytes(pickle.dumps({"conv1.weight": _Foreign()}))
    with pytest.raises(ValueError, match="eval"):
        load_state_dict_file(bare)
    zipped = tmp_path / "zip.pth"
    torch.save({"conv1.weight": torch.zeros(2), "hook": _Foreign()}, zipped)
    with pytest.raises(ValueError, match="refused"):
        load_state_dict_file(zipped)
    legacy = tmp_path / "legacy.pth"
    torch.save({"hook": _Foreign()}, legacy, _use_new_zipfile_serialization=False)
    with pytest.raises(ValueError, match="refused"):
        load_state_dict_file(legacy)
    buf = io.BytesIO()
    pickle.dump([1, 2], buf)
    (tmp_path / "list.pkl").write_bytes(buf.getvalue())
    with pytest.raises(ValueError, match="not a state dict"):
        load_state_dict_file(tmp_path / "list.pkl")


def test_extractor_spellings_parser_and_shims(monkeypatch):
    made = []

    class Fake:
        def __init__(self, checkpoint, dtype=torch.float32, allow_random_init=False):
            made.append((checkpoint, dtype, allow_random_init))

    monkeypatch.setattr(R, "SwAV", Fake)
    ex, size, name = M.get_extractor("SwAV:/some/where/swav.pth.tar")
    assert isinstance(ex, Fake) and (size, name) == (224, "SwAV") and made[-1] == ("/some/where/swav.pth.tar", torch.float32, False)
    ex, size, name = M.get_extractor("SwAV-bf16:w.pth", allow_random_init=True)
    assert (size, name) == (224, "SwAV") and made[-1] == ("w.pth", torch.bfloat16, True)
    M.get_extractor("SwAV:random", allow_random_init=True)
    assert made[-1] == ("random", torch.float32, True)
    for bare in ("SwAV", "Inception"):
        with pytest.raises(NotImplementedError, match=bare):
            M.get_extractor(bare)
    with pytest.raises(NotImplementedError, match="SwAV:<checkpoint>"):
        M.get_extractor("SwAV")
    with pytest.raises(ValueError, match="SwAV-f16"):
        M.get_extractor("SwAV-f16:w.pth")
    args = M.parser().parse_args(["--data_dir", "d", "--checkpoint", "g.pt", "--extractor", "SwAV:swav.pth.tar"])
    assert args.extractor == "SwAV:swav.pth.tar" and M.parser().parse_args(["--data_dir", "d", "--checkpoint", "c"]).extractor == "SwAV"
    monkeypatch.undo()
    with pytest.raises(FileNotFoundError, match="not bundled"):
        R.SwAV.__init__(object.__new__(R.SwAV), "random")      # refused before anything touches a device
    import maua.GAN.metrics.extractors as ext
    import maua.GAN.metrics.extractors.swav as shim
    import maua.GAN.metrics.compute as c
    assert ext.get_extractor is M.get_extractor is c.get_extractor and shim.SwAV is R.SwAV and shim.ResNetFeatures is R.ResNetFeatures


def test_library_network_agrees_with_the_state_dict():
    from maua_amd.build import build
    build()
    layers = (3, 4, 6, 3)
    shapes = R.conv_shapes(layers)
    names = SR.conv_names(layers)
    assert len(shapes) == len(names) == 53 == len(R.conv_names(layers))
    sd = SR.make_state_dict(1, (1, 1, 1, 1))
    for (conv, bn, ci, co, k), (lci, lco, lk, stride), (rconv, rbn) in zip(names, shapes, R.conv_names(layers)):
        assert (ci, co, k) == (lci, lco, lk) and (conv, bn) == (rconv, rbn), conv
        m = re.fullmatch(r"layer([234])\.0\.(conv2|downsample\.0)", conv)
        assert stride == (2 if m or conv == "conv1" else 1), conv
        if conv + ".weight" in sd:
            assert tuple(sd[conv + ".weight"].shape) == (co, ci, k, k)
    # refusals of the shape-only object: no context, nothing to load into or run
    lib, net = L.lib(), ctypes.c_void_p()
    assert lib.maua_resnet_create(None, L.F32, (ctypes.c_int * 4)(1, 1, 1, 1), 64, ctypes.byref(net)) == 0
    assert lib.maua_resnet_conv_count(net) == 17
    assert lib.maua_resnet_load(net, 0, 1, (ctypes.c_float * 64)(), 64) != 0 and b"without a context" in lib.maua_last_error()
    lib.maua_resnet_destroy(net)
    for bad in ((0, 1, 1, 1), ):
        assert lib.maua_resnet_create(None, L.F32, (ctypes.c_int * 4)(*bad), 64, ctypes.byref(net)) != 0
    assert lib.maua_resnet_create(None, L.F16, (ctypes.c_int * 4)(1, 1, 1, 1), 64, ctypes.byref(net)) != 0
    assert lib.maua_resnet_create(None, L.F32, (ctypes.c_int * 4)(1, 1, 1, 1), 48, ctypes.byref(net)) != 0


def test_sconv_desc_mirror_follows_the_header():
    raw = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "maua_hip.h").read_text(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+maua_sconv_desc\s*\{([^}]*)\}\s*maua_sconv_desc\s*;", raw).group(1)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        first, *rest = decl.split(",")
        ctype, field = re.fullmatch(r"(.*?)(\w+)", first.strip()).groups()
        fields.append((field, L.ctype_of(ctype, "maua_sconv_desc")))
        fields += [(more.strip(), L.ctype_of(ctype, "maua_sconv_desc")) for more in rest]
    assert list(L.SConvDesc._fields_) == fields
