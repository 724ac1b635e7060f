"""Latent directions and the Jacobi solver, without a device: the tournament schedule of maua_jacobi_schedule against
tests/decomp_ref.py's table; that restatement against LAPACK on the very matrices tests/test_gpu_decomposition.py runs on the device
(so the inputs and the bounds are honest before a GPU is involved); every refusal of the *_check entries by its text; the C ABI's
symbols and count; the reference's module paths; Directions' .npz round trip; the command line; and how cff stacks the affine weights."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import decomp_ref as R  # noqa: E402

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["maua_jacobi_schedule", "maua_svd_f64_workspace_bytes", "maua_svd_f64_check", "maua_svd_f64", "maua_eigh_f64_workspace_bytes",
               "maua_eigh_f64_check", "maua_eigh_f64", "maua_latent_add_directions_check", "maua_latent_add_directions"]


def lib():
    from maua_amd import _lib as L
    return L.lib()


def msg(rc):
    assert rc != 0
    return lib().maua_last_error().decode()


# ------------------------------------------------------------------------------------------------------------------ the schedule
def c_schedule(n, rnd):
    N = n + (n & 1)
    pairs, count = (ctypes.c_int * (2 * N))(), ctypes.c_int()
    assert lib().maua_jacobi_schedule(n, rnd, pairs, ctypes.byref(count)) == 0
    return [(pairs[2 * i], pairs[2 * i + 1]) for i in range(count.value)]


@pytest.mark.parametrize("n", list(range(1, 10)) + [16, 17, 33])
def test_schedule_is_the_tournament(n):
    seen = []
    for rnd in range(R.rounds(n)):
        got = c_schedule(n, rnd)
        assert got == R.schedule(n, rnd), (n, rnd)
        flat = [x for pair in got for x in pair]
        assert len(set(flat)) == len(flat) and all(0 <= x < n for x in flat), "the pairs of a round are disjoint columns"
        assert len(got) == n // 2, "an odd n leaves exactly one column out of every round, an even n none"
        seen += [tuple(sorted(pair)) for pair in got]
    assert sorted(seen) == [(p, q) for p in range(n) for q in range(p + 1, n)], "every unordered pair exactly once per sweep"


def test_schedule_refusals():
    one, cnt = (ctypes.c_int * 8)(), ctypes.c_int()
    assert "1 .. 4096" in msg(lib().maua_jacobi_schedule(0, 0, one, ctypes.byref(cnt)))
    assert "N - 1 rounds" in msg(lib().maua_jacobi_schedule(4, 3, one, ctypes.byref(cnt)))
    assert "N - 1 rounds" in msg(lib().maua_jacobi_schedule(3, 3, one, ctypes.byref(cnt)))
    assert "NULL" in msg(lib().maua_jacobi_schedule(4, 0, None, ctypes.byref(cnt)))


# ------------------------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", list(R.matrices()))
def test_restatement_meets_the_device_bounds_against_lapack(name):
    A = R.matrices()[name]
    U, S, V, sweeps, rotated = R.svd(A)
    assert sweeps <= R.MAX_SWEEPS and rotated == 0, (sweeps, rotated)
    figures = R.svd_figures(A, U, S, V, sweeps)
    print(name, sweeps, figures)
    assert all(v <= 1.0 for v in figures.values()), figures
    assert R.sign_rule_holds(V)
    assert (np.diff(S) <= 0).all()
    if name in R.ONE_SWEEP:
        assert sweeps == 1
    if name == R.ZERO_COLUMN:
        assert S[-1] == 0.0 and not U[:, -1].any()


@pytest.mark.parametrize("name", list(R.eigh_matrices()))
def test_restatement_eigh_against_lapack(name):
    S = R.eigh_matrices()[name]
    w, Q, sweeps, rotated = R.eigh(S)
    figures = R.eigh_figures(S, w, Q, sweeps)
    print(name, sweeps, figures)
    assert rotated == 0 and figures.pop("ascending") and all(v <= 1.0 for v in figures.values()), figures
    assert R.sign_rule_holds(Q)


def test_fma32_is_libm_fmaf():
    """the restatement's fused multiply-add against libm's, on products whose float64 sum is inexact as well"""
    libm = ctypes.CDLL("libm.so.6")
    libm.fmaf.restype, libm.fmaf.argtypes = ctypes.c_float, [ctypes.c_float] * 3
    g = np.random.RandomState(5)
    a, b = g.randn(4000).astype(np.float32), g.randn(4000).astype(np.float32)
    c = (g.randn(4000) * 10.0 ** g.randint(-12, 3, 4000)).astype(np.float32)
    got = R.fma32(a, b, c)
    want = np.array([libm.fmaf(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------------------------ refusals
def test_every_check_refusal_by_its_text():
    from maua_amd import _lib as L
    from maua_amd import decomposition as D
    l, one = lib(), ctypes.c_void_p(256)
    big = 1 << 40
    ok = lambda **kw: l.maua_svd_f64_check(*[kw.get(k, d) for k, d in (("a", one), ("m", 8), ("n", 4), ("lda", 4), ("want_u", 1), ("path", 0),
                                                                       ("max_sweeps", 0), ("ws", one), ("ws_bytes", big), ("s", one),
                                                                       ("u", one), ("v", one))])
    assert ok() == 0 and ok(want_u=0, u=None) == 0 and ok(path=1) == 0 and ok(path=2, max_sweeps=30) == 0
    assert "m must be at least n" in msg(ok(m=3))
    assert "n must be at least 1" in msg(ok(n=0))
    assert "at most 4096 columns" in msg(ok(m=5000, n=4097, lda=4097))
    assert "leading dimension" in msg(ok(lda=3))
    assert "path must be" in msg(ok(path=3))
    assert "max_sweeps" in msg(ok(max_sweeps=31))
    assert "NULL" in msg(ok(a=None)) and "want_u needs u" in msg(ok(u=None))
    need = l.maua_svd_f64_workspace_bytes(8, 4)
    assert need > 0 and ok(ws_bytes=need) == 0
    assert "workspace" in msg(ok(ws_bytes=need - 1)) and "workspace" in msg(ok(ws=ctypes.c_void_p(264)))
    # path 1 keeps (m + n) n doubles in one workgroup's LDS: 96 x 96 is the largest square that fits, 200 x 96 does not
    assert ok(m=96, n=96, lda=96, path=1) == 0
    assert "does not fit" in msg(ok(m=200, n=96, lda=96, path=1)) and ok(m=200, n=96, lda=96, path=0) == 0
    assert l.maua_svd_f64_workspace_bytes(3, 4) == 0 and l.maua_svd_f64_workspace_bytes(4, 0) == 0
    assert l.maua_eigh_f64_workspace_bytes(64) == l.maua_svd_f64_workspace_bytes(64, 64)
    assert l.maua_eigh_f64_check(one, 8, 8, 0, 0, one, big, one, one) == 0
    assert "maua_eigh_f64: n must be at least 1" in msg(l.maua_eigh_f64_check(one, 0, 8, 0, 0, one, big, one, one))
    assert "maua_eigh_f64_workspace_bytes" in msg(l.maua_eigh_f64_check(one, 8, 8, 0, 0, one, 16, one, one))
    assert "does not fit" in msg(l.maua_eigh_f64_check(one, 200, 200, 1, 0, one, big, one, one))
    # the Python layer: the same text through svd_check, and some=False by name before a device is asked for
    with pytest.raises(L.MauaHipError, match="does not fit"):
        D.svd_check(200, 96, path="resident")
    with pytest.raises(L.MauaHipError, match="workspace"):
        D.svd_check(8, 4, ws_bytes=16)
    with pytest.raises(NotImplementedError, match="some=False"):
        D.svd(torch.zeros(4, 3), some=False)
    # the latent kernel
    chk = l.maua_latent_add_directions_check
    assert chk(one, one, one, 3, 6, 512, 5, 0, 6, one) == 0 and chk(one, None, None, 3, 6, 512, 0, 0, 6, one) == 0
    assert chk(one, None, None, 3, 6, 512, 5, 4, 4, one) == 0
    assert "bad shape" in msg(chk(one, one, one, 3, 0, 512, 5, 0, 6, one))
    assert "layer range" in msg(chk(one, one, one, 3, 6, 512, 5, 0, 7, one)) and "layer range" in msg(chk(one, one, one, 3, 6, 512, 5, -1, 6, one))
    assert "NULL" in msg(chk(one, None, one, 3, 6, 512, 5, 0, 6, one)) and "NULL" in msg(chk(None, one, one, 3, 6, 512, 5, 0, 6, one))


def test_workspace_sizes_are_pinned():
    """A^T [n][m even], V [n][n even], sigma, sign, shift, row sums, order, rotation counters, info: every piece rounded up to 256 bytes"""
    l = lib()
    up = lambda b: (b + 255) // 256 * 256

    def want(m, n):
        mp, np_, N = m + (m & 1), n + (n & 1), n + (n & 1)
        return up(n * mp * 8) + up(n * np_ * 8) + 3 * up(n * 8) + up(8) + up(n * 4) + up(N // 2 * 4) + up(8)
    for m, n, pinned in ((1, 1, 2304), (65, 33, 29440), (6048, 512, 26885632), (4096, 4096, 268558848)):
        assert l.maua_svd_f64_workspace_bytes(m, n) == want(m, n) == pinned
    assert l.maua_eigh_f64_workspace_bytes(2048) == want(2048, 2048) == 67170816
    assert l.maua_svd_f64_workspace_bytes(4097, 4097) == 0 and l.maua_eigh_f64_workspace_bytes(0) == 0


def test_refusals_that_existed_before_still_refuse():
    """this pull request adds the solver; the callers that name its absence keep refusing until they are moved onto it"""
    from maua_amd import metrics
    with pytest.raises(NotImplementedError, match="singular value decomposition"):
        metrics.symsqrtm(torch.eye(3))


# ------------------------------------------------------------------------------------------------------------------ the C ABI
def test_new_symbols_are_declared_exported_and_counted():
    from maua_amd import _lib as L
    from maua_amd.build import build
    syms = L.declared_symbols()
    assert all(s in syms for s in NEW_SYMBOLS)
    so = ctypes.CDLL(str(build()))
    assert all(hasattr(so, s) for s in NEW_SYMBOLS)
    stated = re.search(r"\*\*(\d+) entry points\*\*", (ROOT / "DESIGN.md").read_text())
    assert stated and int(stated.group(1)) == len(syms), (stated and stated.group(1), len(syms))
    header = (ROOT / "include" / "maua_hip.h").read_text()
    assert "sefa.py:7,25" in header, "the entries cite the reference lines they serve"


def test_reexports_resolve():
    import maua.GAN.decomposition as pkg
    import maua.GAN.decomposition.sefa as ref_sefa
    import maua_amd.audiovisual.audioreactive as ar
    from maua_amd import decomposition as D
    from maua_amd import latent as LT
    assert ref_sefa.cff is D.cff and ref_sefa.apply_sefa is D.apply_sefa
    assert pkg.cff is D.cff and pkg.svd is D.svd and pkg.eigh is D.eigh and pkg.ganspace is D.ganspace and pkg.Directions is D.Directions
    assert ar.direction_modulate is LT.direction_modulate


# ------------------------------------------------------------------------------------------------------------------ Python layer
def test_directions_round_trip(tmp_path):
    from maua_amd import decomposition as D
    g = torch.Generator().manual_seed(3)
    d = D.Directions(torch.randn(4, 64, generator=g), torch.rand(4, generator=g), torch.randn(64, generator=g), "ganspace",
                     dict(n_samples=2048, seed=7, truncation=0.7))
    back = D.load(d.save(tmp_path / "d.npz"))
    assert torch.equal(back.vectors, d.vectors) and torch.equal(back.values, d.values) and torch.equal(back.mean, d.mean)
    assert back.method == "ganspace" and back.source == d.source and len(back) == 4
    plain = D.load(D.Directions(d.vectors, d.values).save(tmp_path / "e.npz"))
    assert plain.mean is None and plain.method == "sefa" and plain.source == {}


def test_cli_arguments():
    from maua_amd import decomposition as D
    a = D.parser().parse_args(["--model_file", "None", "--method", "ganspace", "--num_axes", "4", "--out", "d.npz", "--grid", "g.png", "--seeds", "1,2",
                               "--max_variation", "2.5", "--num_cols", "5", "--layers", "0-5", "--out_size", "32,32"])
    assert (a.model_file, a.method, a.num_axes, a.out, a.grid, a.seeds, a.max_variation, a.num_cols) == ("None", "ganspace", 4, "d.npz", "g.png", "1,2", 2.5, 5)
    d = D.parser().parse_args(["--model_file", "x.pt", "--out", "d.npz"])
    assert (d.method, d.num_axes, d.grid, d.layers, d.num_cols, d.max_variation) == ("sefa", 8, None, None, 7, 3.0)
    assert D.parse_layers("0-5") == [0, 1, 2, 3, 4, 5] and D.parse_layers("0,2,4-5") == [0, 2, 4, 5] and D.parse_layers(None) is None
    for bad in (["--out", "d.npz"], ["--model_file", "x"], ["--model_file", "x", "--out", "d", "--method", "pca"]):
        with pytest.raises(SystemExit):
            D.parser().parse_args(bad)


def test_cff_stacks_the_conv_affines_in_layer_order():
    from maua_amd import decomposition as D
    from maua_amd.load import synthetic_rosinality_checkpoint
    from maua_amd.stylegan2 import SynthesisNetwork
    net = SynthesisNetwork(64, 32, 3, channel_base=1024, channel_max=48, generator=torch.Generator().manual_seed(0))
    sd = net.state_dict()
    keys = ["bs.0.conv1", "bs.1.conv0", "bs.1.conv1", "bs.2.conv0", "bs.2.conv1", "bs.3.conv0", "bs.3.conv1"]
    by_hand = torch.cat([sd[k + ".affine.weight"] for k in keys], 0)
    assert [k for k, _ in D.affine_weights(net)] == [k + ".affine.weight" for k in keys]
    assert all(tuple(w.shape) == (sd[k.replace("affine.weight", "weight")].shape[1], 64) for k, w in D.affine_weights(net)), "[C_in, w_dim] each"
    W = D.stacked_weight(net)
    assert W.shape[1] == 64 and torch.equal(W, by_hand)
    assert torch.equal(D.stacked_weight(sd), W) and torch.equal(D.stacked_weight({"synthesis." + k: v for k, v in sd.items()}), W)
    assert torch.equal(D.stacked_weight(net, layers=range(1, 3)), torch.cat([sd[k + ".affine.weight"] for k in keys[1:3]], 0))
    with_rgb = [k for k, _ in D.affine_weights(net, include_torgb=True)]
    assert with_rgb[:3] == ["bs.0.conv1.affine.weight", "bs.0.torgb.affine.weight", "bs.1.conv0.affine.weight"] and len(with_rgb) == 11
    # a rosinality state dict: conv1, convs.0, convs.1, ... in that order, to_rgb1 / to_rgbs left out
    ros = synthetic_rosinality_checkpoint(res=16)["g_ema"]
    want = torch.cat([ros["conv1.conv.modulation.weight"]] + [ros[f"convs.{i}.conv.modulation.weight"] for i in range(4)], 0)
    assert torch.equal(D.stacked_weight(ros), want) and torch.equal(D.stacked_weight({"g_ema": ros}), want)
    from maua_amd.load import rosinality_to_nvidia
    assert torch.equal(D.stacked_weight(rosinality_to_nvidia({"g_ema": ros}, for_inference=True)[0]), want), "both key spellings give the same W"
    with pytest.raises(KeyError, match="no style-affine weights"):
        D.stacked_weight({"a": torch.zeros(1)})
