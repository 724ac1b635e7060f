"""The strip walk of the fused up-layer kernel (csrc/modconv_tconv_fir.hip, synth option "tconv_walk" = 1) against its tile form
("tconv_walk" = 0; maua_modconv_ex: force_segs < 0) and against the register-staged two-launch path (route tconv2 + FIR pass), bit for bit.

The walk changes which workgroup computes a t value and where the FIR finds it (three t rows carried from one step of 8 position rows to
the next), not how it is summed: the K loop, the rounding of t to the storage type and the FIR / epilogue arithmetic are the tile form's.
So equality holds on ANY data, and the cases use Gaussian operands (the integer family of test_gpu_modconv.py, whose route tests now run the
walk by default, pins the same kernel to float64 references).  Guard regions around the output (Buf.check) show a stray store.

Shapes: the smallest at which each mechanism can fail - see CASES.  A strip has H / 8 + 1 steps; force_segs = 1 keeps them in one segment,
force_segs = 2 splits them (a lower segment starts with a warm-up step whose outputs are masked), 0 leaves it to the cost model."""
import sys
from pathlib import Path

import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
from maua_amd import _lib as L  # noqa: E402
from test_gpu_modconv import DTID, PROD, TFIR, Layer, R, _plan  # noqa: E402
from test_gpu_synth import build  # noqa: E402

import ctypes as C  # noqa: E402

pytestmark = pytest.mark.gpu

TILE = -1   # force_segs < 0: the tile form

# (dt, B, H, W, Ci, Co, force_segs, noise, out_scale, bias, x_bcast)
CASES = [
    # 17 position rows = steps of 8, 8, 1: the carry twice, a nearly empty last step; two strips
    ("bf16", 2, 16, 32, 32, 32, 1, "per", True, True, False),
    # odd sizes, two chunks, two channel blocks; broadcast input and noise, no bias
    ("bf16", 2, 17, 33, 64, 64, 0, "bcast", False, False, True),
    # two segments: a boundary with its warm-up step; three chunks (an odd count); three strips, the last one narrow
    ("bf16", 3, 24, 61, 96, 32, 2, None, True, True, False),
    # eight channel blocks in one XCD group; six steps in one segment
    ("bf16", 1, 40, 32, 32, 256, 1, "per", False, True, False),
    # the f16 instantiation
    ("f16", 2, 16, 32, 32, 32, 0, "bcast", True, False, False),
]


def _run(p, route, force_segs=0):
    p.y.reset()
    d = p.desc()
    L.check(L.lib().maua_modconv_ex(L.ctx(), C.byref(d), None, DTID[p.dt], R[route], force_segs, 1))
    torch.cuda.synchronize()
    p.y.check(what=f"{route} (force_segs {force_segs}) y")
    return p.y.get().view(torch.int16).clone()


@pytest.mark.parametrize("dt,B,H,W,Ci,Co,segs,noise,osc,bias,xb", [pytest.param(*c, id="-".join(map(str, c[:7]))) for c in CASES])
def test_walk_equals_tile_form_and_two_launch_path(dt, B, H, W, Ci, Co, segs, noise, osc, bias, xb):
    p = Layer(B, H, W, Ci, Co, 2, dt, epi=PROD, bias=bias, noise=noise, x_bcast=xb, out_scale=osc, family="gauss", seed=H + W)
    two = _run(p, "tconv2")
    tile = _run(p, "tconv_fir", TILE)
    walk = _run(p, "tconv_fir", segs)
    assert (two != 0).float().mean() > 0.9, "the reference output is mostly zero"
    assert torch.equal(tile, two), "the tile form differs from tconv2 + upfir"
    bad = (walk != tile).nonzero().flatten()
    where = [divmod(int(i) // Co, 2 * W) for i in bad[:4]]   # ((b * Ho + Y), X) of the first differences
    assert bad.numel() == 0, f"the walk differs from the tile form in {bad.numel()} values, first at (row, column) {where}"
    if segs:   # any other segment count gives the same bits
        assert torch.equal(_run(p, "tconv_fir", 3 - segs), tile), "the segment count changes the result"


def test_network_frames_do_not_depend_on_tconv_walk():
    """a 128^2 network whose 32^2 -> 64^2 and 64^2 -> 128^2 up-layers take the fused kernel (tconv_fir = 32): tconv_walk 0 and 1 in turn"""
    net, _ = build(128, 8192, 128, torch.bfloat16)
    g = torch.Generator().manual_seed(5)
    B = 3
    ws = torch.randn(B, net.num_ws, 64, generator=g)
    noise = [torch.randn(B, 1, s[3], s[3], generator=g) for s in net.layer_shapes()]
    h = net._handle()
    L.check(L.lib().maua_synth_set_option(h, b"tconv_fir", 32))
    assert sum(c[0] == TFIR for c in _plan(h, False)[0]) == 2, "the up-layers do not take the fused kernel"
    frames = {}
    for v in (0, 1):
        L.check(L.lib().maua_synth_set_option(h, b"tconv_walk", v))
        u8 = torch.empty((B, 128, 128, 3), dtype=torch.uint8, device="cuda")
        frames[v] = (net(ws, noise=noise).cpu(), None)
        net(ws, noise=noise, rgb8_out=u8)
        frames[v] = (frames[v][0], u8.cpu())
    assert float(frames[0][0].abs().max()) > 0
    assert torch.equal(frames[0][0], frames[1][0]) and torch.equal(frames[0][1], frames[1][1])
