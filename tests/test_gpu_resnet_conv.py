"""The kernels of the ResNet backbone (csrc/resnet_conv.hip) one operation at a time, against exact references.

Convolutions: inputs are integers in [-4, 4], weights in [-2, 2], bias and residual small integers, so every product and every partial
sum is an integer below 2^24 - exact in float32 in any order - and the one rounding of the store (bfloat16: nearest even of an exact
integer) is a function of the value alone.  The result must therefore EQUAL the float64 CPU convolution, rounded once to the storage type,
bit for bit in both dtypes.  Max-pool picks input values and the average pool of integers is an exact sum times one float32 factor: exact
too.  Shapes: every (k, stride) form and the stem; odd sizes (5x7 -> 3x4, 9x6 -> 5x3, 1x1); one and several channel tiles; and two
shapes large enough (>= 256 tiles of 128 x 128) to take the 128 x 128 tile instead of the 64 x 64 one.
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
FORMS = [(1, 1, 0), (1, 2, 0), (3, 1, 1), (3, 2, 1)]


@pytest.fixture(scope="module")
def L():
    from maua_amd import _lib
    _lib.require_device()
    return _lib


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def nhwc(t, dtype):
    return t.permute(0, 2, 3, 1).contiguous().to(dtype).cuda()


def run_conv(L, x_dev, w, bias, res_dev, shape, k, stride, pad, relu, dtype, out_shape, y=None):
    B, H, W, Ci, Co = shape
    wd, bd = w.float().contiguous().cuda(), None if bias is None else bias.float().cuda()
    if y is None:
        y = torch.full(out_shape, -77.0, dtype=dtype, device="cuda")
    d = L.SConvDesc(x=x_dev.data_ptr(), w=wd.data_ptr(), bias=0 if bd is None else bd.data_ptr(), res=0 if res_dev is None else res_dev.data_ptr(),
                    y=y.data_ptr(), B=B, H=H, W=W, Ci=Ci, Co=Co, k=k, stride=stride, pad=pad, relu=int(relu))
    rc = L.lib().maua_conv_strided_ex(L.ctx(), ctypes.byref(d), L.dtype_id(dtype) if isinstance(dtype, torch.dtype) else dtype)
    torch.cuda.synchronize()
    return rc, y


def check_conv(L, g, dtype, B, H, W, Ci, Co, k, stride, pad, with_res, relu):
    x, w, bias = ints(g, (B, Ci, H, W), -4, 4), ints(g, (Co, Ci, k, k), -2, 2), ints(g, (Co,), -3, 3)
    want = F.conv2d(x, w, bias, stride, pad)
    res = ints(g, tuple(want.shape), -5, 5) if with_res else None
    if with_res:
        want = want + res
    if relu:
        want = want.clamp_min(0)
    assert float(want.abs().max()) < 2 ** 24
    Ho, Wo = want.shape[2:]
    assert (Ho, Wo) == ((H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1)
    rc, y = run_conv(L, nhwc(x, dtype), w, bias, None if res is None else nhwc(res, dtype), (B, H, W, Ci, Co), k, stride, pad, relu, dtype,
                     (B, Ho, Wo, Co))
    assert rc == 0, L.lib().maua_last_error()
    assert torch.equal(y.cpu(), want.permute(0, 2, 3, 1).to(dtype)), (dtype, (B, H, W, Ci, Co), (k, stride), with_res, relu)


@pytest.mark.parametrize("hw", [(5, 7), (9, 6), (1, 1)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("form", FORMS, ids=lambda f: f"k{f[0]}s{f[1]}")
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_conv_forms_are_exact(L, dt, form, hw):
    g = torch.Generator().manual_seed(100 * form[0] + 10 * form[1] + hw[0])
    for ci, co in ((64, 64), (128, 256)):
        for with_res in (False, True):
            for relu in (False, True):
                check_conv(L, g, DTYPES[dt], 2, hw[0], hw[1], ci, co, *form, with_res, relu)


@pytest.mark.parametrize("case", [(2, 91, 91, 64, 256, 3, 1, 1), (2, 181, 181, 64, 256, 1, 2, 0)], ids=["k3s1", "k1s2"])
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_conv_wide_tile_is_exact(L, dt, case):
    """2 x 91 x 91 output pixels = 130 row tiles of 128, times two channel tiles: the 128 x 128 route, with a ragged last row tile"""
    B, H, W, ci, co, k, stride, pad = case
    assert -(-(B * 91 * 91) // 128) * (co // 128) >= 256
    check_conv(L, torch.Generator().manual_seed(7), DTYPES[dt], B, H, W, ci, co, k, stride, pad, True, True)


@pytest.mark.parametrize("hw", [(9, 11), (40, 56)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_stem_is_exact(L, dt, hw):
    dtype, g = DTYPES[dt], torch.Generator().manual_seed(hw[0])
    B, (H, W) = 2, hw
    x, w, bias = ints(g, (B, 3, H, W), -4, 4), ints(g, (64, 3, 7, 7), -2, 2), ints(g, (64,), -3, 3)
    for relu in (False, True):
        want = F.conv2d(F.pad(x, (1, 1, 1, 1)), w, bias, 2, 2)      # ConstantPad2d(1, 0) + padding 2: a zero border of 3
        assert tuple(want.shape[2:]) == ((H - 1) // 2 + 1, (W - 1) // 2 + 1)
        want = want.clamp_min(0) if relu else want
        rc, y = run_conv(L, x.float().contiguous().cuda(), w, bias, None, (B, H, W, 3, 64), 7, 2, 3, relu, dtype,
                         (B, want.shape[2], want.shape[3], 64))
        assert rc == 0, L.lib().maua_last_error()
        assert torch.equal(y.cpu(), want.permute(0, 2, 3, 1).to(dtype))


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_maxpool_is_exact(L, dt):
    dtype, g = DTYPES[dt], torch.Generator().manual_seed(5)
    for B, H, W, C in ((2, 5, 7, 64), (2, 9, 6, 8), (3, 1, 1, 64), (2, 20, 28, 64)):
        x = torch.randn((B, C, H, W), generator=g).to(dtype)
        x[0] = -x[0].abs() - 0.5      # a sample of negative values only: a border tap counted as zero would win every window
        want = F.max_pool2d(x.float(), 3, 2, 1)
        y = torch.full((B, want.shape[2], want.shape[3], C), 55.0, dtype=dtype, device="cuda")
        assert L.lib().maua_maxpool3x3s2(L.ctx(), L.ptr(nhwc(x, dtype)), L.ptr(y), B, H, W, C, L.dtype_id(dtype)) == 0, L.lib().maua_last_error()
        assert torch.equal(y.cpu().float(), want.permute(0, 2, 3, 1)) and float(y[0].max()) < 0


@pytest.mark.parametrize("dt", sorted(DTYPES))
def test_global_avgpool_is_exact(L, dt):
    dtype, g = DTYPES[dt], torch.Generator().manual_seed(6)
    for B, H, W, C in ((2, 2, 2, 2048), (3, 7, 7, 64), (2, 3, 4, 8), (1, 1, 1, 64)):
        x = ints(g, (B, C, H, W), -8, 8)
        out = torch.full((B, C), 9.0, dtype=torch.float32, device="cuda")
        assert L.lib().maua_global_avgpool(L.ctx(), L.ptr(nhwc(x, dtype)), L.ptr(out), B, H, W, C, L.dtype_id(dtype)) == 0, L.lib().maua_last_error()
        want = x.sum(dim=(2, 3)).float() * (torch.ones((), dtype=torch.float32) / torch.tensor(float(H * W), dtype=torch.float32))
        assert torch.equal(out.cpu(), want)


def test_refused_shapes_launch_nothing(L):
    g = torch.Generator().manual_seed(8)
    lib = L.lib()
    x = nhwc(ints(g, (2, 64, 6, 6), -4, 4), torch.float32)
    w5, w3, w1 = (ints(g, (64, 64, k, k), -2, 2) for k in (5, 3, 1))
    y = torch.full((2, 6, 6, 64), -77.0, device="cuda")
    refusals = [((2, 6, 6, 64, 64), w5, 5, 1, 2, torch.float32, "must be"),                 # no such kernel size
                ((2, 6, 6, 64, 64), w3, 3, 3, 1, torch.float32, "must be"),                 # no such stride
                ((2, 6, 6, 64, 64), w3, 3, 1, 0, torch.float32, "must be"),                 # 3x3 without its padding
                ((2, 6, 6, 64, 64), w1, 1, 1, 1, torch.float32, "must be"),                 # 1x1 with padding
                ((2, 6, 6, 32, 64), w1, 1, 1, 0, torch.float32, "Ci must be a multiple of 64"),
                ((2, 6, 6, 64, 96), w1, 1, 1, 0, torch.float32, "Co must be a multiple of 64"),
                ((2, 6, 6, 64, 64), w1, 7, 2, 3, torch.float32, "stem"),                    # the stem form with 64 input channels
                ((2, 6, 6, 64, 64), w3, 3, 1, 1, L.F16, "conv_strided: unsupported dtype"),
                ((2, 6, 6, 64, 64), w3, 3, 1, 1, L.F32_SPLIT, "conv_strided: unsupported dtype")]
    for shape, w, k, stride, pad, dtype, message in refusals:
        rc, _ = run_conv(L, x, w, None, None, shape, k, stride, pad, True, dtype, None, y=y)
        assert rc != 0 and message in lib.maua_last_error().decode(), (k, stride, pad, lib.maua_last_error())
        assert bool((y == -77.0).all())
    img = ints(g, (2, 3, 6, 6), -4, 4).float().cuda()
    rc, _ = run_conv(L, img, ints(g, (64, 3, 7, 7), -2, 2), None, y, (2, 6, 6, 3, 64), 7, 2, 3, True, torch.float32, None, y=y)
    assert rc != 0 and "no residual" in lib.maua_last_error().decode() and bool((y == -77.0).all())
    for fn, out in ((lib.maua_maxpool3x3s2, y), (lib.maua_global_avgpool, y)):
        assert fn(L.ctx(), L.ptr(x), L.ptr(out), 2, 6, 6, 12, L.F32) != 0 and "multiple of 8" in lib.maua_last_error().decode()
        assert fn(L.ctx(), L.ptr(x), L.ptr(out), 2, 6, 6, 64, L.F16) != 0 and "unsupported dtype" in lib.maua_last_error().decode()
        assert bool((y == -77.0).all())
