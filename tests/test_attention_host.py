"""CPU-only: what the fused attention launchers (csrc/attention.hip, csrc/attention_vjp.hip) refuse before they launch, through the
host-only maua_attention_check / maua_attention_vjp_check: the return code and the launcher's own text for every refusal, and the
shapes the networks really pass on the accepting side.  Pointers are fake (the checks never dereference them).  The method of
tests/test_modconv_host.py."""
import ctypes as C

import pytest

from maua_amd import _lib as L

F32, BF16, F16 = L.F32, L.BF16, L.F16
QKV, OUT, LSE, DOUT, DQKV, DELTA = (0x100000 * (i + 1) for i in range(6))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from maua_amd.build import build
    build()


def fwd(B=2, T=77, heads=3, D=64, dtype=BF16, **kw):
    """MAUA_OK (0), or the refusal text"""
    d = L.AttnDesc(qkv=QKV, out=OUT, lse=LSE, B=B, T=T, heads=heads, head_ch=D, ld_qkv=3 * heads * D, ld_out=heads * D, scale=0.125,
                   causal=0, dtype=dtype)
    for k, v in kw.items():
        setattr(d, k, v)
    rc = L.lib().maua_attention_check(C.byref(d))
    assert rc in (0, -1)
    return L.lib().maua_last_error().decode() if rc else 0


def vjp(B=2, T=77, heads=3, D=64, dtype=BF16, **kw):
    d = L.AttnVjpDesc(qkv=QKV, out=OUT, d_out=DOUT, lse=LSE, d_qkv=DQKV, delta=DELTA, B=B, T=T, heads=heads, head_ch=D,
                      ld_qkv=3 * heads * D, ld_out=heads * D, scale=0.125, causal=0, dtype=dtype)
    for k, v in kw.items():
        setattr(d, k, v)
    rc = L.lib().maua_attention_vjp_check(C.byref(d))
    assert rc in (0, -1)
    return L.lib().maua_last_error().decode() if rc else 0


BOTH = ((fwd, "attention"), (vjp, "attention_vjp"))


def test_return_codes():
    d = L.AttnDesc(qkv=QKV, out=OUT, B=1, T=1, heads=1, head_ch=32, ld_qkv=96, ld_out=32, scale=1.0, dtype=F32)
    assert L.lib().maua_attention_check(C.byref(d)) == 0
    d.head_ch = 48
    assert L.lib().maua_attention_check(C.byref(d)) == -1 and L.lib().maua_last_error().decode() == "attention: head channels must be 32 or 64"
    assert L.lib().maua_attention_check(None) != 0 and L.lib().maua_last_error().decode() == "maua_attention_check: desc is NULL"
    assert L.lib().maua_attention_vjp_check(None) != 0 and L.lib().maua_last_error().decode() == "maua_attention_vjp_check: desc is NULL"
    # without a context nothing is launched
    assert L.lib().maua_attention_ex(None, C.byref(d)) != 0 and L.lib().maua_last_error().decode() == "maua_attention_ex: NULL argument"
    v = L.AttnVjpDesc()
    assert L.lib().maua_attention_vjp_ex(None, C.byref(v)) != 0 and L.lib().maua_last_error().decode() == "maua_attention_vjp_ex: NULL argument"


def test_accepted_shapes():
    for f, _ in BOTH:
        # the UNet (64-channel heads, T = 64 .. 1024), both CLIP image towers (T = 50 / 197 / 257), the text tower (T = 77), f32 parity mode
        for T, heads, D in ((64, 8, 64), (1024, 4, 64), (50, 12, 64), (197, 12, 64), (257, 16, 64), (77, 8, 64), (1, 1, 32)):
            assert f(T=T, heads=heads, D=D) == 0 and f(T=T, heads=heads, D=D, dtype=F32) == 0
        assert f(B=65535, heads=65535, T=1) == 0
        assert f(B=0) == 0                                                          # nothing to do is not an error
        # padded rows: whole 16-byte pieces, 8 elements of bf16 / 4 of f32
        assert f(ld_qkv=3 * 3 * 64 + 8, ld_out=3 * 64 + 8) == 0 and f(dtype=F32, ld_qkv=3 * 3 * 64 + 4, ld_out=3 * 64 + 4) == 0
    assert fwd(lse=None) == 0 and fwd(causal=1) == 0 and fwd(lse=LSE + 4) == 0


def test_shape_refusals():
    for f, name in BOTH:
        for D in (0, 16, 48, 96, 128):
            assert f(D=D) == f"{name}: head channels must be 32 or 64"
        for dtype in (F16, L.F32_SPLIT, 7, -1):
            assert f(dtype=dtype) == f"{name}: unsupported dtype"
        assert f(T=0) == f"{name}: bad shape" and f(T=-5) == f"{name}: bad shape"
        assert f(heads=0) == f"{name}: bad shape" and f(B=-1) == f"{name}: bad shape"
        assert f(B=65536) == f"{name}: grid too large" and f(heads=65536, T=1) == f"{name}: grid too large"


def test_pointer_refusals():
    assert fwd(qkv=None) == "attention: NULL qkv / out" and fwd(out=None) == "attention: NULL qkv / out"
    for k in ("qkv", "out", "d_out", "lse", "d_qkv", "delta"):
        assert vjp(**{k: None}) == "attention_vjp: NULL argument"
    # every access is a 16-byte vector
    for off in (2, 4, 8, 12):
        assert fwd(qkv=QKV + off) == "attention: qkv / out must be 16-byte aligned"
        assert fwd(out=OUT + off) == "attention: qkv / out must be 16-byte aligned"
        for k, p in (("qkv", QKV), ("out", OUT), ("d_out", DOUT), ("d_qkv", DQKV)):
            assert vjp(**{k: p + off}) == "attention_vjp: qkv / out / d_out / d_qkv must be 16-byte aligned"
    assert fwd(lse=LSE + 2) == "attention: qkv / out must be 16-byte aligned"       # the float rows: 4 bytes
    assert vjp(lse=LSE + 2) == vjp(delta=DELTA + 1) == "attention_vjp: qkv / out / d_out / d_qkv must be 16-byte aligned"
    assert vjp(lse=LSE + 4, delta=DELTA + 8) == 0
    # B == 0 is decided after the checks: a bad descriptor is refused whatever the batch
    assert fwd(B=0, qkv=None) == "attention: NULL qkv / out"


def test_stride_refusals():
    for f, name in BOTH:
        small, piece = f"{name}: row strides below the heads' channels", f"{name}: row strides must be whole 16-byte pieces"
        assert f(ld_qkv=3 * 3 * 64 - 8) == small and f(ld_out=3 * 64 - 8) == small and f(ld_qkv=0) == small and f(ld_out=-192) == small
        assert f(ld_qkv=2 * 3 * 64, ld_out=3 * 64) == small                         # a [q | k] tensor is not a qkv tensor
        for pad in (1, 2, 4, 7, 12):
            assert f(ld_qkv=3 * 3 * 64 + pad) == piece and f(ld_out=3 * 64 + pad) == piece
        for pad in (1, 2, 3, 6):
            assert f(dtype=F32, ld_qkv=3 * 3 * 64 + pad) == piece and f(dtype=F32, ld_out=3 * 64 + pad) == piece


def test_causal_gradient_is_refused():
    assert vjp(causal=1) == "attention_vjp: no gradient of the causal forward"
    assert vjp(causal=-1, dtype=F32, D=32) == "attention_vjp: no gradient of the causal forward"
    assert vjp(causal=0) == 0
