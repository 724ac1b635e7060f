"""CPU-only side of the GroupNorm parity tests.

1. What the fused GroupNorm launchers (csrc/groupnorm.hip launch_group_norm, csrc/groupnorm_vjp.hip launch_group_norm_vjp) refuse before
   they launch, through the host-only maua_group_norm_check / maua_group_norm_vjp_check: return code and the launcher's own text for
   every refusal; the shapes the 256 and 512 px networks pass on the accepting side; the plan queries' answers at the route and
   chunk edges.  Pointers are fake (the checks never dereference them).  The method of tests/test_attention_host.py.
2. The proofs tests/test_gpu_groupnorm.py's exact family relies on, for the very inputs it uses (tests/groupnorm_ref.py generates
   them from the case's seed): group sums are exact, the mean is the intended power of two, `q / cnt - mean * mean` gives the same
   float32 rstd whether it is rounded twice or contracted into one fma; every fma of the apply pass has a float64-exact argument (so
   the float64 -> float32 rounding of the emulation IS the fma's rounding), the emulation equals an exact rational evaluation, and
   does not depend on contracting `beta - mean * ca`; float32 tile sums of the exact inputs are exact; the exact gradient's means are
   exact; and for the Gaussian family the reference taken from float32 tile sums stays inside the piece-sum bound."""
import ctypes as C
import sys
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import groupnorm_ref as R  # noqa: E402

F32, BF16, F16 = L.F32, L.BF16, L.F16
X0, X1, GAMMA, BETA, SS, Y, XR, PS0, PS1, STATS, DY, DRES, ADD0, ADD1, DX0, DX1 = (0x100000 * (i + 1) for i in range(16))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from maua_amd.build import build
    build()


def _err(rc):
    assert rc in (0, -1)
    return L.lib().maua_last_error().decode() if rc else 0


def fdesc(B=2, H=8, W=8, C0=256, C1=0, dtype=BF16, **kw):
    d = L.GnDesc(x0=X0, C0=C0, x1=X1 if C1 else None, C1=C1, B=B, H=H, W=W, gamma=GAMMA, beta=BETA, ss=None, ss_ld=0, silu=1, mode=0,
                 y=Y, xr=None, ps0=None, rows0=0, ps1=None, rows1=0, stats_out=None, force_route=0, dtype=dtype)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def fwd(**kw):
    """MAUA_OK (0), or the refusal text"""
    return _err(L.lib().maua_group_norm_check(C.byref(fdesc(**kw))))


def plan(**kw):
    """(route, RY, ppc, nchunk, stats_source), or the refusal text"""
    o = [C.c_int(-1) for _ in range(5)]
    e = _err(L.lib().maua_group_norm_plan(C.byref(fdesc(**kw)), *[C.byref(t) for t in o]))
    return e if e else tuple(t.value for t in o)


def vdesc(B=2, H=8, W=8, C0=256, C1=0, dtype=BF16, **kw):
    d = L.GnVjpDesc(x0=X0, C0=C0, x1=X1 if C1 else None, C1=C1, stats=STATS, gamma=GAMMA, beta=BETA, ss=None, ss_ld=0, silu=1, mode=0,
                    dy=DY, dres=None, add0=None, add1=None, dx0=DX0, dx1=DX1 if C1 else None, B=B, H=H, W=W, dtype=dtype)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def vjp(**kw):
    return _err(L.lib().maua_group_norm_vjp_check(C.byref(vdesc(**kw))))


def vplan(**kw):
    """(RY, ppc, nchunk, ranges), or the refusal text"""
    o = [C.c_int(-1) for _ in range(4)]
    e = _err(L.lib().maua_group_norm_vjp_plan(C.byref(vdesc(**kw)), *[C.byref(t) for t in o]))
    return e if e else tuple(t.value for t in o)


BOTH = ((fwd, "group_norm"), (vjp, "group_norm_vjp"))
PIECES = ": C % 32 == 0, at most 1024 16-byte pieces per pixel"
ALIGN = ": pointers and ss_ld must be whole 16-byte pieces"
PSUM = "group_norm: piece sums need H % 8 == 0, W % 32 == 0, C % 128 == 0 of their source and rows == (H / 8) * (W / 32)"


def test_return_codes():
    l = L.lib()
    for name in ("maua_group_norm_check", "maua_group_norm_vjp_check", "maua_group_norm_plan", "maua_group_norm_vjp_plan"):
        args = (None,) + (None,) * {"maua_group_norm_plan": 5, "maua_group_norm_vjp_plan": 4}.get(name, 0)
        assert getattr(l, name)(*args) == -1 and l.maua_last_error().decode() == f"{name}: desc is NULL"
    # without a context nothing is launched
    assert l.maua_group_norm_ex(None, C.byref(fdesc())) == -1 and l.maua_last_error().decode() == "maua_group_norm_ex: NULL argument"
    assert l.maua_group_norm_vjp_ex(None, C.byref(vdesc())) == -1 and l.maua_last_error().decode() == "maua_group_norm_vjp_ex: NULL argument"
    # the plan queries accept NULL outputs
    assert l.maua_group_norm_plan(C.byref(fdesc()), None, None, None, None, None) == 0
    assert l.maua_group_norm_vjp_plan(C.byref(vdesc()), None, None, None, None) == 0


def test_refusals_shared():
    for f, n in BOTH:
        assert f() == 0
        for dt in (F16, 3, -1, 7):
            assert f(dtype=dt) == f"{n}: unsupported dtype"
        for k in ("x0", "gamma", "beta"):
            assert f(**{k: None}) == f"{n}: NULL argument"
        for k in ("B", "H", "W", "C0", "C1"):
            assert f(**{k: -1}) == f"{n}: bad shape"
        assert f(H=0) == f(W=0) == f(C0=0, C1=256) == f"{n}: bad shape"
        assert f(B=0) == 0
        assert f(C0=48) == f(C0=16) == f(C0=260) == n + PIECES                              # C % 32
        assert f(C0=8192) == 0 and f(C0=8224) == n + PIECES                                 # bf16: 1024 / 1028 pieces
        assert f(C0=4096, dtype=F32) == 0 and f(C0=4100, dtype=F32) == n + PIECES           # PPP = 1025
        assert f(C0=4128, dtype=F32) == n + PIECES
        assert f(C0=100, C1=156, dtype=F32) == 0 and f(C0=200, C1=312) == 0                 # a group across the boundary is legal
        assert f(C0=100, C1=156) == f(C0=98, C1=158, dtype=F32) == n + PIECES               # C0 % EPC
        for m in (-1, 3, 100):
            assert f(mode=m) == f"{n}: bad resample mode"
        assert f(mode=1) == f(mode=2) == 0
        t = f": ss_ld is 0 (one row for all samples) or at least 2 C"
        assert f(ss=SS, ss_ld=0) == f(ss=SS, ss_ld=512) == f(ss=SS, ss_ld=576) == 0
        assert f(ss=SS, ss_ld=508) == f(ss=SS, ss_ld=-512) == f(ss=SS, ss_ld=256) == n + t
        assert f(ss=None, ss_ld=8) == 0                                                      # (unused without ss)
        assert f(ss=SS, ss_ld=514) == n + ALIGN
        for k in ("x0", "gamma", "beta", "ss"):
            assert f(**{"ss": SS, "ss_ld": 512, k: X0 + 8}) == n + ALIGN
        assert f(B=65535) == 0 and f(B=65536) == f"{n}: grid too large"
        assert f(H=65536, W=32768) == f"{n}: grid too large"


def test_refusals_forward():
    n = "group_norm"
    assert fwd(y=None) == f"{n}: NULL argument"
    assert fwd(C0=128, C1=128, x1=None) == f"{n}: x1 is NULL with C1 > 0"
    assert fwd(C0=128, C1=128) == 0
    # mode 1 floors like avg_pool2d; one row or column would give an empty grid
    assert fwd(mode=1, H=5, W=7) == 0 and fwd(mode=1, H=2, W=2) == 0
    assert fwd(mode=1, H=1, W=8) == fwd(mode=1, H=8, W=1) == f"{n}: bad resample mode"
    assert fwd(mode=2, H=1, W=1) == 0
    for k in ("y", "xr", "ps0", "stats_out"):
        assert fwd(H=8, W=32, rows0=1, **{k: Y + 4}) == n + ALIGN
    assert fwd(C0=128, C1=128, x1=X1 + 2) == n + ALIGN
    assert fwd(force_route=2) == fwd(force_route=-1) == f"{n}: force_route is 0 (as routed) or 1 (per-channel kernels)"
    assert fwd(force_route=1) == 0
    assert fwd(B=3, H=32768, W=1, mode=2) == 0 and fwd(B=1, H=65536, W=32768) == f"{n}: grid too large"
    # piece sums
    ok = dict(H=16, W=64, ps0=PS0, rows0=4)
    assert fwd(**ok) == 0 and fwd(C0=128, **ok) == 0 and fwd(H=8, W=32, ps0=PS0, rows0=1) == 0
    assert fwd(dtype=F32, **ok) == f"{n}: piece sums are bf16 only"
    assert fwd(C0=128, C1=128, dtype=F32, ps1=PS1, rows1=4, H=16, W=64) == f"{n}: piece sums are bf16 only"
    assert fwd(ps1=PS1, rows1=4, H=16, W=64) == f"{n}: ps1 without a second source"
    for bad in (dict(rows0=3), dict(rows0=0), dict(rows0=8), dict(H=12, rows0=2), dict(H=20), dict(W=48, rows0=2), dict(W=96),
                dict(C0=192), dict(C0=320), dict(C0=64, C1=192)):
        assert fwd(**{**ok, **bad}) == PSUM, bad
    two = dict(C0=128, C1=256, H=16, W=64, ps0=PS0, rows0=4, ps1=PS1, rows1=4)
    assert fwd(**two) == 0
    assert fwd(**{**two, "rows1": 2}) == fwd(**{**two, "C1": 192}) == fwd(**{**two, "C0": 64, "C1": 320}) == PSUM
    assert fwd(**{**two, "ps0": None, "rows0": 0}) == 0 and fwd(**{**two, "ps1": None, "rows1": 77}) == 0       # one source without sums: legal


def test_refusals_gradient():
    n = "group_norm_vjp"
    for k in ("stats", "dy", "dx0"):
        assert vjp(**{k: None}) == f"{n}: NULL argument"
    assert vjp(C0=128, C1=128, x1=None) == vjp(C0=128, C1=128, dx1=None) == n + PIECES
    assert vjp(C0=128, C1=128, add1=ADD1) == vjp(C0=128, C1=128, add0=ADD0, dres=DRES) == 0
    assert vjp(mode=1, H=2, W=2) == 0
    assert vjp(mode=1, H=5, W=8) == vjp(mode=1, H=8, W=7) == vjp(mode=1, H=1, W=2) == f"{n}: bad resample mode"     # the forward floors
    for k in ("stats", "dy", "dres", "add0", "dx0"):
        assert vjp(**{k: DY + 4}) == n + ALIGN
    assert vjp(C0=128, C1=128, add1=ADD1 + 8) == vjp(C0=128, C1=128, dx1=DX1 + 8) == n + ALIGN
    assert vjp(H=65535, W=1) == 0 and vjp(H=65536, W=1) == f"{n}: grid too large"


def test_accepted_network_shapes():
    """every GroupNorm of the 256 px (256 channels x (1, 1, 2, 2, 4, 4)) and 512 px (x (0.5, 1, 1, 2, 2, 4, 4)) UNets, both types"""
    single = [(128, 512), (128, 256), (256, 256), (256, 128), (256, 64), (512, 64), (512, 32), (512, 16), (1024, 16), (1024, 8)]
    cat = [(1024, 1024, 8), (1024, 1024, 16), (1024, 512, 16), (512, 512, 32), (512, 512, 64), (512, 256, 64), (256, 256, 128),
           (256, 256, 256), (256, 128, 256), (128, 128, 512)]
    for dt in (BF16, F32):
        for f, g in ((fwd, plan), (vjp, vplan)):
            for Cc, px in single:
                for mode in (0, 1, 2) if px <= 256 else (0, 1):
                    assert f(B=2, H=px, W=px, C0=Cc, dtype=dt, mode=mode, ss=SS, ss_ld=21504) == 0
                    assert f(B=2, H=px, W=px, C0=Cc, dtype=dt, mode=mode, ss=SS, ss_ld=0) == 0
            for a, b, px in cat:
                assert f(B=4, H=px, W=px, C0=a, C1=b, dtype=dt) == 0
        for Cc, px in single:
            # the group kernels, but for the 512 px network's 128-channel layers in bf16 (4 channels a group: half a piece)
            assert plan(B=2, H=px, W=px, C0=Cc, dtype=dt)[0] == (1 if (Cc, dt) == (128, BF16) else 0)
    assert fwd(B=2, H=64, W=64, C0=256, ps0=PS0, rows0=16) == 0
    assert plan(B=2, H=64, W=64, C0=256, C1=512, ps0=PS0, rows0=16, ps1=PS1, rows1=16) == (0, 5, 32, 128, 1)


def test_forward_plan_edges():
    # per-channel route: 32 and 96 channels in both types (at 96 a 16-byte piece spans two groups), 128 in bf16
    assert plan(C0=32, H=5, W=9, dtype=F32)[0] == plan(C0=32, H=5, W=9)[0] == 1
    assert plan(C0=96, H=6, W=10, dtype=F32)[0] == plan(C0=96, H=6, W=10)[0] == 1
    assert plan(C0=128, dtype=F32)[0] == 0 and plan(C0=128)[0] == 1
    assert plan(C0=256)[0] == plan(C0=256, dtype=F32)[0] == 0
    # workgroup shapes: RY = max(1, 512 / PPP)
    assert plan(C0=768, H=6, W=10)[:2] == (0, 5)                    # 96 pieces x 5 rows = 480 threads
    assert plan(C0=768, H=6, W=10, dtype=F32)[:2] == (0, 2)         # 192 x 2 = 384
    assert plan(C0=2048, H=3, W=8)[:2] == (0, 2) and plan(C0=2048, H=3, W=8, dtype=F32)[:2] == (0, 1)
    assert plan(C0=4096, H=3, W=8)[:2] == (0, 1)
    assert plan(B=1, C0=4096, H=2, W=2, dtype=F32) == (0, 1, 4, 1, 0)       # PPP = 1024
    assert plan(B=1, C0=8192, H=2, W=2) == (0, 1, 4, 1, 0)
    # HW < RY (threads without a pixel), HW = 1
    assert plan(C0=256, H=1, W=1) == (0, 16, 1, 1, 0) and plan(C0=256, H=1, W=7) == (0, 16, 7, 1, 0)
    assert plan(C0=32, H=1, W=1, dtype=F32) == (1, 64, 1, 1, 0)
    # the chunk count saturates at 128 with a ragged last chunk: 91 x 91 = 8281 = 127 * 65 + 26
    assert plan(C0=256, H=91, W=91) == (0, 16, 65, 128, 0)
    # fewer chunks than HW / (4 RY): 90 pixels, RY = 2 -> 11 asked, ppc 9 -> 10 chunks
    assert plan(C0=2048, H=9, W=10) == (0, 2, 9, 10, 0) and 90 // (4 * 2) == 11
    # the row limit: B * Ho > 65535 runs the per-channel kernels on the same chunks
    assert plan(B=3, H=21845, W=1, C0=256)[0] == 0
    assert plan(B=3, H=21846, W=1, C0=256) == (1, 16, 171, 128, 0)
    assert plan(B=1, H=32768, W=1, C0=256, mode=0)[0] == 0 and plan(B=1, H=32768, W=1, C0=256, mode=2)[0] == 1
    assert plan(B=2, H=65535, W=2, C0=256, mode=1)[0] == 0 and plan(B=3, H=65535, W=2, C0=256, mode=1)[0] == 1
    # forced
    assert plan(C0=256, force_route=1) == (1,) + plan(C0=256)[1:]
    # the statistics source: piece sums only with the group kernels and sums of every source
    t = dict(H=16, W=64, ps0=PS0, rows0=4)
    assert plan(C0=256, **t)[4] == 1 and plan(C0=256, force_route=1, **t)[::4] == (1, 0)
    assert plan(C0=128, **t)[::4] == (1, 0)                                              # C = 128 bf16: per-channel, own pass
    assert plan(C0=128, C1=256, ps1=PS1, rows1=4, **t)[::4] == (1, 0)                    # 384 = 32 x 12: per-channel, own pass
    assert plan(C0=256, C1=512, ps1=PS1, rows1=4, **t)[::4] == (0, 1)
    assert plan(C0=256, C1=512, **t)[::4] == (0, 0)                                      # the second source has no sums: own pass
    assert plan(C0=256, C1=512, H=16, W=64, ps1=PS1, rows1=4)[::4] == (0, 0)
    assert plan(B=600, C0=256, H=128, W=32, ps0=PS0, rows0=16)[::4] == (1, 0)            # over the row limit


def test_gradient_plan_edges():
    # RY = max(1, 256 / PPP): half the forward's rows
    assert vplan(C0=768, H=6, W=10)[0] == 2 and vplan(C0=768, H=6, W=10, dtype=F32)[0] == 1
    assert vplan(C0=32, H=5, W=9)[0] == 64 and vplan(C0=256)[0] == 8 and plan(C0=256)[1] == 16
    assert vplan(C0=2048, H=3, W=8)[0] == 1
    assert vplan(B=1, C0=8192, H=2, W=2) == (1, 4, 1, 1) and vplan(B=1, C0=4096, H=2, W=2, dtype=F32) == (1, 4, 1, 1)
    assert vplan(C0=256, H=1, W=1) == (8, 1, 1, 1)
    assert vplan(C0=256, H=91, W=91) == (8, 65, 128, 1)
    # sample ranges of the last kernel: 65535 / H samples each
    assert vplan(B=3, H=21846, W=1, C0=256) == (8, 171, 128, 2) and vplan(B=3, H=21845, W=1, C0=256)[3] == 1
    assert vplan(B=5, H=40000, W=1, C0=256)[3] == 5


# ---------------------------------------------------------------------------------------------------------- the exact family's proofs
# every exact case of tests/test_gpu_groupnorm.py (the case's index is its seed); the apply pass of the largest ones is proven there, at
# run time, by the same assertions
EXACT = R.EXACT_CASES
exact_stats = R.exact_stats


@pytest.mark.parametrize("i", range(len(EXACT)))
def test_exact_family_is_predictable(i):
    B, H, W, C0, C1 = EXACT[i][:5]
    Cc = C0 + C1
    x = R.exact_input(B, H, W, Cc, seed=i)
    m32, r32, var = exact_stats(x)
    if x.size > 1 << 20:
        return
    assert (var == 0).any() and (r32[var == 0] == np.float32(1.0 / np.sqrt(np.float64(R.EPS)))).all(), "a group of variance exactly 0"
    if H * W * (Cc // 32) > 1:
        ratio = np.abs(m32) * r32
        assert ratio[var > 0].max() >= 40, "a group with a large mean and a tiny spread"
    rng = np.random.default_rng(i)
    for with_ss in (False, True):
        gamma, beta, ss = R.exact_params(B, Cc, i, with_ss)
        for mode in (0, 1, 2):
            if mode == 1 and min(H, W) < 2:
                continue
            y, ok = R.emulate_apply(x, m32, r32, gamma, beta, ss, False, mode)
            yc, okc = R.emulate_apply(x, m32, r32, gamma, beta, ss, False, mode, contracted=True)
            assert ok and okc, "an fma whose float64 argument is not exact"
            assert np.array_equal(y, yc), "the result depends on contracting beta - mean * ca"
            assert np.isfinite(y).all()
        # the emulation against exact rational arithmetic on sampled elements (mode 0)
        y, _ = R.emulate_apply(x, m32, r32, gamma, beta, ss, False, 0)
        cpg = Cc // 32
        for _ in range(40):
            b, h, w, c = (int(rng.integers(0, n)) for n in (B, H, W, Cc))
            want = R.apply_rational(x[b, h, w, c], m32[b, c // cpg], r32[b, c // cpg], gamma[c], beta[c],
                                    None if ss is None else ss[b, c], None if ss is None else ss[b, Cc + c])
            assert Fraction(float(y[b, h, w, c])) == want, (b, h, w, c)
    # the raw second output: float32 sums of four bf16 values are exact
    for mode in (1, 2):
        if mode == 1 and min(H, W) < 2:
            continue
        assert np.array_equal(R.resample_raw(x, mode).astype(np.float64), R.resample64(x, mode))


def test_round_f32_is_correct_rounding():
    rng = np.random.default_rng(0)
    for _ in range(300):
        a, b = float(np.float32(rng.normal())), float(np.float32(rng.normal() * 100))
        assert R.round_f32(Fraction(a) * Fraction(b)) == Fraction(float(np.float32(np.float64(a) * np.float64(b))))   # (48-bit product: exact in f64)
    assert R.round_f32(Fraction(2 ** 24 + 1)) == 2 ** 24 and R.round_f32(Fraction(2 ** 24 + 3)) == 2 ** 24 + 4       # ties to even
    assert R.round_f32(Fraction(1, 3)) == Fraction(float(np.float32(1 / 3)))


@pytest.mark.parametrize("H,W,C0,C1", [(8, 32, 256, 0), (16, 64, 256, 512), (16, 64, 128, 256), (8, 32, 128, 0)])
def test_exact_piece_sums(H, W, C0, C1):
    """float32 tile sums of the exact inputs are exact, so the piece-sum source must give the very statistics of the own pass"""
    x = R.exact_input(2, H, W, C0 + C1, seed=H + C0)
    parts = [x[..., :C0]] + ([x[..., C0:]] if C1 else [])
    ps = [R.psum_layout(p) for p in parts]
    for p, q in zip(ps, parts):
        assert p.shape == (2, (H // 8) * (W // 32), q.shape[3] // 8, 16)
        assert np.array_equal(p.astype(np.float64), R.psum_layout(q, np.float64).astype(np.float64)), "a float32 tile sum rounded"
    s, q, cnt = R.group_sums(x)
    s2, q2 = R.stats_from_psum(ps, cnt)
    assert np.array_equal(s, s2) and np.array_equal(q, q2)
    # the layout: tile (ty, tx) is row ty * (W / 32) + tx; the first 8 floats of a piece are the channel sums
    t = x[1, 8 * (H // 8 - 1):, 32 * (W // 32 - 1):, 8:16]
    assert np.array_equal(ps[0][1, -1, 1, :8], t.sum((0, 1))) and np.array_equal(ps[0][1, -1, 1, 8:], (t * t).sum((0, 1)))


@pytest.mark.parametrize("mode,H,W,Cc,with_ss", [(0, 5, 9, 256, True), (1, 6, 10, 96, False), (2, 3, 5, 768, True), (0, 1, 1, 32, False),
                                                 (1, 2, 2, 8192, True), (0, 2, 12, 2048, False)])
def test_exact_gradient_is_predictable(mode, H, W, Cc, with_ss):
    B, seed = 2, 10 * mode + H
    x = R.exact_grad_input(B, H, W, Cc, seed)
    m32, r32, var = exact_stats(x)
    assert (var == 0).all()
    # xh = fma(x, rstd, -(mean * rstd)) = 0: mean * rstd is exact (a power of two times rstd) and x == mean
    assert np.array_equal((m32 * r32).astype(np.float64), m32.astype(np.float64) * r32.astype(np.float64))
    Ho, Wo = R.out_size(H, W, mode)
    dy, _ = R.exact_grad_dy(B, Ho, Wo, Cc, seed)
    dres, _ = R.exact_grad_dy(B, Ho, Wo, Cc, seed + 1)
    add, _ = R.exact_grad_dy(B, H, W, Cc, seed + 2)
    gamma, beta, ss = R.exact_params(B, Cc, seed, with_ss, per_group=True)
    out, m1, exact = R.emulate_grad_const(dy, r32, gamma, ss, False, mode, H, W, dres, add)
    assert exact, "a group mean of dxh that is not exact"
    assert np.isfinite(out).all() and (m1 != 0).any()
    for t in (dy, dres, add):
        assert R.representable(t, "bf16")


@pytest.mark.parametrize("C0,C1,regime", [(256, 0, 0), (256, 512, 1), (256, 0, 1)])
def test_piece_sum_bound_holds_for_float32_tile_sums(C0, C1, regime):
    """Gaussian family, piece-sum source: the statistics taken from float32 tile sums (any summation order errs by at most 256 v of
    the sums of magnitudes) stay inside bound_mean / bound_rstd = the float32 error times (mean / std)^2"""
    x = gaussian_input(2, 16, 64, C0 + C1, regime, seed=5)
    ref = R.forward_reference(x, np.ones(C0 + C1, np.float32), np.zeros(C0 + C1, np.float32), None, False, 0, 0, "bf16", False, psum_err=256.0)
    parts = [x[..., :C0]] + ([x[..., C0:]] if C1 else [])
    for order in (np.float32, "seq"):
        if order == "seq":     # sequential float32 accumulation: the worst ordering the bound allows
            ps = []
            for p in parts:
                B, H, W, Cp = p.shape
                t = p.reshape(B, H // 8, 8, W // 32, 32, Cp // 8, 8).transpose(0, 1, 3, 5, 2, 4, 6).reshape(B, -1, Cp // 8, 256, 8).astype(np.float32)
                ps.append(np.concatenate((np.cumsum(t, 3, dtype=np.float32)[:, :, :, -1], np.cumsum(t * t, 3, dtype=np.float32)[:, :, :, -1]), -1))
        else:
            ps = [R.psum_layout(p) for p in parts]
        cnt = 16 * 64 * (C0 + C1) // 32
        s, q = R.stats_from_psum(ps, cnt)
        m32, r32, _, _ = R.stats_from_sums(s, q, cnt)
        assert (np.abs(m32 - ref["mean"]) <= ref["bmean"]).all()
        assert (np.abs(r32 - ref["rstd"]) <= ref["brstd"]).all()
    if regime == 1:
        assert (np.abs(ref["mean"]) * ref["rstd"]).max() > 30


gaussian_input = R.gaussian_input


def test_bounds_are_tight_enough_to_catch_an_ulp():
    """the element-wise bound must refuse what the old global tolerance let through: one group's mean off by a bf16 ulp, and one pixel
    column wrong by 1 %"""
    x = gaussian_input(1, 6, 10, 256, 1, seed=1)
    gamma, beta = np.ones(256, np.float32), np.zeros(256, np.float32)
    ref = R.forward_reference(x, gamma, beta, None, False, 0, 0, "bf16", True)
    g = int(np.argmax(np.abs(ref["mean"][0])))
    assert ref["bmean"][0, g] < np.abs(ref["mean"][0, g]) * 2.0 ** -12              # a bf16 ulp of the mean is 2^-8: far outside
    y = ref["y"].copy()
    y[:, :, 3, :] *= 1.01
    assert (np.abs(y - ref["y"]) > ref["by"]).any()
