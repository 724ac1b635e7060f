"""The latent schedule and noise kernels (csrc/latent.hip, csrc/noise.hip) one entry point at a time, straight through the C ABI,
against the float64 twin tests/latent_ref.py - the method of tests/test_gpu_audio_kernels.py: 4096 guard elements on both sides of
every buffer (tests/cabi_guard.py: NaN around inputs, a sentinel bit pattern in outputs; after each call the guards are intact, the
body is fully written and no NaN leaked in), an exact family compared bit for bit (indices as integers) and a random family inside a
derived bound, plus every argument check of the launchers as a refusal.  tests/test_latent_host.py proves what the exact families
rest on, holds the twin against torch, a dense spline solve and the oracle, and shows that these comparisons reject off-by-one
mutants of the twin.  test_zz_report prints the worst error / bound per family (WORST) and the measured deviations of the library
functions (DEVS).

Exact, bit for bit: blend (always: the kernel switches contraction off, every operation rounds once), scale_round_index, gather_rows, resample_linear (the
float32 chain; torch's CPU kernel is the same chain with its multiply-adds contracted, tests/test_latent_host.py), latent_merge in
its three modes and in place, the spline on data linear in t over power-of-two knot intervals (M = 0, every product exact),
noise_combine on operands whose products are float32 numbers, noise_mix on integer planes with dyadic modulators,
maua_noise_loop_batch against maua_noise_loop per layer, and the 65537-row case of every kernel whose row index rides in
gridDim.y / gridDim.z.

Bounds (v = 2^-24, u = 2^-53), each in tests/latent_ref.py next to the result it belongs to:
    weighted_sum      (2 A + 1) v sum |w| |lat|: A v on every weight (the sequential sum and the division), A v on every term
                      (its product and the additions after it).  Positive envelopes.
    spline_natural    v |value| (the rounding to float32) + the float64 part: 12 u of the terms' magnitudes and the Thomas sweep's
                      backward error 5 u (|A|, the right-hand side) through ||A^-1||_inf <= 1 / min (h_{i-1} + h_i)
    slerp             per element, first order: the five fixed-order sums (ceil(D / 256) + 9 roundings each), the divisions,
                      d_dot / sqrt(1 - dot^2) through acosf, acosf / cosf / sinf at their allowance (latent_ref.slerp lists the steps)
    noise_loop        per element: v |idx + n0|, cosf, times 50 / sigma and its two roundings, v |. + n1|, sinf, times n2; the sum of
                      squares carries its terms' errors and 1 + per-thread terms + 6 + 4 + blocks roundings, the root halves them;
                      raw maps at the first line, scales at the second (the raw pass's own block count)
    raw * scales      2 v of the normalised map: both forms reduce the same partial sums in the same order, so the factor is the same
                      float32 number and only the normalised map's own rounding (v) is left
    noise_mix         (M + 1) v sum |terms| (with two banks the second weight is the float32 1 - mod)
Library functions on the device (the project's convention): the float32 CPU function against float64 over the case's own arguments,
4 x the largest deviation allowed, no other margin.  noise.hip's own short sine and cosine are held to the same allowance; restated
on the CPU (tests/test_latent_host.py) they stay within 1.43 x the libm deviation for |x| <= 1e4, the range their header gives.
Measured deviations (absolute): acosf 1.3e-07, cosf 5.0e-08 and sinf 6.0e-08 over slerp's arguments; cosf 6.8e-08 and sinf 6.9e-08
over the Loop arguments (up to 1e3 at sigma 0.05); the report prints them.
Measured on an MI355X, worst error / bound: weighted_sum 0.55, spline_natural 1.00 (the bound is the rounding to float32 itself:
half a unit in the last place is reached), slerp 0.073 (endpoints 0.073), noise_loop 0.61 / 0.62 / 0.62 at sigma 5 / 0.5 / 0.05,
raw maps 0.65, raw scales 0.40, raw * scales 0.50 of 2 v (the same factor: v, the normalised map's rounding), noise_mix 0.94.

Where the reference itself returns NaN or inf - a row of envelopes summing to 0, parallel vectors in slerp - the twin follows it.
gather_rows takes indices in [-n_rows, n_rows) only (include/maua_hip.h): nothing outside is passed here."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import latent_ref as R  # noqa: E402
from cabi_guard import SENT, Buf, call, inp, ratio, refused, same  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
DEVS = {}
SENT_F32 = np.array([SENT[4]], np.uint32).view(np.float32)[0]        # the sentinel's bits as a (finite) float32


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), float(r))
    return r


def dev_note(name, value):
    DEVS[name] = max(DEVS.get(name, 0.0), float(value))
    return 4 * value


def hostp(a):
    return a.ctypes.data_as(C.c_void_p)


def refused_with(text, name, *args):
    """refused, and with the entry point's own message (never a bare launch error)"""
    rc = getattr(L.lib(), name)(L.ctx(), *args)
    assert rc != 0, f"{name} accepted {args}"
    with pytest.raises(L.MauaHipError, match=text):
        L.check(rc)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- blend
def run_blend(a, b, env, T, Cc):
    ab, bb, eb, out = inp(a), inp(b), inp(env), Buf(T * Cc)
    call("maua_latent_blend", ab.ptr, Cc if a.shape[0] > 1 or T == 1 else 0, bb.ptr, Cc if b.shape[0] > 1 or T == 1 else 0, eb.ptr, T, Cc, out.ptr)
    out.check("blend")
    for x in (ab, bb, eb):
        x.check("blend input")
    return out.get().reshape(T, Cc)


@pytest.mark.parametrize("Cc", R.TC_C)
def test_latent_blend(Cc):
    for T in R.TC_T:
        env = R.envelope(T, T + Cc)
        for ra, rb in ((T, T), (1, 1), (1, T)):
            a, b = R.normal((ra, Cc), 1 + T), R.normal((rb, Cc), 2 + T)
            got = run_blend(a, b, env, T, Cc)
            assert same(got, R.blend32(a, b, env)), (T, ra, rb)
            assert same(got[0], a[0]) and (T == 1 or same(got[-1], b[-1])), "env of 0 and 1 returns a and b"


def test_latent_blend_empty_and_refusals():
    a, e, out = inp(np.zeros(8)), inp(np.zeros(2)), Buf(8)
    call("maua_latent_blend", a.ptr, 4, a.ptr, 4, e.ptr, 0, 4, out.ptr)
    call("maua_latent_blend", a.ptr, 0, a.ptr, 0, e.ptr, 2, 0, out.ptr)
    assert out.untouched()
    refused("maua_latent_blend", None, 4, a.ptr, 4, e.ptr, 2, 4, out.ptr)
    refused("maua_latent_blend", a.ptr, 4, a.ptr, 4, None, 2, 4, out.ptr)
    refused("maua_latent_blend", a.ptr, 4, a.ptr, 4, e.ptr, 2, 4, None)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- weighted_sum
def run_weighted_sum(env, lat, nan_ok=False):
    T, A = env.shape
    n, Cc = lat.shape
    eb, lb, out = inp(env), inp(lat), Buf(T * Cc)
    call("maua_weighted_sum", eb.ptr, lb.ptr, T, A, n, Cc, out.ptr)
    out.check("weighted_sum", nan_ok=nan_ok)
    eb.check("env")
    lb.check("latents")
    return out.get().reshape(T, Cc)


@pytest.mark.parametrize("Cc", R.TC_C)
def test_weighted_sum(Cc):
    for T in R.TC_T:
        for A, n in ((5, 3), (1, 1), (2, 2), (257, 4)):       # A > n: the a % n wrap
            env = np.abs(R.normal((T, A), A + T)) + np.float32(0.05)
            lat = R.normal((n, Cc), n + Cc)
            want, bound = R.weighted_sum(env, lat)
            assert note("weighted_sum", ratio(run_weighted_sum(env, lat), want, bound)) <= 1, (T, A, n)
    env = R.f32([[0.0, 0.0], [1.0, -1.0], [1.0, 3.0]])         # rows summing to 0: NaN, or inf where the two latents differ in sign
    lat = np.ones((2, Cc), np.float32)
    lat[1, 1::2] = -1
    got = run_weighted_sum(env, lat, nan_ok=True)
    assert same(got[:2], R.weighted_sum32(env, lat)[:2]) and np.isnan(got[0]).all() and np.isfinite(got[2]).all()


def test_weighted_sum_limits_and_refusals():
    A = R.LDS_MAX
    env, lat = np.abs(R.normal((1, A), 0)) + np.float32(0.05), R.normal((3, 1), 1)
    want, bound = R.weighted_sum(env, lat)
    assert note("weighted_sum", ratio(run_weighted_sum(env, lat), want, bound)) <= 1, "the largest A the entry point accepts"
    e, l, out = inp(np.ones(A + 1)), inp(np.ones(4)), Buf(4)
    refused_with("maua_weighted_sum", "maua_weighted_sum", e.ptr, l.ptr, 1, A + 1, 1, 1, out.ptr)
    refused("maua_weighted_sum", e.ptr, l.ptr, 1, 0, 1, 1, out.ptr)
    refused("maua_weighted_sum", e.ptr, l.ptr, 1, 2, 0, 1, out.ptr)
    refused("maua_weighted_sum", None, l.ptr, 1, 2, 1, 1, out.ptr)
    call("maua_weighted_sum", e.ptr, l.ptr, 0, 2, 1, 1, out.ptr)
    call("maua_weighted_sum", e.ptr, l.ptr, 1, 2, 1, 0, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- indices
def test_scale_round_index():
    ties = R.round_input()
    for n in (ties.size, 1, 255, 256, 257, 1000):
        x = ties if n == ties.size else R.f32(np.round(R.normal(n, n) * 8) / 2)          # halves: every other one a tie
        xb = inp(x)
        for scale in (1.0, 0.5, -1.0, 0.0, 3.0):
            out = Buf(n, torch.int64)
            call("maua_scale_round_index", xb.ptr, scale, n, out.ptr)
            out.check("scale_round_index")
            assert np.array_equal(out.get(), R.scale_round_index(x, scale)), (n, scale)
        xb.check("x")
    out = Buf(4, torch.int64)
    call("maua_scale_round_index", xb.ptr, 1.0, 0, out.ptr)
    refused("maua_scale_round_index", None, 1.0, 4, out.ptr)
    refused("maua_scale_round_index", xb.ptr, 1.0, 4, None)
    assert out.untouched()


def run_gather(src, idx):
    n_rows, Cc = src.shape
    T = idx.size
    sb, ib, out = inp(src), inp(idx, torch.int64, guard=0), Buf(T * Cc)
    call("maua_gather_rows", sb.ptr, ib.ptr, n_rows, T, Cc, out.ptr)
    out.check("gather_rows")
    sb.check("src")
    return out.get().reshape(T, Cc)


@pytest.mark.parametrize("Cc", R.TC_C)
def test_gather_rows(Cc):
    for T in R.TC_T + (9,):
        for n_rows in (1, 5):
            src = R.normal((n_rows, Cc), n_rows + Cc)
            idx = R.gather_input(n_rows, T, T)               # -1 and -n_rows: the negative branch; nothing outside [-n_rows, n_rows)
            assert same(run_gather(src, idx), R.gather_rows(src, idx)), (T, n_rows)
    out, s, i = Buf(4), inp(np.zeros(4)), inp(np.zeros(2), torch.int64, guard=0)
    call("maua_gather_rows", s.ptr, i.ptr, 2, 0, 2, out.ptr)
    call("maua_gather_rows", s.ptr, i.ptr, 2, 2, 0, out.ptr)
    refused("maua_gather_rows", s.ptr, None, 2, 2, 2, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- resample
def run_resample(x, size):
    n, Cc = x.shape
    xb, out = inp(x), Buf(size * Cc)
    call("maua_resample_linear", xb.ptr, n, Cc, size, out.ptr)
    out.check("resample_linear")
    xb.check("x")
    return out.get().reshape(size, Cc)


@pytest.mark.parametrize("Cc", R.TC_C)
def test_resample_linear(Cc):
    for n, size in R.RESAMPLE:                               # n = 1, size = 1, up, down, size = n, 3 -> 9 and 7 -> 21 (src next to an integer)
        x = R.normal((n, Cc), n * 100 + size)
        assert same(run_resample(x, size), R.resample_linear32(x, size)), (n, size)
    x, out = inp(np.zeros(4)), Buf(4)
    call("maua_resample_linear", x.ptr, 2, 2, 0, out.ptr)
    call("maua_resample_linear", x.ptr, 2, 0, 2, out.ptr)
    refused("maua_resample_linear", x.ptr, 0, 2, 2, out.ptr)
    refused("maua_resample_linear", None, 2, 2, 2, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- spline
def run_spline(tk, y, te):
    n, Cc = y.shape
    T = te.size
    tk, te = np.ascontiguousarray(tk, dtype=np.float64), np.ascontiguousarray(te, dtype=np.float64)
    yb, out = inp(y), Buf(T * Cc)
    call("maua_spline_natural", hostp(tk), n, yb.ptr, Cc, hostp(te), T, out.ptr)
    out.check("spline_natural")
    yb.check("knot values")
    return out.get().reshape(T, Cc)


@pytest.mark.parametrize("Cc", R.TC_C)
def test_spline_natural(Cc):
    for n in (2, 3, 7):
        tk = R.spline_knots(n)                               # unequal spacing
        for T in R.TC_T + (20,):
            te = R.spline_eval_points(tk, T) if T > 2 else np.array([tk[-1] + 0.375, tk[0] - 0.25][:T])     # knots, before the first, after the last
            y, alpha, beta = R.spline_linear_data(tk, Cc, n + T)
            assert same(run_spline(tk, y, te), R.f32(te[:, None] * alpha + beta)), ("linear data", n, T)
            y = R.normal((n, Cc), n * T)
            want, bound = R.spline_natural(tk, y, te)
            assert note("spline_natural", ratio(run_spline(tk, y, te), want, bound)) <= 1, (n, T)
    tk = np.linspace(0.0, 1.0, 5)                            # spline_loop_latents: the % 1 wrap puts te = 0 last
    te = R.loop_eval_points(9, 2)
    assert te[-1] == 0
    y = R.normal((4, Cc), 5)
    Y = np.concatenate((y, y[:1]))
    want, bound = R.spline_natural(tk, Y, te)
    got = run_spline(tk, Y, te)
    assert note("spline_natural", ratio(got, want, bound)) <= 1 and same(got[-1], y[0]) and same(got[0], y[0])


def test_spline_natural_empty_and_refusals():
    tk, te = np.array([0.0, 1.0, 2.0]), np.array([0.5, 1.5])
    y, out = inp(np.zeros(6)), Buf(4)
    call("maua_spline_natural", hostp(tk), 3, y.ptr, 2, hostp(te), 0, out.ptr)
    call("maua_spline_natural", hostp(tk), 3, y.ptr, 0, hostp(te), 2, out.ptr)
    refused("maua_spline_natural", hostp(tk), 1, y.ptr, 2, hostp(te), 2, out.ptr)
    for bad in (np.array([0.0, 1.0, 1.0]), np.array([0.0, 2.0, 1.0]), np.array([0.0, np.nan, 1.0])):
        refused_with("strictly increasing", "maua_spline_natural", hostp(bad), 3, y.ptr, 2, hostp(te), 2, out.ptr)
    refused("maua_spline_natural", hostp(tk), 3, None, 2, hostp(te), 2, out.ptr)
    refused("maua_spline_natural", None, 3, y.ptr, 2, hostp(te), 2, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- slerp
def run_slerp(y, t, nan_ok=False):
    n_seg, Ln, D = y.shape[0] - 1, y.shape[1], y.shape[2]
    yb, tb, out = inp(y), inp(t), Buf(t.size * n_seg * Ln * D)
    call("maua_slerp", yb.ptr, tb.ptr, t.size, n_seg, Ln, D, out.ptr)
    out.check("slerp", nan_ok=nan_ok)
    yb.check("y")
    tb.check("t")
    return out.get().reshape(t.size, n_seg, Ln, D)


def slerp_reference(y, t):
    _, _, dot, p = R.slerp(y, t)
    ad = dev_note("acosf, absolute (slerp)", R.measured_dev(np.arccos, np.arccos, [dot]))
    cd = dev_note("cosf, absolute (slerp)", R.measured_dev(np.cos, np.cos, [p]))
    sd = dev_note("sinf, absolute (slerp)", R.measured_dev(np.sin, np.sin, [p]))
    return R.slerp(y, t, ad, cd, sd)[:2]


@pytest.mark.parametrize("D", R.SLERP_D)
def test_slerp(D):
    y = R.slerp_input(2, 3, D, D)
    t = R.f32([0.0, 1.0, 0.25, 0.7, 0.5])
    want, bound = slerp_reference(y, t)
    got = run_slerp(y, t)
    assert note("slerp", ratio(got, want, bound)) <= 1
    y64 = y.astype(np.float64)
    for k, end in ((0, y64[:-1]), (1, y64[1:])):             # t of 0 and 1: the normalised endpoints
        assert note("slerp, endpoints", ratio(got[k], end / np.linalg.norm(end, axis=-1, keepdims=True), bound[k])) <= 1
    par = np.zeros((2, 1, D), np.float32)                    # parallel vectors: c = 0 / 0, NaN throughout, like the reference
    par[:, 0, 0] = (2.0, 3.0)
    got = run_slerp(par, t[:2], nan_ok=True)
    assert np.isnan(got).all() and np.isnan(R.slerp(par, t[:2])[0]).all()


def test_slerp_empty_and_refusals():
    y, t, out = inp(np.ones(8)), inp(np.zeros(2)), Buf(8)
    call("maua_slerp", y.ptr, t.ptr, 0, 1, 2, 2, out.ptr)
    call("maua_slerp", y.ptr, t.ptr, 2, 0, 2, 2, out.ptr)
    refused("maua_slerp", y.ptr, t.ptr, 2, 1, 0, 2, out.ptr)
    refused("maua_slerp", y.ptr, t.ptr, 2, 1, 2, 0, out.ptr)
    refused("maua_slerp", None, t.ptr, 2, 1, 2, 2, out.ptr)
    refused("maua_slerp", y.ptr, None, 2, 1, 2, 2, out.ptr)
    refused_with("65535 segments", "maua_slerp", y.ptr, t.ptr, 1, 65536, 1, 1, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- latent_merge
def merge_case(T, Ln, D, l0, l1, seed):
    """lat with the sentinel's bits in every layer outside [l0, l1); seq with NaN there (never read)"""
    lat, seq = R.normal((T, Ln, D), seed), R.normal((T, Ln, D), seed + 1)
    keep = np.ones(Ln, bool)
    keep[l0:l1] = False
    lat[:, keep] = SENT_F32
    seq[:, keep] = np.nan
    return lat, seq, R.envelope(T, seed + 2)


def run_merge(lat, seq, mod, mode, l0, l1):
    T, Ln, D = lat.shape
    lb, sb = inp(lat), inp(seq)
    mb = inp(mod) if mod is not None else None
    call("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr if mb else None, mode, T, Ln, D, l0, l1)
    lb.check("latents in place")
    sb.check("sequence")
    return lb.get().reshape(T, Ln, D)


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_latent_merge(mode):
    for D in R.TC_C:                                         # the span of one layer: the edges of the 256-thread block
        for T in R.TC_T:
            for Ln, l0, l1 in ((3, 1, 2), (3, 0, 3), (4, 2, 4), (4, 0, 1)):
                lat, seq, mod = merge_case(T, Ln, D, l0, l1, D + T + l0)
                got = run_merge(lat, seq, mod if mode == 1 else None, mode, l0, l1)
                want = R.latent_merge32(lat, seq, mod, mode, l0, l1)
                assert same(got.view(np.uint32), want.view(np.uint32)), (D, T, Ln, l0, l1)
                assert not np.isnan(got).any()
                keep = np.ones(Ln, bool)
                keep[l0:l1] = False
                assert (got[:, keep].view(np.uint32) == SENT[4]).all(), "layers outside [l0, l1) keep their bits"
    lat, seq, mod = merge_case(2, 3, 5, 1, 2, 0)
    for l0, l1 in ((2, 2), (2, 1)):                          # an empty slice: success, nothing written
        assert same(run_merge(lat, seq, mod, mode, l0, l1).view(np.uint32), lat.view(np.uint32))


def test_latent_merge_refusals():
    lat = R.normal((2, 3, 5), 0)
    lb, sb, mb = inp(lat), inp(lat), inp(np.zeros(2))
    refused("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr, 3, 2, 3, 5, 0, 3)
    refused("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr, -1, 2, 3, 5, 0, 3)
    refused("maua_latent_merge", lb.ptr, sb.ptr, None, 1, 2, 3, 5, 0, 3)
    refused("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr, 0, 2, 3, 5, 0, 4)
    refused("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr, 0, 2, 3, 5, -1, 2)
    refused("maua_latent_merge", None, sb.ptr, mb.ptr, 0, 2, 3, 5, 0, 3)
    refused("maua_latent_merge", lb.ptr, None, mb.ptr, 0, 2, 3, 5, 0, 3)
    call("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr, 0, 0, 3, 5, 0, 3)
    call("maua_latent_merge", lb.ptr, sb.ptr, mb.ptr, 0, 2, 3, 0, 0, 3)      # D = 0: success, nothing to launch
    lb.check("latents")
    assert same(lb.get(), lat.reshape(-1))


# ---------------------------------------------------------------------------------------------------------------- 65537 rows
@pytest.mark.parametrize("kernel", ("blend", "weighted_sum", "gather_rows", "resample_linear", "spline", "merge", "slerp"))
def test_beyond_one_grid(kernel):
    """65537 rows of one column: the row index no longer fits one launch's gridDim.y (slerp: gridDim.z); bit for bit"""
    T = R.BIG_T
    if kernel == "blend":
        env = R.envelope(T, 1)
        a, b = R.normal((T, 1), 2), R.normal((T, 1), 3)
        assert same(run_blend(a, b, env, T, 1), R.blend32(a, b, env)), "strides C"
        assert same(run_blend(a[:1], b[:1], env, T, 1), R.blend32(a[:1], b[:1], env)), "strides 0"
    elif kernel == "weighted_sum":                           # dyadic weights over a power-of-two sum, integer latents: exact
        env = R.f32(np.random.default_rng(4).choice([1.0, 3.0], size=(T, 2)))
        env[:, 1] = np.where(env[:, 0] == 1, R.f32(np.random.default_rng(5).choice([1.0, 3.0, 7.0], size=T)), R.f32(np.random.default_rng(6).choice([1.0, 5.0], size=T)))
        lat = R.f32([[3.0], [-5.0]])
        want = R.weighted_sum(env, lat)[0]
        assert R.is_f32(env / env.sum(1, keepdims=True)) and R.is_f32(want) and len(np.unique(want)) > 3
        assert same(run_weighted_sum(env, lat), R.f32(want))
    elif kernel == "gather_rows":
        src, idx = R.normal((3, 1), 7), R.gather_input(3, T, 8)
        assert same(run_gather(src, idx), R.gather_rows(src, idx))
    elif kernel == "resample_linear":
        x = R.normal((3, 1), 9)
        assert same(run_resample(x, T), R.resample_linear32(x, T))
    elif kernel == "spline":
        tk = R.spline_knots(3)
        te = np.random.default_rng(10).integers(-64, 200, size=T) / 256.0
        y, alpha, beta = R.spline_linear_data(tk, 1, 11)
        want = te[:, None] * alpha + beta
        assert alpha[0] != 0 and R.is_f32(want) and same(R.spline_natural(tk, y, te)[0], want)
        assert same(run_spline(tk, y, te), R.f32(want))
    elif kernel == "merge":
        lat, seq, mod = R.normal((T, 1, 1), 12), R.normal((T, 1, 1), 13), R.envelope(T, 14)
        for mode in (0, 1, 2):
            got = run_merge(lat, seq, mod if mode == 1 else None, mode, 0, 1)
            assert same(got, R.latent_merge32(lat, seq, mod, mode, 0, 1)), mode
    else:                                                    # every t its own block: the same bits as the first 300 rows run alone
        y = R.slerp_input(1, 1, 2, 15)
        t = R.f32(np.random.default_rng(16).uniform(0, 1, T))
        got = run_slerp(y, t)
        want, bound = slerp_reference(y, t)
        assert note("slerp", ratio(got, want, bound)) <= 1
        assert same(got[:300], run_slerp(y, t[:300])) and same(got[-300:], run_slerp(y, t[-300:]))


# ---------------------------------------------------------------------------------------------------------------- noise: Loop
I0 = 2                                                      # frames start at idx[2]; idx[0], idx[1] and the guards behind the last are NaN


def loop_case(hw, B, sigma, seed):
    planes = R.normal((3, hw), seed)
    idx = R.loop_idx(I0 + B)
    idx_dev = idx.copy()
    idx_dev[:I0] = np.nan
    return planes, idx, idx_dev


def loop_reference(planes, idx, B, sigma, nblk):
    _, _, x0, x1 = R.loop_values(planes, idx[I0:I0 + B], sigma)
    cd = dev_note("cosf, absolute (noise_loop)", R.measured_dev(np.cos, np.cos, [x0]))
    sd = dev_note("sinf, absolute (noise_loop)", R.measured_dev(np.sin, np.sin, [x1]))
    val, dval, _, _ = R.loop_values(planes, idx[I0:I0 + B], sigma, cd, sd)
    return (val, dval) + R.loop_normalised(val, dval, nblk)


def run_loop(planes, idx_dev, B, hw, sigma):
    pb, ib, out = inp(planes), inp(idx_dev), Buf(B * hw)
    call("maua_noise_loop", pb.ptr, ib.ptr, I0, B, hw, 1, sigma, out.ptr)
    out.check("noise_loop")
    pb.check("planes")
    ib.check("idx")
    return out.get().reshape(B, hw)


@pytest.mark.parametrize("hw", R.NOISE_HW)
def test_noise_loop(hw):
    for B in (1, 3):
        for sigma in R.NOISE_SIGMA:
            planes, idx, idx_dev = loop_case(hw, B, sigma, hw + B)
            _, _, want, bound, _, _ = loop_reference(planes, idx, B, sigma, R.noise_path(hw)[3])
            got = run_loop(planes, idx_dev, B, hw, sigma)
            assert note(f"noise_loop, sigma {sigma:g}", ratio(got, want, bound)) <= 1, (B, sigma)


@pytest.mark.parametrize("n", (1, 5, 24))
def test_noise_loop_batch(n):
    """large, small, large: both paths, both sides of both caps.  The batch equals the single call bit for bit per layer; the raw
    maps times their scales equal the normalised maps within 2 v; the raw maps and the scales against the twin"""
    B = 3
    hws = [R.BATCH_HW[l % len(R.BATCH_HW)] for l in range(n)]
    sig = [R.NOISE_SIGMA[l % 3] for l in range(n)]
    cases = [loop_case(hw, B, s, 100 + l) for l, (hw, s) in enumerate(zip(hws, sig))]
    single = [run_loop(c[0], c[2], B, hw, s) for c, hw, s in zip(cases, hws, sig)]
    pbs, ibs = [inp(c[0]) for c in cases], [inp(c[2]) for c in cases]
    P, Ix = (C.c_void_p * n)(*[b.ptr.value for b in pbs]), (C.c_void_p * n)(*[b.ptr.value for b in ibs])
    H, W, S = (C.c_int * n)(*hws), (C.c_int * n)(*([1] * n)), (C.c_float * n)(*sig)
    outs = [Buf(B * hw) for hw in hws]
    call("maua_noise_loop_batch", n, P, Ix, H, W, S, I0, B, (C.c_void_p * n)(*[b.ptr.value for b in outs]))
    raws, scales = [Buf(B * hw) for hw in hws], Buf(n * B)
    call("maua_noise_loop_batch_raw", n, P, Ix, H, W, S, I0, B, (C.c_void_p * n)(*[b.ptr.value for b in raws]), scales.ptr)
    scales.check("scales")
    sc = scales.get().reshape(n, B).astype(np.float64)
    for l, (hw, s) in enumerate(zip(hws, sig)):
        outs[l].check("noise_loop_batch")
        raws[l].check("noise_loop_batch_raw")
        assert same(outs[l].get().reshape(B, hw), single[l]), (l, hw)
        raw = raws[l].get().reshape(B, hw).astype(np.float64)
        val, dval, _, _, want_scale, rel = loop_reference(cases[l][0], cases[l][1], B, s, R.noise_path(hw)[3])
        assert note("noise_loop_batch_raw, maps", ratio(raw, val, dval)) <= 1, (l, hw)
        assert note("noise_loop_batch_raw, scales", ratio(sc[l], want_scale, rel * want_scale)) <= 1, (l, hw)
        norm = single[l].astype(np.float64)
        capped = R.noise_path(hw)[2] > R.noise_path(hw)[3]
        assert note("raw * scales, " + ("256 blocks, grid-stride" if capped else "one sweep per block"), ratio(raw * sc[l][:, None], norm, 2 * R.V * np.abs(norm))) <= 1, (l, hw)
    for b in pbs + ibs:
        b.check("an input")


def test_noise_loop_refusals():
    p, i, out, sc = inp(np.zeros(12)), inp(np.zeros(4)), Buf(8), Buf(8)
    call("maua_noise_loop", p.ptr, i.ptr, 0, 0, 2, 2, 5.0, out.ptr)
    call("maua_noise_loop", p.ptr, i.ptr, 0, 2, 0, 2, 5.0, out.ptr)
    refused_with("sigma", "maua_noise_loop", p.ptr, i.ptr, 0, 2, 2, 2, 0.0, out.ptr)
    refused_with("65535", "maua_noise_loop", p.ptr, i.ptr, 0, 65536, 2, 2, 5.0, out.ptr)
    refused("maua_noise_loop", None, i.ptr, 0, 2, 2, 2, 5.0, out.ptr)
    refused("maua_noise_loop", p.ptr, None, 0, 2, 2, 2, 5.0, out.ptr)

    def arrays(n, sigma=5.0, planes=p):
        return (n, (C.c_void_p * n)(*[planes.ptr.value if planes else None] * n), (C.c_void_p * n)(*[i.ptr.value] * n), (C.c_int * n)(*[2] * n), (C.c_int * n)(*[2] * n),
                (C.c_float * n)(*[sigma] * n))
    O25 = (C.c_void_p * 25)(*[out.ptr.value] * 25)
    for name, tail in (("maua_noise_loop_batch", ()), ("maua_noise_loop_batch_raw", (sc.ptr,))):
        refused_with("24 layers", name, *arrays(25), 0, 1, O25, *tail)
        refused(name, *arrays(2, sigma=0.0), 0, 1, O25, *tail)
        refused(name, *arrays(2, planes=None), 0, 1, O25, *tail)
        refused_with("65535", name, *arrays(2), 0, 65536, O25, *tail)
        call(name, *arrays(2), 0, 0, O25, *tail)
        call(name, 0, *arrays(2)[1:], 0, 1, O25, *tail)
    refused("maua_noise_loop_batch_raw", *arrays(2), 0, 1, O25, None)
    assert out.untouched() and sc.untouched()


# ---------------------------------------------------------------------------------------------------------------- noise: mix, combine
def run_mix(n1, n2, mod, hw):
    B, M = mod.shape
    b1, b2, mb, out = inp(n1), (inp(n2) if n2 is not None else None), inp(mod), Buf(B * hw)
    call("maua_noise_mix", b1.ptr, b2.ptr if b2 else None, mb.ptr, M, B, hw, 1, out.ptr)
    out.check("noise_mix")
    for b in (b1, b2, mb):
        if b:
            b.check("noise_mix input")
    return out.get().reshape(B, hw)


@pytest.mark.parametrize("M", R.MIX_M)
def test_noise_mix(M):
    for hw in (1, 255, 257) + ((65537,) if M < 257 else ()):  # 65537: the grid-stride loop's second round
        for B in (1, 3):
            n1, n2, mod = R.mix_exact_input(M, hw, B, M + hw)
            for banks in (1, 2):
                got = run_mix(n1, n2 if banks == 2 else None, mod, hw)
                assert same(got, R.f32(R.noise_mix(n1, n2 if banks == 2 else None, mod)[0])), ("exact", hw, B, banks)
            n1, n2 = R.normal((M, hw), hw), R.normal((M, hw), hw + 1)
            mod = R.f32(np.random.default_rng(B).uniform(0, 1, (B, M)))
            for banks in (1, 2):
                want, bound = R.noise_mix(n1, n2 if banks == 2 else None, mod)
                assert note("noise_mix", ratio(run_mix(n1, n2 if banks == 2 else None, mod, hw), want, bound)) <= 1, (hw, B, banks)


def test_noise_mix_limits_and_refusals():
    M = R.LDS_MAX
    n1, mod = R.normal((M, 1), 0), R.f32(np.random.default_rng(1).uniform(0, 1, (1, M)))
    want, bound = R.noise_mix(n1, None, mod)
    assert note("noise_mix", ratio(run_mix(n1, None, mod, 1), want, bound)) <= 1, "the largest M the entry point accepts"
    nb, mb, out = inp(np.zeros(M + 1)), inp(np.zeros(M + 1)), Buf(4)
    refused_with("maua_noise_mix", "maua_noise_mix", nb.ptr, None, mb.ptr, M + 1, 1, 1, 1, out.ptr)
    refused_with("65535", "maua_noise_mix", nb.ptr, None, mb.ptr, 1, 65536, 1, 1, out.ptr)
    refused("maua_noise_mix", nb.ptr, None, mb.ptr, 0, 1, 1, 1, out.ptr)
    refused("maua_noise_mix", None, None, mb.ptr, 1, 1, 1, 1, out.ptr)
    refused("maua_noise_mix", nb.ptr, None, None, 1, 1, 1, 1, out.ptr)
    call("maua_noise_mix", nb.ptr, None, mb.ptr, 1, 0, 1, 1, out.ptr)
    call("maua_noise_mix", nb.ptr, None, mb.ptr, 1, 1, 0, 1, out.ptr)
    assert out.untouched()


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_noise_combine(mode):
    for hw in (1, 255, 257, 256 * 256 - 3, 256 * 256 + 5):   # below and above one round of the grid-stride loop
        for B in (1, 3):
            x, y, mod, scale, bias = R.combine_exact_input(B, hw, hw + B)
            xb, yb, mb, out = inp(x), inp(y), inp(mod), Buf(B * hw)
            call("maua_noise_combine", xb.ptr, yb.ptr if mode < 2 else None, mb.ptr if mode == 1 else None, mode, scale, bias, B, hw, 1, out.ptr)
            out.check("noise_combine")
            assert same(out.get().reshape(B, hw), R.noise_combine32(x, y, mod, mode, scale, bias)), (hw, B)
            for b in (xb, yb, mb):
                b.check("noise_combine input")


def test_noise_combine_refusals():
    x, m, out = inp(np.zeros(8)), inp(np.zeros(2)), Buf(8)
    refused("maua_noise_combine", x.ptr, None, None, 0, 1.0, 0.0, 2, 2, 2, out.ptr)
    refused("maua_noise_combine", x.ptr, None, m.ptr, 1, 1.0, 0.0, 2, 2, 2, out.ptr)
    refused("maua_noise_combine", x.ptr, x.ptr, None, 1, 1.0, 0.0, 2, 2, 2, out.ptr)
    refused("maua_noise_combine", x.ptr, x.ptr, m.ptr, 3, 1.0, 0.0, 2, 2, 2, out.ptr)
    refused("maua_noise_combine", x.ptr, x.ptr, m.ptr, -1, 1.0, 0.0, 2, 2, 2, out.ptr)
    refused("maua_noise_combine", None, x.ptr, m.ptr, 0, 1.0, 0.0, 2, 2, 2, out.ptr)
    refused("maua_noise_combine", x.ptr, x.ptr, m.ptr, 0, 1.0, 0.0, 2, 2, 2, None)
    refused_with("65535", "maua_noise_combine", x.ptr, x.ptr, m.ptr, 0, 1.0, 0.0, 65536, 2, 2, out.ptr)
    call("maua_noise_combine", x.ptr, x.ptr, m.ptr, 0, 1.0, 0.0, 0, 2, 2, out.ptr)
    call("maua_noise_combine", x.ptr, x.ptr, m.ptr, 0, 1.0, 0.0, 2, 0, 2, out.ptr)
    assert out.untouched()


def test_negative_sizes_are_refused():
    """a negative count is an error, never a launch that silently does nothing"""
    x, e, i64, out, o64 = inp(np.ones(16)), inp(np.ones(4)), inp(np.zeros(4), torch.int64, guard=0), Buf(16), Buf(4, torch.int64)
    tk = np.array([0.0, 1.0, 2.0])
    for T, Cc in ((-1, 2), (2, -1)):
        refused("maua_latent_blend", x.ptr, 2, x.ptr, 2, e.ptr, T, Cc, out.ptr)
        refused("maua_weighted_sum", e.ptr, x.ptr, T, 2, 2, Cc, out.ptr)
        refused("maua_gather_rows", x.ptr, i64.ptr, 2, T, Cc, out.ptr)
        refused("maua_resample_linear", x.ptr, 2, Cc, T, out.ptr)
        refused("maua_spline_natural", hostp(tk), 3, x.ptr, Cc, hostp(tk), T, out.ptr)
        refused("maua_latent_merge", x.ptr, x.ptr, e.ptr, 0, T, 2, Cc, 0, 2)
        refused("maua_slerp", x.ptr, e.ptr, T, Cc, 1, 2, out.ptr)
    refused("maua_scale_round_index", x.ptr, 1.0, -1, o64.ptr)
    for B, h, w in ((-1, 2, 2), (1, -2, 2), (1, 2, -2)):
        refused("maua_noise_loop", x.ptr, e.ptr, 0, B, h, w, 5.0, out.ptr)
        refused("maua_noise_mix", x.ptr, None, e.ptr, 1, B, h, w, out.ptr)
        refused("maua_noise_combine", x.ptr, x.ptr, e.ptr, 0, 1.0, 0.0, B, h, w, out.ptr)
        P, Ix, O = (C.c_void_p * 1)(x.ptr.value), (C.c_void_p * 1)(e.ptr.value), (C.c_void_p * 1)(out.ptr.value)
        for name, tail in (("maua_noise_loop_batch", ()), ("maua_noise_loop_batch_raw", (e.ptr,))):
            refused(name, 1, P, Ix, (C.c_int * 1)(h), (C.c_int * 1)(w), (C.c_float * 1)(5.0), 0, B, O, *tail)
            refused(name, -1, P, Ix, (C.c_int * 1)(2), (C.c_int * 1)(2), (C.c_float * 1)(5.0), 0, 1, O, *tail)
    assert out.untouched() and o64.untouched()
    x.check("x")


# ---------------------------------------------------------------------------------------------------------------- report
def test_zz_report():
    """the worst error / bound per family and the measured deviations of the library functions"""
    for k in sorted(WORST):
        print(f"[latent kernels] worst error / bound, {k}: {WORST[k]:.4f}")
    for k in sorted(DEVS):
        print(f"[latent kernels] float32 against float64 over the cases' arguments, {k}: {DEVS[k]:.3e} (4 x allowed)")
    assert all(v <= 1 for v in WORST.values())
