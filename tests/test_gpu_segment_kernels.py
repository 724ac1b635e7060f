"""The beat tracker and segmentation kernels (csrc/segment.hip) one entry point at a time, straight through the C ABI, against the
twin tests/segment_ref.py - the method of tests/test_gpu_audio_kernels.py: 4096 guard elements on both sides of every buffer
(tests/cabi_guard.py: NaN around float inputs, a sentinel bit pattern in outputs; after each call the guards are intact, the body is
fully written and no NaN leaked in), an exact family compared bit for bit (indices as integers) and a random family inside a derived
bound, plus every argument check of the launchers as a refusal.  tests/test_segment_host.py holds the twin against scipy, torch, the
oracle and the filter written literally, proves the preconditions and shows that these comparisons reject off-by-one mutants.
test_zz_report prints the worst error / bound per family (WORST) and the measured deviations of the library functions (DEVS).

Exact, bit for bit: segment_reduce (the lower median by rank; the mean as the sequential float32 sum and one division; NaN for an
empty segment), the kept set of recurrence_affinity on integer features (every distance the correctly rounded root of an exact
integer; ties: lower row first; the bandwidth one of those distances), timelag_median, median_filter_rows (and its 65537-row case),
the links of beat_dp on every frame whose best candidate leads by more than the margin, every link and cumulative score of beat_dp
where whole windows tie exactly (the first maximum wins), soft_kmeans with k = 1 or iters = 0.

Bounds (v = 2^-24, u = 2^-53), each in tests/segment_ref.py next to the result it belongs to:
    beat localscore   (2 period + 6) u sum |env| |window|: exp on the host and in numpy within one ulp of the truth, a product and
                      2 period + 1 additions in float64 (contracted or not)
    beat cumscore     against the twin's program fed the device's own localscore: per frame the largest candidate error (the
                      predecessor's bound + 12 u |txwt| for the two logs + u of the sum) + u |cumscore|; links compared where the
                      best candidate leads the second by more than twice that (at most 1 % of a case's frames may fall below)
    recurrence values rec (2 v |arg| + expf + v) + the smallest normal number: the quotient's rounding through the exponential
    soft_kmeans       4 x the deviation of the twin's float32 restatement (the kernel's own reduction order) from its float64 form
                      on the same inputs, for r and for mu; rows of r sum to 1 within (k + 1) v (k - 1 additions and the division)
Library functions on the device (the project's convention): the float32 CPU function against float64 over the case's own arguments,
4 x the largest deviation allowed, no other margin: expf 1.7e-07 relative over the recurrence arguments; the report prints it.
Measured on an MI355X, worst error / bound: beat localscore 0.17, cumscore 0.27 (in the twin alone no frame of any case is below the margin),
recurrence values 0.20, soft_kmeans r 0.39, mu 0.61, rows of r 0.48.

The constant envelope over 5000 frames at period 2047 is left out (segment_ref.beat_kinds): a third of its frames have two
candidates within 1e-13 of each other.  With period 1 the predecessor window reaches offset 0, whose penalty is -inf: it never
wins, in the reference and here."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import segment_ref as R  # noqa: E402
from cabi_guard import Buf, call, inp, ratio, refused, same  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
DEVS = {}


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), float(r))
    return r


def ints(a):
    return inp(np.asarray(a), torch.int32, guard=0)


# ---------------------------------------------------------------------------------------------------------------- beat tracker
def run_beat(env, period, tightness=100.0):
    T = env.size
    eb, ls, cum, back = inp(env), Buf(T, torch.float64), Buf(T, torch.float64), Buf(T, torch.int32)
    call("maua_beat_dp", eb.ptr, T, period, tightness, ls.ptr, cum.ptr, back.ptr)
    for b, what in ((ls, "localscore"), (cum, "cumscore"), (back, "backlink"), (eb, "envelope")):
        b.check(what)
    return ls.get(), cum.get(), back.get()


@pytest.mark.parametrize("period", R.BEAT_PERIODS)
def test_beat_dp(period):
    for T in R.beat_T(period):                               # 1, 2, period, 5000 (with period 2047 the ring of 4096 entries wraps)
        for kind in R.beat_kinds(T, period):                 # random, all zero, constant, a click train
            env = R.beat_input(T, period, kind, T + period)
            ls, cum, back = run_beat(env, period)
            want_ls, bound_ls = R.beat_localscore(env, period)
            assert note("beat_dp, localscore", ratio(ls, want_ls, bound_ls)) <= 1, (T, kind)
            if kind == "zeros":
                assert (ls == 0).all() and (cum == 0).all()
            dp = R.beat_dp(ls, period, 100.0)                # the twin's program on the device's own localscore
            assert note("beat_dp, cumscore", ratio(cum, dp["cumscore"], dp["err"])) <= 1, (T, kind)
            safe = dp["safe"]
            assert (~safe).sum() <= 0.01 * T, (T, kind)
            assert np.array_equal(back[safe], dp["backlink"][safe]), (T, kind)
            assert (back < np.arange(T)).all() and (back >= -2 * period - 1).all()


@pytest.mark.parametrize("period", R.BEAT_PERIODS)
def test_beat_dp_exact_ties(period):
    """the tie tightness makes every txwt a zero: the candidates are the cumulative scores themselves, whole windows tie exactly, and
    with no error anywhere every link and every cumulative score is compared bit for bit - the first maximum wins, within a lane
    and across the lanes (tests/test_segment_host.py: the last-maximum mutant differs on a quarter of the frames and more)"""
    T = R.beat_tie_T(period)                                 # 5000 at period 2047: ties across the ring's wrap
    for kind in R.BEAT_TIE_KINDS:
        env = R.beat_input(T, period, kind, 0)
        ls, cum, back = run_beat(env, period, R.BEAT_TIE_TIGHTNESS)
        dp = R.beat_dp(ls, period, R.BEAT_TIE_TIGHTNESS)
        assert dp["safe"].all() and (dp["err"] == 0).all()
        assert same(cum, dp["cumscore"]) and np.array_equal(back, dp["backlink"]), kind


def test_beat_dp_refusals():
    e, ls, cum, back = inp(np.ones(8)), Buf(8, torch.float64), Buf(8, torch.float64), Buf(8, torch.int32)
    refused("maua_beat_dp", e.ptr, 8, 2048, 100.0, ls.ptr, cum.ptr, back.ptr)
    refused("maua_beat_dp", e.ptr, 8, 0, 100.0, ls.ptr, cum.ptr, back.ptr)
    refused("maua_beat_dp", e.ptr, 8, 2, 0.0, ls.ptr, cum.ptr, back.ptr)
    refused("maua_beat_dp", None, 8, 2, 100.0, ls.ptr, cum.ptr, back.ptr)
    refused("maua_beat_dp", e.ptr, 8, 2, 100.0, None, cum.ptr, back.ptr)
    refused("maua_beat_dp", e.ptr, 8, 2, 100.0, ls.ptr, None, back.ptr)
    refused("maua_beat_dp", e.ptr, 8, 2, 100.0, ls.ptr, cum.ptr, None)
    call("maua_beat_dp", e.ptr, 0, 2, 100.0, ls.ptr, cum.ptr, back.ptr)
    assert ls.untouched() and cum.untouched() and back.untouched()


# ---------------------------------------------------------------------------------------------------------------- segment_reduce
@pytest.mark.parametrize("C", R.REDUCE_C)
def test_segment_reduce(C):
    for kind in ("ties", "integers", "random"):
        x, bounds = R.reduce_input(C, kind, C)               # segments of 1, 2, 3, 64 and 65 frames, two empty ones
        xb, bb = inp(x), ints(bounds)
        for mode in (0, 1):
            out = Buf((len(bounds) - 1) * C)
            call("maua_segment_reduce", xb.ptr, x.shape[0], C, bb.ptr, len(bounds) - 1, mode, out.ptr)
            out.check("segment_reduce", nan_ok=True)
            got = out.get().reshape(-1, C)
            assert same(got, R.segment_reduce(x, bounds, mode)), (kind, mode)
            assert np.isnan(got[np.diff(bounds) == 0]).all() and not np.isnan(got[np.diff(bounds) > 0]).any()
        xb.check("x")
        bb.check("bounds")
    out = Buf(4)
    call("maua_segment_reduce", xb.ptr, x.shape[0], C, bb.ptr, 0, 0, out.ptr)
    call("maua_segment_reduce", xb.ptr, x.shape[0], 0, bb.ptr, 2, 0, out.ptr)
    refused("maua_segment_reduce", xb.ptr, x.shape[0], C, bb.ptr, 2, 2, out.ptr)
    refused("maua_segment_reduce", xb.ptr, x.shape[0], C, bb.ptr, 2, -1, out.ptr)
    refused("maua_segment_reduce", xb.ptr, -1, C, bb.ptr, 2, 0, out.ptr)
    refused("maua_segment_reduce", None, x.shape[0], C, bb.ptr, 2, 0, out.ptr)
    refused("maua_segment_reduce", xb.ptr, x.shape[0], C, None, 2, 0, out.ptr)
    refused("maua_segment_reduce", xb.ptr, x.shape[0], C, bb.ptr, 2, 0, None)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- recurrence
@pytest.mark.parametrize("n", R.REC_N)
def test_recurrence_affinity(n):
    for kind in ("random", "duplicates", "constant"):        # duplicate rows: ties, lower row first; constant: the zero-median fallback
        data = R.recurrence_input(n, kind, n)
        db = inp(data)
        for width in R.REC_WIDTH:
            for k in sorted({1, min(2, n), n}):
                ref = R.recurrence_affinity(data, k, width)
                dev = R.measured_dev(np.exp, np.exp, [ref["arg"]])
                DEVS["expf, relative (recurrence_affinity)"] = max(DEVS.get("expf, relative (recurrence_affinity)", 0.0), dev)
                ref = R.recurrence_affinity(data, k, width, 4 * dev)
                assert ref["ambiguous"] == 0
                out = Buf(n * n)
                call("maua_recurrence_affinity", db.ptr, n, data.shape[1], k, width, out.ptr)
                out.check("recurrence_affinity")
                got = out.get().reshape(n, n)
                assert (got[~ref["kept"]] == 0).all(), (kind, width, k)
                big = ref["rec"] >= R.TINY
                assert (got[ref["kept"] & big] != 0).all(), (kind, width, k)
                assert note("recurrence_affinity, values", ratio(got, ref["rec"], np.maximum(ref["bound"], 1e-300))) <= 1, (kind, width, k)
                assert same(got, got.T)
        db.check("data")
    out = Buf(4)
    call("maua_recurrence_affinity", db.ptr, 0, 5, 1, 1, out.ptr)
    refused("maua_recurrence_affinity", db.ptr, n, 5, 0, 1, out.ptr)
    refused("maua_recurrence_affinity", db.ptr, n, 5, n + 1, 1, out.ptr)
    refused("maua_recurrence_affinity", db.ptr, R.REC_MAX_N + 1, 5, 1, 1, out.ptr)
    refused("maua_recurrence_affinity", None, n, 5, 1, 1, out.ptr)
    refused("maua_recurrence_affinity", db.ptr, n, 5, 1, 1, None)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- median filters
@pytest.mark.parametrize("n", (4, 5, 256, 257))
def test_timelag_median(n):
    rec = R.affinity_like(n, n)
    rb, out = inp(rec), Buf(n * n)
    call("maua_timelag_median", rb.ptr, n, out.ptr)
    out.check("timelag_median")
    rb.check("rec")
    assert same(out.get().reshape(n, n), R.timelag_median(rec))


def test_timelag_median_refusals():
    rb, out = inp(np.zeros(16)), Buf(16)
    refused("maua_timelag_median", rb.ptr, 3, out.ptr)
    refused("maua_timelag_median", rb.ptr, 4, rb.ptr)
    refused("maua_timelag_median", rb.ptr, R.REC_MAX_N + 1, out.ptr)
    refused("maua_timelag_median", None, 4, out.ptr)
    refused("maua_timelag_median", rb.ptr, 4, None)
    call("maua_timelag_median", rb.ptr, 0, out.ptr)
    assert out.untouched()
    rb.check("rec")


def run_median_rows(x, k):
    n, m = x.shape
    xb, out = inp(x), Buf(n * m)
    call("maua_median_filter_rows", xb.ptr, n, m, k, out.ptr)
    out.check("median_filter_rows")
    xb.check("x")
    return out.get().reshape(n, m)


@pytest.mark.parametrize("k", (1, 3, 15))
def test_median_filter_rows(k):
    for n in (k // 2 + 1, k // 2 + 2, 40):                   # n = k / 2 + 1: the shortest the reflect padding allows
        for m in (1, 257):
            x = R.f32(np.random.default_rng(n + m).integers(0, 6, size=(n, m)) / 2.0)
            assert same(run_median_rows(x, k), R.median_filter_rows(x, k)), (n, m)


def test_median_filter_rows_beyond_one_grid():
    """65537 rows: the row index no longer fits one launch's gridDim.y"""
    x = R.f32(np.random.default_rng(0).integers(0, 9, size=(65537, 1)))
    assert same(run_median_rows(x, 3), R.median_filter_rows(x, 3))


def test_median_filter_rows_refusals():
    xb, out = inp(np.zeros(64)), Buf(64)
    for k in (2, 16, 17, 0, -1):
        refused("maua_median_filter_rows", xb.ptr, 32, 2, k, out.ptr)
    refused("maua_median_filter_rows", xb.ptr, 7, 2, 15, out.ptr)
    refused("maua_median_filter_rows", xb.ptr, 32, 2, 3, xb.ptr)
    refused("maua_median_filter_rows", None, 32, 2, 3, out.ptr)
    refused("maua_median_filter_rows", xb.ptr, 32, 2, 3, None)
    call("maua_median_filter_rows", xb.ptr, 0, 2, 3, out.ptr)
    call("maua_median_filter_rows", xb.ptr, 32, 0, 3, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- soft k-means
@pytest.mark.parametrize("k", R.KM_K)
def test_soft_kmeans(k):
    for n in R.KM_N:
        data, mu0 = R.kmeans_input(n, k, n + k)
        db, mb = inp(data), inp(mu0)
        for iters in R.KM_ITERS:
            r_out, mu_out = Buf(n * k), Buf(k * k)
            call("maua_soft_kmeans", db.ptr, n, k, mb.ptr, iters, 5.0, r_out.ptr, mu_out.ptr)
            r_out.check("r")
            mu_out.check("mu")
            r, mu = r_out.get().reshape(n, k), mu_out.get().reshape(k, k)
            r64, mu64 = R.soft_kmeans(data, mu0, iters, 5.0)
            r32, mu32 = R.soft_kmeans(data, mu0, iters, 5.0, np.float32)
            dev_r, dev_mu = float(np.abs(r32 - r64).max()), float(np.abs(mu32 - mu64).max())
            print(f"[segment kernels] soft_kmeans k {k} n {n} iters {iters}: restatement deviation r {dev_r:.3e} mu {dev_mu:.3e}, "
                  f"device error r {np.abs(r - r64).max():.3e} mu {np.abs(mu - mu64).max():.3e}")
            assert note("soft_kmeans, r", ratio(r, r64, 4 * dev_r)) <= 1, (n, iters)
            assert note("soft_kmeans, mu", ratio(mu, mu64, 4 * dev_mu)) <= 1, (n, iters)
            assert note("soft_kmeans, rows of r sum to 1", ratio(r.astype(np.float64).sum(1), 1.0, (k + 1) * R.V)) <= 1, (n, iters)
            if iters == 0:
                assert same(mu, mu0)
        db.check("data")
        mb.check("mu0")
    r_out, mu_out = Buf(8), Buf(8)
    refused("maua_soft_kmeans", db.ptr, 4, 17, mb.ptr, 1, 5.0, r_out.ptr, mu_out.ptr)
    refused("maua_soft_kmeans", db.ptr, 4, 0, mb.ptr, 1, 5.0, r_out.ptr, mu_out.ptr)
    refused("maua_soft_kmeans", db.ptr, 0, 2, mb.ptr, 1, 5.0, r_out.ptr, mu_out.ptr)
    refused("maua_soft_kmeans", db.ptr, 4, 2, mb.ptr, -1, 5.0, r_out.ptr, mu_out.ptr)
    refused("maua_soft_kmeans", None, 4, 2, mb.ptr, 1, 5.0, r_out.ptr, mu_out.ptr)
    refused("maua_soft_kmeans", db.ptr, 4, 2, None, 1, 5.0, r_out.ptr, mu_out.ptr)
    refused("maua_soft_kmeans", db.ptr, 4, 2, mb.ptr, 1, 5.0, None, mu_out.ptr)
    refused("maua_soft_kmeans", db.ptr, 4, 2, mb.ptr, 1, 5.0, r_out.ptr, None)
    assert r_out.untouched() and mu_out.untouched()


def test_negative_sizes_are_refused():
    """a negative count is an error, never a launch that silently does nothing"""
    x, b, out, o64, oi = inp(np.ones(64)), ints(np.zeros(4)), Buf(64), Buf(8, torch.float64), Buf(8, torch.int32)
    refused("maua_beat_dp", x.ptr, -1, 2, 100.0, o64.ptr, o64.ptr, oi.ptr)
    refused("maua_segment_reduce", x.ptr, 8, 2, b.ptr, -1, 0, out.ptr)
    refused("maua_segment_reduce", x.ptr, 8, -2, b.ptr, 2, 0, out.ptr)
    refused("maua_recurrence_affinity", x.ptr, -4, 2, 1, 1, out.ptr)
    refused("maua_timelag_median", x.ptr, -4, out.ptr)
    refused("maua_median_filter_rows", x.ptr, -8, 2, 3, out.ptr)
    refused("maua_median_filter_rows", x.ptr, 8, -2, 3, out.ptr)
    refused("maua_soft_kmeans", x.ptr, -4, 2, x.ptr, 1, 5.0, out.ptr, out.ptr)
    assert out.untouched() and o64.untouched() and oi.untouched()


# ---------------------------------------------------------------------------------------------------------------- report
def test_zz_report():
    """the worst error / bound per family and the measured deviations of the library functions"""
    for k in sorted(WORST):
        print(f"[segment kernels] worst error / bound, {k}: {WORST[k]:.4f}")
    for k in sorted(DEVS):
        print(f"[segment kernels] float32 against float64 over the cases' arguments, {k}: {DEVS[k]:.3e} (4 x allowed)")
    assert all(v <= 1 for v in WORST.values())
