"""What tests/test_gpu_segment_kernels.py rests on, checked without a GPU: the twin tests/segment_ref.py against independent
implementations (scipy.signal.convolve, torch.median, oracle/segment.py, the pad / roll / median / roll / crop of
timelag_median_filter written literally), the preconditions of the exact families per input (squared distances and sums exactly
representable; at most 1 % of a beat case's frames decided by less than the derived margin), and that every comparison rejects
off-by-one mutants of the twin."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

try:
    from scipy import signal as sps
except ImportError:                                         # (numpy.convolve then)
    sps = None

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import segment_ref as R  # noqa: E402
from oracle import segment as OS  # noqa: E402

V = R.V


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def inside(got, want, bound):
    err = np.abs(np.asarray(got, dtype=np.float64) - want)
    return bool(np.isfinite(err).all() and (err <= bound).all())


# ----------------------------------------------------------------------------------------------------------------- beat tracker
@pytest.mark.parametrize("period", R.BEAT_PERIODS)
def test_beat_twin_against_scipy_and_the_oracle(period):
    gw, offsets, txwt = R.beat_tables(period, 100.0)
    assert gw.size == 2 * period + 1 and gw[period] == 1.0 and offsets[0] == -2 * period and offsets[-1] == -int(np.rint(period / 2.0))
    assert (period == 1) == bool(np.isinf(txwt).any()), "period 1: the offset 0, log(0)"
    for T in R.beat_T(period):
        for kind in R.beat_kinds(T, period):
            env = R.beat_input(T, period, kind, T + period)
            ls, bound = R.beat_localscore(env, period)
            conv = (lambda a, b, mode: sps.convolve(a, b, mode, method="direct")) if sps else np.convolve
            want = conv(env.astype(np.float64), gw, "same") if T >= gw.size else conv(gw, env.astype(np.float64), "full")[period:period + T]
            assert inside(ls, want, bound + 1e-300), (T, kind)
            dp = R.beat_dp(ls, period, 100.0)
            # at most 1 % of the frames may be decided by less than the margin (the GPU test leaves those out)
            assert (~dp["safe"]).sum() <= 0.01 * T, (T, kind, int((~dp["safe"]).sum()))
            if kind != "zeros" and T > 1:                   # (the oracle returns early on silence and divides by its own std)
                scale = env.astype(np.float32).std(ddof=1)
                if scale > 0:
                    _, ols, ocum, oback = _oracle_dp(env, period)
                    assert inside(ols, ls, bound + 1e-300)
                    mine = R.beat_dp(ols, period, 100.0)
                    assert inside(mine["cumscore"], ocum, mine["err"] + 1e-300) and same(mine["backlink"][mine["safe"]], oback[mine["safe"]]), (T, kind)


def _oracle_dp(env, period):
    """oracle.beat_track on an envelope that is already normalised: its own loop, fed the same window"""
    env = np.asarray(env, np.float32)
    window = np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2)
    ls = np.convolve(env.astype(np.float64), window, "full")[period:period + len(env)]
    back, cum = np.zeros(len(env), np.int64), np.zeros(len(env))
    offsets = np.arange(-2 * period, -np.round(period / 2) + 1, dtype=int)
    with np.errstate(divide="ignore"):
        txwt = -100.0 * (np.log(-offsets / period) ** 2)
    first, smax = True, ls.max()
    for i, score_i in enumerate(ls):
        prev = offsets + i
        cand = txwt.copy()
        ok = prev >= 0
        cand[ok] += cum[prev[ok]]
        j = int(np.argmax(cand))
        cum[i] = score_i + cand[j]
        if first and score_i < 0.01 * smax:
            back[i] = -1
        else:
            back[i] = prev[j]
            first = False
    return None, ls, cum, back


def test_beat_oracle_loop_is_the_oracles():
    """the loop above is oracle/segment.py's own (which normalises first): the same links on an envelope with unit deviation"""
    env = R.beat_input(400, 7, "random", 1)
    bpm = 60.0 * (22050 / 1024) / 7
    _, ols, ocum, oback = OS.beat_track(env, bpm)
    _, ls, cum, back = _oracle_dp((env / env.std(ddof=1)).astype(np.float32), 7)
    assert np.abs(ols - ls).max() <= 1e-12 * np.abs(ls).max() and same(oback, back) and np.abs(ocum - cum).max() <= 1e-9 * np.abs(cum).max()


@pytest.mark.parametrize("period", R.BEAT_PERIODS)
def test_beat_exact_ties_take_the_first_maximum(period):
    """with the tie tightness every txwt is a zero, no candidate carries an error (every frame is comparable) and whole windows tie
    exactly: the first maximum is the earliest predecessor, the mutant that takes the last one is rejected on every tie case"""
    _, offsets, txwt = R.beat_tables(period, R.BEAT_TIE_TIGHTNESS)
    assert (txwt[np.isfinite(txwt)] == 0).all() and np.isfinite(txwt).sum() >= 2
    T = R.beat_tie_T(period)
    for kind in R.BEAT_TIE_KINDS:
        ls = R.beat_localscore(R.beat_input(T, period, kind, 0), period)[0]
        dp = R.beat_dp(ls, period, R.BEAT_TIE_TIGHTNESS)
        last = R.beat_dp(ls, period, R.BEAT_TIE_TIGHTNESS, mutant="last_max")
        assert dp["safe"].all() and (dp["err"] == 0).all(), kind
        differ = dp["backlink"] != last["backlink"]
        assert differ.sum() >= T // 4, (kind, int(differ.sum()))
        assert (dp["backlink"][differ] < last["backlink"][differ]).all(), "the first maximum is the earlier frame"
        if kind == "zeros":
            assert same(dp["backlink"], np.arange(T) - 2 * period)


def test_beat_ring_wraps():
    """T = 5000 with period 2047: the look-back reaches 4094 frames, the ring of 4096 entries wraps"""
    assert 2 * R.BEAT_MAX_PERIOD + 2 == 4096 and 5000 > 4096
    dp = R.beat_dp(R.beat_localscore(R.beat_input(5000, 2047, "clicks", 3), 2047)[0], 2047, 100.0)
    assert (dp["backlink"][4200:] >= 0).all() and (dp["backlink"][4200:] < np.arange(4200, 5000)).all()


# ----------------------------------------------------------------------------------------------------------------- reductions
@pytest.mark.parametrize("C", R.REDUCE_C)
def test_segment_reduce_against_torch_and_the_oracle(C):
    for kind in ("ties", "integers", "random"):
        x, bounds = R.reduce_input(C, kind, C)
        lens = np.diff(bounds)
        assert set(R.REDUCE_L) <= set(lens.tolist()) and 0 in lens and bounds[0] == 0 and bounds[-1] == x.shape[0]
        med, mean = R.segment_reduce(x, bounds, 0), R.segment_reduce(x, bounds, 1)
        for s, (lo, hi) in enumerate(zip(bounds[:-1], bounds[1:])):
            if hi == lo:
                assert np.isnan(med[s]).all() and np.isnan(mean[s]).all()
                continue
            assert same(med[s], torch.median(torch.from_numpy(x[lo:hi]), dim=0).values.numpy()), (kind, s)
            exact = x[lo:hi].astype(np.float64).mean(0)
            assert inside(mean[s], exact, (hi - lo + 1) * V * np.abs(x[lo:hi].astype(np.float64)).mean(0) + 1e-300)
            if kind == "integers":                          # sums below 2^24: exact, the mean is the one division
                assert np.abs(x[lo:hi]).sum(0).max() < 2 ** 24 and same(mean[s], (x[lo:hi].astype(np.float64).sum(0) / (hi - lo)).astype(np.float32))
    x, bounds = R.reduce_input(C, "random", 0)
    nz = np.diff(bounds) > 0
    b2 = np.concatenate(([0], bounds[1:][nz]))
    assert same(R.segment_reduce(x, b2, 0), OS.sync(x, b2[1:-1])), "without the empty segments: the oracle's sync"


@pytest.mark.parametrize("n", R.REC_N)
def test_recurrence_against_the_oracle(n):
    for kind in ("random", "duplicates", "constant"):
        data = R.recurrence_input(n, kind, n)
        d64 = data.astype(np.float64)
        sq = ((d64[:, None] - d64[None]) ** 2).sum(2)
        assert sq.max() < 2 ** 24 and same(sq, np.round(sq)), "squared distances are exact integers"
        for width in R.REC_WIDTH:
            for k in sorted({1, min(2, n), n}):
                ref = R.recurrence_affinity(data, k, width)
                assert ref["bw"] > 0 and ref["ambiguous"] == 0
                if kind == "constant" and n == 257 and k == 1:
                    assert ref["fallback"] and (~(R.recurrence_affinity(data, k, width)["kept"])).all(1).sum() > n // 2, "the zero-median fallback is reached"
                if ref["fallback"] or width == 0:           # (the reference divides by the zero median: NaN; it takes no width below 1)
                    continue
                want = OS.recurrence_matrix(data, k=k, width=width)
                ref = R.recurrence_affinity(data, k, width, 4 * R.measured_dev(np.exp, np.exp, [ref["arg"]]))
                big = ref["rec"] >= R.TINY
                assert same((want != 0) & big, ref["kept"] & big) and (want[~ref["kept"]] == 0).all(), (kind, width, k)
                assert inside(want, ref["rec"], ref["bound"]), (kind, width, k)
    dup = R.recurrence_input(9, "duplicates", 1)
    assert same(dup[0], dup[1]) and same(dup[1], dup[2])


@pytest.mark.parametrize("n", (4, 5, 16, 257))
def test_timelag_median_is_the_literal_filter(n):
    rec = R.affinity_like(n, n)
    got = R.timelag_median(rec)
    assert same(got, R.timelag_literal(rec)) and same(got, OS.timelag_median_filter(rec))


@pytest.mark.parametrize("k", (1, 3, 15))
def test_median_filter_rows_against_torch_and_the_oracle(k):
    for n in (k // 2 + 1, k // 2 + 2, 40):
        for m in (1, 5):
            x = R.affinity_like(max(n, m), n + m)[:n, :m] + R.f32(np.random.default_rng(n).integers(0, 3, size=(n, m)))
            got = R.median_filter_rows(x, k)
            assert same(got, OS.median_filter1d(x.T, k, k // 2).T), (n, m)
            pad = torch.nn.functional.pad(torch.from_numpy(x.T.copy())[None], (k // 2, k // 2), mode="reflect")[0] if k > 1 else torch.from_numpy(x.T.copy())
            want = pad.unfold(1, k, 1).median(dim=-1).values.numpy().T
            assert same(got, want), (n, m)


@pytest.mark.parametrize("k", R.KM_K)
def test_soft_kmeans_against_the_oracle(k):
    for n in R.KM_N:
        data, mu0 = R.kmeans_input(n, k, n + k)
        assert np.abs(np.linalg.norm(data.astype(np.float64), axis=1) - 1).max() <= 2e-7
        for iters in R.KM_ITERS:
            r64, mu64 = R.soft_kmeans(data, mu0, iters, 5.0)
            r32, mu32 = R.soft_kmeans(data, mu0, iters, 5.0, np.float32)
            omu, orr, _ = OS.soft_kmeans(data, k, iters, 5.0, mu0)
            dev_r, dev_mu = np.abs(r32 - r64).max(), np.abs(mu32 - mu64).max()
            assert r32.dtype == np.float32 and mu32.dtype == np.float32
            # the oracle (float32 in numpy's own order) sits inside the bound the GPU test uses: 4 x the restatement's deviation
            assert np.abs(orr - r64).max() <= 4 * dev_r + 1e-300 or np.abs(orr - r64).max() <= 1e-6, (n, iters)
            assert np.abs(omu - mu64).max() <= 4 * dev_mu + 1e-300 or np.abs(omu - mu64).max() <= 1e-6, (n, iters)
            assert np.abs(r64.sum(1) - 1).max() <= 1e-15 * k and np.abs(r32.astype(np.float64).sum(1) - 1).max() <= (k + 1) * V
            if iters == 0:
                assert same(mu32, mu0)


# ----------------------------------------------------------------------------------------------------------------- mutants
def test_mutants_are_rejected():
    env = R.beat_input(600, 7, "random", 5)
    ls = R.beat_localscore(env, 7)[0]
    dp = R.beat_dp(ls, 7, 100.0)
    m = R.beat_dp(ls, 7, 100.0, mutant="j+1")
    assert not same(dp["backlink"][dp["safe"]], m["backlink"][dp["safe"]]) and not inside(m["cumscore"], dp["cumscore"], dp["err"])
    sil = ls.copy()
    sil[:20] = 0.0
    sil[20] = 0.01 * sil.max()                              # exactly at the threshold: < keeps it as the first beat, <= does not
    assert not same(R.beat_dp(sil, 7, 100.0)["backlink"], R.beat_dp(sil, 7, 100.0, mutant="le")["backlink"])
    x, bounds = R.reduce_input(5, "ties", 1)
    for mode in (0, 1):
        good = R.segment_reduce(x, bounds, mode)
        for mut in ("hi+1", "lo+1") + (("upper",) if mode == 0 else ()):
            assert not same(good, R.segment_reduce(x, bounds, mode, mutant=mut)), (mode, mut)
    data = R.recurrence_input(30, "duplicates", 2)
    ref = R.recurrence_affinity(data, 4, 1, 1e-6)
    for mut in ("k+1", "k-1", "width+1", "last_first"):
        other = R.recurrence_affinity(data, 4, 1, mutant=mut)
        assert not (same(other["kept"], ref["kept"]) and inside(other["rec"], ref["rec"], ref["bound"])), mut
    data = R.recurrence_input(30, "random", 2)              # (an even count whose two middle row maxima differ)
    ref = R.recurrence_affinity(data, 4, 1, 1e-6)
    assert not inside(R.recurrence_affinity(data, 4, 1, mutant="upper")["rec"], ref["rec"], ref["bound"]), "upper median"
    rec = R.affinity_like(9, 3)
    for mut in ("edge_repeat", "row+1", "mod_n", "upper"):
        assert not same(R.timelag_median(rec), R.timelag_median(rec, mutant=mut)), mut
    xm = R.f32(np.random.default_rng(4).integers(0, 50, size=(12, 3)))
    for k in (3, 15):
        for mut in ("edge_repeat", "row+1", "upper"):
            assert not same(R.median_filter_rows(xm, k), R.median_filter_rows(xm, k, mutant=mut)), (k, mut)
