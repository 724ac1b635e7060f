"""The cellular automaton's step kernel (csrc/nca.hip) through maua_amd.nca.CA, against the float64 restatement tests/nca_ref.py.

Exact family (nca_ref.exact_family; tests/test_nca_host.py proves it exact in float32 in any order and as hi + lo bf16): compared bit for
bit in both product modes, on grids smaller than a tile (3 x 3, 5 x 7), spanning tiles with a remainder in both directions (20 x 36,
19 x 70), B in {1, 2, 3}, the three instantiation paths (12/96, 16/128, 4/32 zero-padded), 1, 3 and 5 steps (both ping-pong parities), the
scalar-rate, map-rate, caller-u and in-kernel Philox forms, and window mode.  The state lies inside a NaN-guarded buffer that must come back
untouched outside the state.

Gaussian family (the reference's own recorded inputs, tests/golden/g40_nca.npz): inside nca_ref's element-wise bound - the float32 unit per
operation of every sum, plus 2^-16 of each product in split mode - around the float64 restatement, and the reference's float32 result
inside the same bound."""
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent))
import nca_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "g40_nca.npz"
G = 4096
MODES = ("f32", "split")


@pytest.fixture(scope="module")
def g40():
    return R.load_g40(GOLDEN)


def make_ca(w1, b1, w2, products, seed=0, stream=0, k=1):
    from maua_amd import nca
    hidden, k1 = w1.shape
    ca = nca.CA(k1 // 4, hidden, products=products, seed=seed, stream=stream, steps_per_launch=k)
    ca.load_state_dict({"w1.weight": torch.from_numpy(np.ascontiguousarray(w1)).reshape(hidden, k1, 1, 1), "w1.bias": torch.from_numpy(np.ascontiguousarray(b1)),
                        "w2.weight": torch.from_numpy(np.ascontiguousarray(w2)).reshape(k1 // 4, hidden, 1, 1)})
    return ca.cuda()


class Guarded:
    """a state inside a NaN-filled buffer: .x is the view the kernel gets, .check() asserts the guards are untouched"""

    def __init__(self, x):
        x = np.ascontiguousarray(x, dtype=np.float32)
        self.buf = torch.full((x.size + 2 * G,), float("nan"), device="cuda")
        self.x = self.buf[G:G + x.size].view(*x.shape)
        self.x.copy_(torch.from_numpy(x))

    def check(self):
        assert bool(torch.isnan(self.buf[:G]).all()) and bool(torch.isnan(self.buf[-G:]).all()), "the kernel wrote outside the state"

    def numpy(self):
        return self.x.cpu().numpy()


def same_bits(got, want64):
    want = np.asarray(want64).astype(np.float32)
    assert np.array_equal(want.astype(np.float64), want64), "the expected result is not a float32"
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("products", MODES)
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_family_bit_for_bit(case, products):
    seed, b, c, h, w, hidden, n, dense = case
    x, w1, b1, w2, u = R.exact_family(seed, b, c, h, w, hidden, n, dense)
    ca = make_ca(w1, b1, w2, products, seed=5, stream=9)
    # the caller's uniforms, scalar rate
    s = Guarded(x)
    ca.step(s.x, n, 0.5, u=torch.from_numpy(u))
    s.check()
    same_bits(s.numpy(), R.steps(x, w1, b1, w2, u))
    # a rate map
    rmap = np.random.default_rng(seed).random((h, w), dtype=np.float32)
    s = Guarded(x)
    ca.step(s.x, n, torch.from_numpy(rmap), u=torch.from_numpy(u))
    s.check()
    same_bits(s.numpy(), R.steps(x, w1, b1, w2, u, rmap))
    # the in-kernel Philox draws from step 7 on
    up = np.stack([R.philox_u(5, 9, 7 + t, b, h, w) for t in range(n)])
    s = Guarded(x)
    ca.step(s.x, n, 0.5, step0=7)
    s.check()
    same_bits(s.numpy(), R.steps(x, w1, b1, w2, up))
    # forward_keep: every state, the input left as it is
    s = Guarded(x)
    states = ca.forward_keep(s.x, n, 0.5, u=torch.from_numpy(u))
    s.check()
    assert np.array_equal(s.numpy(), x)
    same_bits(states.cpu().numpy(), R.steps(x, w1, b1, w2, u, keep=True))


@pytest.mark.parametrize("products", MODES)
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("case", R.EXACT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_exact_family_several_steps_per_launch(case, k, products):
    """k steps per launch (a k-pixel halo advanced inside the workgroup): 1, 3 and 5 steps - launches of k, then the remainder as 2 and 1,
    either ping-pong parity - on grids smaller than the halo (3 x 3 wraps onto itself several times), across tiles with remainders, B = 3,
    all three instantiations; the caller's uniforms with a rate map, and the in-kernel draws"""
    seed, b, c, h, w, hidden, n, dense = case
    x, w1, b1, w2, u = R.exact_family(seed, b, c, h, w, hidden, n, dense)
    ca = make_ca(w1, b1, w2, products, seed=5, stream=9, k=k)
    s = Guarded(x)
    ca.step(s.x, n, 0.5, u=torch.from_numpy(u))
    s.check()
    same_bits(s.numpy(), R.steps(x, w1, b1, w2, u))
    rmap = np.random.default_rng(seed).random((h, w), dtype=np.float32)
    s = Guarded(x)
    ca.step(s.x, n, torch.from_numpy(rmap), u=torch.from_numpy(u))
    s.check()
    same_bits(s.numpy(), R.steps(x, w1, b1, w2, u, rmap))
    up = np.stack([R.philox_u(5, 9, 7 + t, b, h, w) for t in range(n)])
    s = Guarded(x)
    ca.step(s.x, n, 0.5, step0=7)
    s.check()
    same_bits(s.numpy(), R.steps(x, w1, b1, w2, up))


@pytest.mark.parametrize("products", MODES)
def test_several_steps_per_launch_same_bits_on_gaussian_inputs(g40, products):
    """9 steps (k = 4: 4 + 4 + 1, k = 2: four launches and one) of Gaussian states with Philox masks: k = 2 and k = 4 give k = 1's bits -
    below a tile (5 x 7, B = 2), 20 x 36, and 19 x 70 with B = 2 (tiles with remainders in both directions)"""
    rng = np.random.default_rng(12)
    cases = [("a", g40["a_x0"]), ("b", g40["b_x0"]), ("b", rng.standard_normal((2, 12, 19, 70)).astype(np.float32))]
    for p, x0 in cases:
        prm = [g40[f"{p}_{k}"] for k in ("w1", "b1", "w2")]
        got = {}
        for k in (1, 2, 4):
            s = Guarded(x0)
            make_ca(*prm, products, seed=3, stream=1, k=k).step(s.x, 9, 0.5, step0=2)
            s.check()
            got[k] = s.numpy()
        assert np.isfinite(got[1]).all() and not np.array_equal(got[1], x0)
        for k in (2, 4):
            assert np.array_equal(got[k].view(np.uint32), got[1].view(np.uint32)), (x0.shape, k)


def test_several_steps_per_launch_refusals(g40):
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    ca = make_ca(*prm, "f32", k=4)
    x = torch.from_numpy(g40["g_x0"]).cuda()
    before = x.clone()
    ca.step(x, 1, window=(0, 7, 1))                              # window mode runs one step per launch whatever the module's k
    assert not torch.equal(x, before)
    states = ca.forward_keep(torch.from_numpy(g40["a_x0"]).cuda(), 3)     # ... and so does forward_keep
    assert states.shape[0] == 4


@pytest.mark.parametrize("products", MODES)
def test_window_mode_bit_for_bit(products):
    x, w1, b1, w2, u = R.exact_family(11, 2, 12, 6, 12, 96, 3, False)
    ca = make_ca(w1, b1, w2, products)
    s = Guarded(x)
    for i, win in enumerate(R.WINDOWS):
        ca.step(s.x, 1, 0.5, u=torch.from_numpy(u[i:i + 1]), window=win)
    s.check()
    same_bits(s.numpy(), R.window_rounds(x, w1, b1, w2, u))
    # two steps in one window call = two calls
    s2, s3 = Guarded(x), Guarded(x)
    ca.step(s2.x, 2, 0.5, u=torch.from_numpy(u[:2]), window=R.WINDOWS[1])
    for i in range(2):
        ca.step(s3.x, 1, 0.5, u=torch.from_numpy(u[i:i + 1]), window=R.WINDOWS[1])
    assert np.array_equal(s2.numpy(), s3.numpy())
    want = x
    for i in range(2):
        want = R.window_step(want, w1, b1, w2, u[i], *R.WINDOWS[1])
    same_bits(s2.numpy(), want)


def within(name, got, want64, bound):
    err = np.abs(got.astype(np.float64) - want64)
    ratio = float((err / bound).max())
    print(f"{name}: max error {err.max():.3e}, worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, name


@pytest.mark.parametrize("products", MODES)
def test_gaussian_family_on_recorded_inputs(g40, products):
    split = products == "split"
    for p, checks in (("a", [(n, g40["a_traj"][n - 1]) for n in range(1, 6)]), ("b", [(1, g40["b_x1"]), (5, g40["b_x5"])])):
        prm = [g40[f"{p}_{k}"] for k in ("w1", "b1", "w2")]
        ca = make_ca(*prm, products)
        for n, recorded in checks:
            x = torch.from_numpy(g40[f"{p}_x0"]).cuda()
            ca.step(x, n, 0.5, u=torch.from_numpy(g40[f"{p}_u"][:n]))
            want, bound = R.steps_bound(g40[f"{p}_x0"], *prm, g40[f"{p}_u"][:n], split=split)
            within(f"{p} {n} steps {products}", x.cpu().numpy(), want, bound)
            _, bound32 = R.steps_bound(g40[f"{p}_x0"], *prm, g40[f"{p}_u"][:n])
            within(f"{p} {n} steps, the reference", recorded, want, bound32)
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    ca = make_ca(*prm, products)
    x = torch.from_numpy(g40["a_x0"]).cuda()
    ca.step(x, 1, torch.from_numpy(g40["m_map"]), u=torch.from_numpy(g40["m_u"]))
    want, bound = R.step(g40["a_x0"], *prm, g40["m_u"][0], g40["m_map"], bound=0.0, split=split)
    within(f"rate map {products}", x.cpu().numpy(), want, bound)
    within("rate map, the reference", g40["m_x1"], want, bound)


@pytest.mark.parametrize("products", MODES)
def test_recorded_checkpoint_grid_round(g40, products):
    split = products == "split"
    x, w = torch.from_numpy(g40["g_x0"]).cuda(), int(g40["g_w"])
    for ci, p in enumerate("ab"):
        ca = make_ca(*[g40[f"{p}_{k}"] for k in ("w1", "b1", "w2")], products)
        u = np.zeros((1, 1) + tuple(x.shape[2:]), dtype=np.float32)
        u[..., ci * w:ci * w + w + 2] = g40["g_u"][ci]
        ca.step(x, 1, 0.5, u=torch.from_numpy(u), window=(ci * w, w + 2, 1))
    want = R.checkgrid_round(g40)
    ones = np.zeros((1, 6, 12), np.float32)
    _, b0 = R.step(g40["g_x0"], g40["a_w1"], g40["a_b1"], g40["a_w2"], ones, 1.0, bound=0.0, split=split)
    _, b1 = R.step(want, g40["b_w1"], g40["b_b1"], g40["b_w2"], ones, 1.0, bound=b0, split=split)
    within(f"checkpoint grid {products}", x.cpu().numpy(), want, b1)
    within("checkpoint grid, the reference", g40["g_x1"], want, b1)


def test_device_masks_equal_the_twin():
    """w1 = 0, b1 = 1, w2[0, 0] = 1: channel 0 of one step from zero IS the mask, the other channels stay zero"""
    b, h, w, hidden = 3, 5, 7, 96
    w1, b1, w2 = np.zeros((hidden, 48), np.float32), np.ones(hidden, np.float32), np.zeros((12, hidden), np.float32)
    w2[0, 0] = 1
    rmap = np.linspace(0, 1, h * w, dtype=np.float32).reshape(h, w)
    for products in MODES:
        ca = make_ca(w1, b1, w2, products, seed=(1 << 40) + 3, stream=(1 << 33) + 1)
        for t in (0, 1, 6, (1 << 31) + 5):               # the last: the word index passes 2^32 and the counter's low word wraps
            u = R.philox_u((1 << 40) + 3, (1 << 33) + 1, t, b, h, w)
            for rate in (0.0, 0.5, float(np.float32(1 - 2.0 ** -24)), rmap):
                x = torch.zeros(b, 12, h, w, device="cuda")
                ca.step(x, 1, torch.from_numpy(rate) if isinstance(rate, np.ndarray) else rate, step0=t)
                got = x.cpu().numpy()
                assert np.array_equal(got[:, 0], R.mask_of(u, rate)) and not got[:, 1:].any(), (products, t)


@pytest.mark.parametrize("products", MODES)
def test_split_calls_carry_the_stream(g40, products):
    prm = [g40[f"b_{k}"] for k in ("w1", "b1", "w2")]
    ca = make_ca(*prm, products, seed=3)
    one = torch.from_numpy(g40["b_x0"]).cuda()
    ca.step(one, 5, step0=10)
    two = torch.from_numpy(g40["b_x0"]).cuda()
    ca.step(two, 2, step0=10)
    ca.step(two, 3, step0=12)
    assert torch.equal(one, two)
    run = torch.from_numpy(g40["b_x0"]).cuda()           # the module's own running count does the same
    ca.steps_done = 10
    ca.step(run, 2)
    ca.step(run, 3)
    assert torch.equal(one, run) and ca.steps_done == 15
    kept = ca.forward_keep(torch.from_numpy(g40["b_x0"]).cuda(), 5, step0=10)
    assert torch.equal(kept[5], one) and torch.equal(kept[2], ca.step(torch.from_numpy(g40["b_x0"]).cuda(), 2, step0=10))
    other = torch.from_numpy(g40["b_x0"]).cuda()
    ca.step(other, 5, step0=11)
    assert not torch.equal(one, other)


def test_forward_returns_a_new_state_and_refusals(g40):
    from maua_amd import _lib as L
    ca = make_ca(*[g40[f"a_{k}"] for k in ("w1", "b1", "w2")], "f32")
    x = torch.from_numpy(g40["a_x0"]).cuda()
    y = ca(x)
    assert y.data_ptr() != x.data_ptr() and torch.equal(x.cpu(), torch.from_numpy(g40["a_x0"])) and not torch.equal(x, y)
    with pytest.raises(L.MauaHipError, match="at least 3"):
        ca.step(torch.zeros(1, 12, 2, 8, device="cuda"))
    with pytest.raises(ValueError, match="contiguous float32"):
        ca.step(torch.zeros(1, 8, 8, 8, device="cuda"))
    from maua_amd import nca
    with pytest.raises(L.MauaHipError, match="multiple of 4 up to 16"):
        nca.CA(20, 96).cuda().step(torch.zeros(1, 20, 8, 8, device="cuda"))


class Collect:
    """a writer in ffmpeg's place: keeps the frames it is handed"""

    def __init__(self):
        self.frames = []

    def write(self, t):
        self.frames.append(t.cpu().numpy())


def test_render_frames_equal_the_restatement():
    from maua_amd import nca
    x0, w1, b1, w2, _ = R.exact_family(21, 1, 12, 32, 32, 96, 3, False)
    ca = make_ca(w1, b1, w2, "f32", seed=4)
    sink = Collect()
    nca.render_evolution(ca, sink.write, num_frames=3, size=32)
    x = np.zeros_like(x0)                                  # the renderer starts from the zero state; the biases move it
    for k in range(3):
        x = R.step(x, w1, b1, w2, R.philox_u(4, 0, k, 1, 32, 32))
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
        want = np.repeat(np.repeat(R.to_u8(x[:, :3]), 2, 1), 2, 2)
        assert sink.frames[k].shape == (1, 64, 64, 3) and np.array_equal(sink.frames[k], want), k
    assert len(sink.frames) == 3 and sink.frames[2].any()


def test_checkgrid_video_equals_the_restatement():
    from maua_amd import nca
    xa, w1a, b1a, w2a, _ = R.exact_family(22, 1, 12, 6, 12, 96, 2, False)
    _, w1b, b1b, w2b, _ = R.exact_family(23, 1, 12, 6, 12, 96, 2, False)
    models = [make_ca(w1a, b1a, w2a, "f32"), make_ca(w1b, b1b, w2b, "f32")]
    sink = Collect()
    nca.render_checkgrid(models, sink.write, num_frames=2, strip=5, rows=6, rounds=2, x=torch.from_numpy(xa).cuda())
    x, t = xa.astype(np.float64), 0
    for k in range(2):
        for _ in range(2):
            u = R.philox_u(0, 0, t, 1, 6, 12)
            x = R.window_step(x, w1a, b1a, w2a, u, 0, 7, 1)
            x = R.window_step(x, w1b, b1b, w2b, u, 5, 7, 1)
            t += 1
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x) and np.abs(x).max() < 2 ** 16
        assert np.array_equal(sink.frames[k], np.repeat(np.repeat(R.to_u8(x[:, :3]), 2, 1), 2, 2)), k


# ---- the steps' gradient (csrc/nca_vjp.hip) ---------------------------------------------------------------------------------------------

def run_vjp(ca, x0, u, g_last, rate=0.5, step0=None):
    uu = None if u is None else torch.from_numpy(u)
    n = len(u) if u is not None else 3
    states = ca.forward_keep(torch.from_numpy(x0).cuda(), n, rate, u=uu, step0=step0 or 0)
    out = ca.backward(states, torch.from_numpy(g_last).cuda(), rate, u=uu, step0=step0 or 0)
    return states.cpu().numpy(), [t.cpu().numpy().reshape(t.shape[0], -1) if t.ndim == 4 and t.shape[-1] == 1 else t.cpu().numpy() for t in out]


@pytest.mark.parametrize("case", [R.EXACT_CASES[7], R.EXACT_CASES[9], R.EXACT_CASES[4], R.EXACT_CASES[5]], ids=lambda c: "x".join(map(str, c)))
def test_vjp_exact_family_bit_for_bit(case):
    """integer states, parameters and g_last: every product and sum of the walk is an integer below 2^24 (asserted), so any order gives
    the same bits; tiles with remainders, B = 3, the 16/128 and zero-padded 4/32 instantiations"""
    seed, b, c, h, w, hidden, n, dense = case
    x, w1, b1, w2, u = R.exact_family(seed, b, c, h, w, hidden, n, dense)
    g_last = np.random.default_rng(seed).integers(-2, 3, x.shape).astype(np.float32)
    ca = make_ca(w1, b1, w2, "f32")
    states, got = run_vjp(ca, x, u, g_last)
    same_bits(states, R.steps(x, w1, b1, w2, u, keep=True))
    want = R.vjp(states, w1, b1, w2, u, g_last)
    assert R.vjp_magnitude(states, w1, b1, w2, u, g_last) < 2 ** 24, "the exact case leaves the float32 integers"
    for name, g, wnt in zip(("g_first", "dw1", "db1", "dw2"), got, want):
        assert wnt.any(), name
        same_bits(g.reshape(wnt.shape), wnt)


def test_vjp_against_restatement_and_recorded_autograd(g40):
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    ca = make_ca(*prm, "f32")
    states, got = run_vjp(ca, g40["v_x0"], g40["v_u"], g40["v_g_last"])
    want, bound = R.vjp(states, *prm, g40["v_u"], g40["v_g_last"], bound=True)       # fed the device's own stored states
    for name, g, w, b in zip(("g_first", "dw1", "db1", "dw2"), got, want, bound):
        within(f"vjp {name}", g.reshape(w.shape), w, b)
    # autograd ran on the reference's float32 states: the distance between the two sets of states goes through the gradient as well
    states64 = R.steps(g40["v_x0"], *prm, g40["v_u"], keep=True)
    far = R.vjp(states64, *prm, g40["v_u"], g40["v_g_last"])
    near = R.vjp(R.steps(g40["v_x0"], *prm, g40["v_u"], keep=True, dtype=np.float32), *prm, g40["v_u"], g40["v_g_last"])
    for name, g, w, b, f, nr in zip(("g_first", "dw1", "db1", "dw2"), got, want, bound, far, near):
        within(f"vjp {name} against autograd", g.reshape(w.shape), g40[f"v_{name}"].reshape(w.shape).astype(np.float64),
               2 * b + np.abs(w - f) + np.abs(nr - f))


def test_vjp_twice_identical_bits_and_philox_masks(g40):
    prm = [g40[f"b_{k}"] for k in ("w1", "b1", "w2")]
    ca = make_ca(*prm, "f32", seed=8)
    g_last = np.random.default_rng(1).standard_normal(g40["b_x0"].shape).astype(np.float32)
    s1, a = run_vjp(ca, g40["b_x0"], None, g_last, step0=4)
    s2, b = run_vjp(ca, g40["b_x0"], None, g_last, step0=4)
    assert np.array_equal(s1, s2) and all(np.array_equal(p.view(np.uint32), q.view(np.uint32)) for p, q in zip(a, b))
    u = np.stack([R.philox_u(8, 0, 4 + t, 1, 20, 36) for t in range(3)])          # the in-kernel masks are the twin's, forward and backward
    s3, c = run_vjp(ca, g40["b_x0"], u, g_last)
    assert np.array_equal(s1, s3) and all(np.array_equal(p, q) for p, q in zip(a, c))


def test_vjp_through_a_zero_mask(g40):
    prm = [g40[f"a_{k}"] for k in ("w1", "b1", "w2")]
    ca = make_ca(*prm, "f32")
    _, (g, dw1, db1, dw2) = run_vjp(ca, g40["v_x0"], g40["v_u"], g40["v_g_last"], rate=0.0)
    assert np.array_equal(g, g40["v_g_last"]) and not dw1.any() and not db1.any() and not dw2.any()
    states = ca.forward_keep(torch.from_numpy(g40["v_x0"]).cuda(), 0)
    out = ca.backward(states, torch.from_numpy(g40["v_g_last"]).cuda(), step0=0)
    with pytest.raises(ValueError, match="step0"):
        ca.backward(states, torch.from_numpy(g40["v_g_last"]).cuda())
    assert torch.equal(out[0].cpu(), torch.from_numpy(g40["v_g_last"])) and not any(bool(t.any()) for t in out[1:])


def test_perception_operator(g40):
    from maua_amd import nca
    x, *_ = R.exact_family(2, 3, 12, 5, 7, 96, 1, True)
    same_bits(nca.perception(torch.from_numpy(x).cuda()).cpu().numpy(), R.perception(x))
    for key in ("a_x0", "b_x0"):
        got = nca.perception(torch.from_numpy(g40[key]).cuda()).cpu().numpy()
        within(f"perception {key}", got, R.perception(g40[key]), 9 * R.EPS * R._abs_perception(g40[key]) + 1e-300)
    assert nca.perception(torch.zeros(1, 5, 3, 3, device="cuda")).shape == (1, 20, 3, 3)


def test_generate_writes_the_three_videos(tmp_path):
    """generate() end to end with a collecting writer: file naming, frame sizes and counts, the checkpoint list, and the rate-map video's
    frames against the restatement (exact family, so the bytes are equal)"""
    from maua_amd import nca
    x0, w1, b1, w2, _ = R.exact_family(31, 1, 12, 32, 32, 96, 3, False)
    ca = make_ca(w1, b1, w2, "f32")
    for tag in ("500", "1000", "7500"):
        nca.save(ca, tmp_path / f"style_{tag}.pt")
    sinks = {}

    class Writer(Collect):
        def __init__(self, path, size, fps):
            super().__init__()
            self.size = size
            sinks[Path(path).name] = self

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            return False
    rmap = np.random.default_rng(3).random((32, 32), dtype=np.float32)
    nca.generate(tmp_path / "style_7500.pt", tmp_path, num_frames=3, size=32, grid=(32, 15), checkpoints=[tmp_path / "style_500.pt", tmp_path / "style_1000.pt"],
                 rate_map=torch.from_numpy(rmap), products="f32", writer=Writer)
    assert sorted(sinks) == ["style-7500-wav.mp4", "style_7500.mp4", "style_checkgrid.mp4"]
    evo, grid, wav = sinks["style_7500.mp4"], sinks["style_checkgrid.mp4"], sinks["style-7500-wav.mp4"]
    assert evo.size == (64, 64) and [f.shape for f in evo.frames] == [(1, 64, 64, 3)] * 3
    assert grid.size == (2 * (15 * 2 + 2), 64) and [f.shape for f in grid.frames] == [(1, 64, 64, 3)] * 3
    assert wav.size == (64, 64) and len(wav.frames) == 3
    x, xe = np.zeros((1, 12, 32, 32)), np.zeros((1, 12, 32, 32))
    for k in range(3):
        x = R.step(x, w1, b1, w2, R.philox_u(0, 0, k, 1, 32, 32), rmap)
        xe = R.step(xe, w1, b1, w2, R.philox_u(0, 0, k, 1, 32, 32))
        assert np.array_equal(x.astype(np.float32).astype(np.float64), x) and np.array_equal(xe.astype(np.float32).astype(np.float64), xe)
        assert np.array_equal(wav.frames[k], np.repeat(np.repeat(R.to_u8(x[:, :3]), 2, 1), 2, 2)), k
        assert np.array_equal(evo.frames[k], np.repeat(np.repeat(R.to_u8(xe[:, :3]), 2, 1), 2, 2)), k
    assert evo.frames[2].any()
