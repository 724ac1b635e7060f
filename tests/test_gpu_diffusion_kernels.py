"""The small kernels that hold the guided-diffusion path together - the sampler steps (csrc/sampler.hip), the two f32 kernels of the
timestep path (csrc/unet.hip) and the secondary model's glue (csrc/secondary.hip) - one entry point at a time, straight through the C
ABI, against the twin tests/diffusion_ref.py; the method of tests/test_gpu_latent_kernels.py: 4096 guard elements on both sides of
every buffer (tests/cabi_guard.py: NaN around inputs, a sentinel bit pattern in outputs; after each call the guards are intact, the
body is fully written and no NaN leaked in).  tests/test_diffusion_kernels_host.py holds the twin against the oracle and torch and
shows that the comparison made here (diffusion_ref.judge) rejects mutants of the twin at these very inputs, and that the contracted
and uncontracted restatements differ on them.

Exact, bit for bit with the uncontracted float32 restatement (the kernels switch contraction off; the device's float32 division is the
correctly rounded one): ddim_step, plms_eps, plms_update at every weight set, axpby_rows, p_sample_step's pred_xstart, mse_guide_grad
with its NaN rule, the pool, both masks, the skip gradient, both layout kernels, the bilinear map and its adjoint (order pinned in the
kernels), and the pass-through channels of sec_input / sec_output, in f32 and with one RNE in bf16.
Bounded (the bound next to its result in the twin; v = 2^-24; expf 3, sinf / cosf 4 float32 units of the float64 result):
p_sample_step's sample, timestep_embedding with the uploaded table and with the device's own frequencies, linear_rows, the
trigonometric channels of sec_input, pred and eps of sec_output.  test_zz_report prints the worst error / bound per family.
Measured on an MI355X, worst error / bound: p_sample_step sample 0.78, timestep_embedding 0.27 with the table and 0.25 with the
device's frequencies, linear_rows 0.22, sec_input 0.78, sec_output pred 0.32 and eps 0.29 (DESIGN_LOG.md section 15).
test_linear_rows samples the cross product: every (B, K, N), all four activation combinations at three (K, N) only, one combination
elsewhere, bias NULL on every third case."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

sys.path.insert(0, str(Path(__file__).resolve().parent))
import diffusion_ref as R  # noqa: E402
from cabi_guard import G, SENT, Buf, call, inp, refused, same  # noqa: E402

pytestmark = pytest.mark.gpu

WORST = {}
TD = {R.F32: torch.float32, R.BF16: torch.bfloat16}


def note(family, r):
    WORST[family] = max(WORST.get(family, 0.0), float(r))
    return r


def refused_with(text, name, *args):
    rc = getattr(L.lib(), name)(L.ctx(), *args)
    assert rc != 0, f"{name} accepted {args}"
    with pytest.raises(L.MauaHipError, match=text):
        L.check(rc)
    torch.cuda.synchronize()


def checked(bufs, what):
    for b in bufs:
        b.check(what)


# ---------------------------------------------------------------------------------------------------------------- sampler steps
def run_ddim(c, cf, grad, noise, pred=True, alias=False):
    n = c["x"].size
    xb, mb, gb, nb, cb = inp(c["x"]), inp(c["mo"]), inp(c["grad"]), inp(c["noise"]), inp(cf)
    sb, pb = (xb if alias else Buf(n)), (Buf(n) if pred else None)
    call("maua_ddim_step", xb.ptr, mb.ptr, gb.ptr if grad else None, nb.ptr if noise else None, cb.ptr, c["B"], c["C"], c["Cm"], c["HW"],
         sb.ptr, pb.ptr if pred else None)
    checked([b for b in (xb, mb, gb, nb, cb, sb, pb) if b is not None], "ddim_step")
    return sb.get().reshape(c["x"].shape), (pb.get().reshape(c["x"].shape) if pred else None)


@pytest.mark.parametrize("shape", R.SAMPLER_SHAPES)
def test_ddim_step(shape):
    B, Cc, HW = shape
    for Cm in R.cms(Cc):
        c = R.sampler_case(B, Cc, HW, Cm)
        for grad in (False, True):
            for noise in (False, True):
                cf = R.ddim_coef(c["t"], 0.5 if noise else 0.0)
                want_s, want_p = R.ddim_step32(c, cf, grad, noise)
                got_s, got_p = run_ddim(c, cf, grad, noise)
                assert R.judge(got_s, ("exact", want_s)) <= 1 and R.judge(got_p, ("exact", want_p)) <= 1, (Cm, grad, noise)
        got_s, got_p = run_ddim(c, cf, True, True, pred=False)
        assert got_p is None and R.judge(got_s, ("exact", want_s)) <= 1, "pred_xstart NULL"
        got_s, got_p = run_ddim(c, cf, True, True, alias=True)
        assert R.judge(got_s, ("exact", want_s)) <= 1 and R.judge(got_p, ("exact", want_p)) <= 1, "sample aliasing x"


def run_p_sample(c, cf, grad, pred=True, alias=False):
    n = c["x"].size
    xb, mb, gb, nb, cb = inp(c["x"]), inp(c["mo"]), inp(c["grad"]), inp(c["noise"]), inp(cf)
    sb, pb = (xb if alias else Buf(n)), (Buf(n) if pred else None)
    call("maua_p_sample_step", xb.ptr, mb.ptr, gb.ptr if grad else None, nb.ptr, cb.ptr, c["B"], c["C"], c["HW"], sb.ptr,
         pb.ptr if pred else None)
    checked([b for b in (xb, mb, gb, nb, cb, sb, pb) if b is not None], "p_sample_step")
    return sb.get().reshape(c["x"].shape), (pb.get().reshape(c["x"].shape) if pred else None)


@pytest.mark.parametrize("shape", R.SAMPLER_SHAPES)
def test_p_sample_step(shape):
    B, Cc, HW = shape
    c = R.sampler_case(B, Cc, HW, 2 * Cc, nan_rest=False)
    cf = R.p_coef(c["t"])
    for grad in (False, True):
        want_p, _, expect = R.p_sample(c, cf, grad)
        got_s, got_p = run_p_sample(c, cf, grad)
        assert R.judge(got_p, ("exact", want_p)) <= 1, grad
        assert note("p_sample_step sample", R.judge(got_s, expect)) <= 1, grad
    got_s, got_p = run_p_sample(c, cf, True, pred=False)
    assert got_p is None and R.judge(got_s, expect) <= 1
    got_s, got_p = run_p_sample(c, cf, True, alias=True)
    assert R.judge(got_s, expect) <= 1 and R.judge(got_p, ("exact", want_p)) <= 1


@pytest.mark.parametrize("shape", R.SAMPLER_SHAPES)
def test_plms_eps(shape):
    B, Cc, HW = shape
    for Cm in R.cms(Cc):
        c = R.sampler_case(B, Cc, HW, Cm)
        cf = R.ddim_coef(c["t"])
        n = c["x"].size
        for grad in (False, True):
            for outs in (3, 1):
                xb, mb, gb, cb = inp(c["x"]), inp(c["mo"]), inp(c["grad"]), inp(cf)
                ob = [Buf(n) for _ in range(outs)]
                call("maua_plms_eps", xb.ptr, mb.ptr, gb.ptr if grad else None, cb.ptr, B, Cc, Cm, HW, ob[0].ptr,
                     ob[1].ptr if outs == 3 else None, ob[2].ptr if outs == 3 else None)
                checked([xb, mb, gb, cb] + ob, "plms_eps")
                for got, want in zip(ob, R.plms_eps32(c, cf, grad)):
                    assert R.judge(got.get().reshape(c["x"].shape), ("exact", want)) <= 1, (Cm, grad, outs)


@pytest.mark.parametrize("shape", R.SAMPLER_SHAPES)
def test_plms_update(shape):
    B, Cc, HW = shape
    c = R.sampler_case(B, Cc, HW, Cc)
    cf = R.plms_coef(c["t"])
    n = c["x"].size
    for weights, div in R.PLMS_WEIGHTS:
        for alias in (False, True):
            xb, pb, cb = inp(c["x"]), inp(c["pred"]), inp(cf)
            eb = [inp(e) for e in c["eps"][:len(weights)]]
            sb = xb if alias else Buf(n)
            ptrs = (C.c_void_p * len(weights))(*[e.ptr.value for e in eb])
            ws = (C.c_float * len(weights))(*weights)
            call("maua_plms_update", xb.ptr, ptrs, ws, len(weights), div, pb.ptr, cb.ptr, B, Cc * HW, sb.ptr)
            checked([xb, pb, cb, sb] + eb, "plms_update")
            got = sb.get().reshape(c["x"].shape)
            assert R.judge(got, ("exact", R.plms_update32(c, cf, weights, div))) <= 1, (weights, alias)
            if B > 1:
                assert same(got[1], c["pred"][1]), "t = 0: the sample is pred_xstart"


@pytest.mark.parametrize("shape", R.SAMPLER_SHAPES)
def test_axpby_rows(shape):
    B, Cc, HW = shape
    c = R.sampler_case(B, Cc, HW, Cc)
    ab = R.q_coef(c["t"])
    for alias in (False, True):
        xb, yb, cb = inp(c["x"]), inp(c["noise"]), inp(ab)
        ob = xb if alias else Buf(c["x"].size)
        call("maua_axpby_rows", xb.ptr, yb.ptr, cb.ptr, B, Cc * HW, ob.ptr)
        checked([xb, yb, cb, ob], "axpby_rows")
        assert R.judge(ob.get().reshape(c["x"].shape), ("exact", R.axpby_rows32(c["x"], c["noise"], ab))) <= 1, alias


def test_sampler_empty_and_refusals():
    a, out = inp(np.zeros(16)), Buf(8)
    call("maua_ddim_step", a.ptr, a.ptr, None, None, a.ptr, 0, 3, 3, 4, out.ptr, None)
    call("maua_ddim_step", a.ptr, a.ptr, None, None, a.ptr, 1, 3, 3, 0, out.ptr, None)
    call("maua_axpby_rows", a.ptr, a.ptr, a.ptr, 1, 0, out.ptr)
    call("maua_mse_guide_grad", a.ptr, a.ptr, 0, 1.0, 0, 4, out.ptr)
    refused_with("maua_ddim_step", "maua_ddim_step", a.ptr, a.ptr, None, None, a.ptr, -1, 3, 3, 4, out.ptr, None)
    refused_with("maua_ddim_step", "maua_ddim_step", a.ptr, a.ptr, None, None, a.ptr, 1, 3, 3, -4, out.ptr, None)
    refused_with("maua_ddim_step", "maua_ddim_step", a.ptr, a.ptr, None, None, a.ptr, 1, 3, 2, 4, out.ptr, None)
    refused_with("maua_p_sample_step", "maua_p_sample_step", a.ptr, a.ptr, None, a.ptr, a.ptr, -1, 1, 4, out.ptr, None)
    refused_with("maua_plms_eps", "maua_plms_eps", a.ptr, a.ptr, None, a.ptr, 1, 1, 1, -4, out.ptr, None, None)
    refused_with("maua_axpby_rows", "maua_axpby_rows", a.ptr, a.ptr, a.ptr, 1, -4, out.ptr)
    refused_with("maua_mse_guide_grad", "maua_mse_guide_grad", a.ptr, a.ptr, 0, 1.0, -1, 4, out.ptr)
    refused("maua_ddim_step", None, a.ptr, None, None, a.ptr, 1, 1, 1, 4, out.ptr, None)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- mse_guide_grad
def run_mse(img, target, k, bstride):
    B, row = img.shape
    ib, tb, ob = inp(img), inp(target), Buf(B * row)
    call("maua_mse_guide_grad", ib.ptr, tb.ptr, bstride, k, B, row, ob.ptr)
    checked([ib, tb], "mse_guide_grad")
    ob.check("mse_guide_grad", nan_ok=True)
    return ob.get().reshape(B, row)


@pytest.mark.parametrize("B", (1, 3))
def test_mse_guide_grad(B):
    for row in (85, 64, 333):                       # B * row: 85, 255, 999 - partial last waves; 64, 192 - whole ones
        for per_sample in (False, True):
            img = R.normal((B, row), B + row)
            target = R.normal((B, row) if per_sample else (1, row), 2 * B + row)
            bstride = row if per_sample else 0
            for k in (0.37, 0.0):
                assert same(run_mse(img, target, k, bstride), R.mse_guide_grad32(img, target, k)), (row, per_sample, k)
            for where in (0, B * row - 1):          # a single NaN in the first / the very last element zeroes everything
                bad = img.copy()
                bad.reshape(-1)[where] = np.nan
                got = run_mse(bad, target, 0.37, bstride)
                assert not got.any() and not np.isnan(got).any(), (row, per_sample, where)
                # the flag is reset: a clean call right after returns the clean gradient
                assert same(run_mse(img, target, 0.37, bstride), R.mse_guide_grad32(img, target, 0.37)), (row, per_sample, where)
            big = img.copy()
            big.reshape(-1)[B * row // 2] = np.inf
            got = run_mse(big, target, 0.37, bstride)
            assert same(got, R.mse_guide_grad32(big, target, 0.37)) and np.isinf(got).sum() == 1, "an infinity without a NaN is kept"


# ---------------------------------------------------------------------------------------------------------------- timestep path
T_VALUES = (0.0, 1.0, 37.5, 999.0, 1000.0)


@pytest.mark.parametrize("dim", (2, 8, 9, 256))
def test_timestep_embedding(dim):
    for B in (1, 3, 100):
        t = R.f32([T_VALUES[(i + B) % len(T_VALUES)] for i in range(B)])
        for table in (True, False):
            tb, fb, eb = inp(t), inp(R.freqs32(dim)), Buf(B * dim)
            call("maua_timestep_embedding", tb.ptr, fb.ptr if table else None, B, dim, eb.ptr)
            checked([tb, fb, eb], "timestep_embedding")
            got = eb.get().reshape(B, dim)
            assert note("timestep_embedding " + ("table" if table else "device freqs"), R.judge(got, R.timestep_embedding(t, dim, table))) <= 1, (B, table)
            if dim & 1:
                assert not got[:, -1].any()
    t, out = inp(np.zeros(4)), Buf(8)
    call("maua_timestep_embedding", t.ptr, None, 0, 8, out.ptr)
    refused_with("maua_timestep_embedding", "maua_timestep_embedding", t.ptr, None, 1, 1, out.ptr)
    refused_with("maua_timestep_embedding", "maua_timestep_embedding", t.ptr, None, -1, 8, out.ptr)
    refused("maua_timestep_embedding", None, None, 1, 8, out.ptr)
    assert out.untouched()


LIN_SPECIALS = (-104.0, -88.0, 0.0, 88.0)


def run_linear(x, W, bias, ai, ao):
    B, K = x.shape
    N = W.shape[0]
    xb, wb, bb, yb = inp(x), inp(W), (inp(bias) if bias is not None else None), Buf(B * N)
    call("maua_linear_rows", xb.ptr, wb.ptr, bb.ptr if bb else None, B, K, N, ai, ao, yb.ptr)
    checked([b for b in (xb, wb, bb, yb) if b is not None], "linear_rows")
    return yb.get().reshape(B, N)


def linear_inputs(B, K, N, i):
    x, W = R.normal((B, K), 7 * B + K) * np.float32(2), R.normal((N, K), 3 * N + K) / np.float32(np.sqrt(K))
    x.reshape(-1)[:min(4, x.size)] = LIN_SPECIALS[:min(4, x.size)]
    return x, W, (None if i % 3 == 0 else R.normal((N,), N))


@pytest.mark.parametrize("B", (1, 8, 9, 16, 17, 100))
def test_linear_rows(B):
    i = 0
    for K in (1, 63, 64, 65, 200):
        for N in (1, 3, 4, 5, 130):
            x, W, bias = linear_inputs(B, K, N, i)
            acts = ((0, 0), (0, 1), (1, 0), (1, 1)) if (K, N) in ((65, 5), (200, 130), (1, 1)) else (((i >> 1) & 1, i & 1),)
            for ai, ao in acts:
                got = run_linear(x, W, bias, ai, ao)
                assert note("linear_rows", R.judge(got, R.linear_rows(x, W, bias, ai, ao))) <= 1, (K, N, ai, ao)
            i += 1
    # the outer SiLU at the overflow side: W = 1, no bias, so the product is x itself
    x = R.f32([LIN_SPECIALS[j % 4] for j in range(B)]).reshape(B, 1)
    got = run_linear(x, R.f32([[1.0]]), None, 0, 1)
    assert note("linear_rows", R.judge(got, R.linear_rows(x, R.f32([[1.0]]), None, 0, 1))) <= 1 and np.isfinite(got).all()


def test_linear_rows_empty_and_refusals():
    a, out = inp(np.zeros(16)), Buf(8)
    call("maua_linear_rows", a.ptr, a.ptr, None, 0, 4, 4, 0, 0, out.ptr)
    call("maua_linear_rows", a.ptr, a.ptr, None, 2, 4, 0, 0, 0, out.ptr)
    for bad in ((-1, 4, 4), (1, -4, 4), (1, 4, -4)):
        refused_with("maua_linear_rows", "maua_linear_rows", a.ptr, a.ptr, None, *bad, 0, 0, out.ptr)
    refused_with("maua_linear_rows", "maua_linear_rows", a.ptr, a.ptr, None, 1, 4, 4, 2, 0, out.ptr)
    refused("maua_linear_rows", None, a.ptr, None, 1, 4, 4, 0, 0, out.ptr)
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------- secondary glue
def dbuf(a, dtype):
    return inp(a, TD[dtype])


def strided_result(out, shape, Cc, what):
    """an output with a pixel stride beyond C: the C channels written, the gap left as it was"""
    out.check(what, written=False, nan_ok=True)
    bits = out._bits()[G:G + out.n].cpu().numpy().reshape(shape)
    assert (bits[..., Cc:] == np.array(SENT[out.es]).astype(bits.dtype)).all(), f"{what}: the gap between pixels was written"
    assert (bits[..., :Cc] != np.array(SENT[out.es]).astype(bits.dtype)).all(), f"{what}: elements of the result were never written"
    got = out.get().reshape(shape)[..., :Cc]
    assert not np.isnan(got).any(), f"{what}: NaN in the result (a gap or a guard was read)"
    return got


GLUE_CASES = [(g, p, d, w) for d in (R.F32, R.BF16) for p in R.GLUE_PIECES for w in (False, True) for g in R.GLUE_GRIDS]


@pytest.mark.parametrize("grid,pieces,dtype,wide", GLUE_CASES)
def test_secondary_glue(grid, pieces, dtype, wide):
    B, H, W = grid
    c = R.glue_case(B, H, W, pieces, dtype, wide)
    Cc, st = c["C"], c["stride"]
    h, w = H // 2, W // 2
    # pool
    sb, ob = dbuf(c["fine"], dtype), Buf(B * h * w * Cc, TD[dtype])
    call("maua_avgpool2_nhwc", sb.ptr, st, B, H, W, Cc, dtype, ob.ptr)
    checked([sb, ob], "avgpool2")
    assert R.judge(ob.get().reshape(B, h, w, Cc), ("exact", R.avgpool2_32(c["fine"][..., :Cc], dtype))) <= 1
    # bilinear x2 into a strided destination
    sb, ob = dbuf(c["coarse"], dtype), Buf(B * H * W * st, TD[dtype])
    call("maua_bilinear_up2_nhwc", sb.ptr, B, h, w, Cc, dtype, ob.ptr, st)
    sb.check("bilinear_up2")
    got = strided_result(ob, (B, H, W, st), Cc, "bilinear_up2")
    assert R.judge(got, ("exact", R.bilinear_up2_32(c["coarse"], dtype))) <= 1
    # its adjoint, with and without the mask
    for act in (None, c["act_coarse"]):
        gb, ab, ob = dbuf(c["fine"], dtype), (dbuf(act, dtype) if act is not None else None), Buf(B * h * w * Cc, TD[dtype])
        call("maua_bilinear_up2_nhwc_vjp", gb.ptr, st, ab.ptr if ab else None, B, h, w, Cc, dtype, ob.ptr)
        checked([b for b in (gb, ab, ob) if b is not None], "bilinear_up2_vjp")
        assert R.judge(ob.get().reshape(B, h, w, Cc), ("exact", R.bilinear_up2_adjoint32(c["fine"][..., :Cc], act, dtype))) <= 1, act is None
    # the ReLU mask, in place
    gb, ab = dbuf(c["gdense"], dtype), dbuf(c["act_fine"], dtype)
    call("maua_relu_mask_nhwc", gb.ptr, ab.ptr, st, B * H * W, Cc, dtype)
    checked([gb, ab], "relu_mask")
    assert R.judge(gb.get().reshape(B, H, W, Cc), ("exact", R.relu_mask32(c["gdense"], c["act_fine"][..., :Cc], dtype))) <= 1
    # the skip gradient
    gb, ab, pb, ob = dbuf(c["fine"], dtype), dbuf(c["act_fine"], dtype), dbuf(c["coarse"], dtype), Buf(B * H * W * Cc, TD[dtype])
    call("maua_skip_grad_nhwc", gb.ptr, ab.ptr, st, pb.ptr, B, H, W, Cc, dtype, ob.ptr)
    checked([gb, ab, pb, ob], "skip_grad")
    assert R.judge(ob.get().reshape(B, H, W, Cc), ("exact", R.skip_grad32(c["fine"][..., :Cc], c["act_fine"][..., :Cc], c["coarse"], dtype))) <= 1


@pytest.mark.parametrize("dtype", (R.F32, R.BF16))
def test_secondary_input_output_and_layout(dtype):
    wemb = R.normal((8,), 5)
    for B in (1, 2):
        for HW in (1, 37, 300):
            x, vn = R.normal((B, 3, HW), B + HW), R.store(R.normal((B, HW, 32), 2 * B + HW), dtype)
            g = R.normal((B, 3, HW), 3 * B + HW)
            for t0 in (0.0, 0.3, 1.0):
                t = R.f32([t0, 1.0 - t0][:B])
                xb, tb, wb, ob = inp(x), inp(t), inp(wemb), Buf(B * HW * 32, TD[dtype])
                call("maua_secondary_input", xb.ptr, tb.ptr, wb.ptr, B, HW, dtype, ob.ptr)
                checked([xb, tb, wb, ob], "secondary_input")
                got = ob.get().reshape(B, HW, 32)
                exact, expect = R.sec_input(x, t, wemb, dtype)
                assert same(got[..., :3], exact[..., :3]) and not got[..., 19:].any()
                assert note("sec_input", R.judge(got, expect)) <= 1, (B, HW, t0)
                want_v, e_pred, e_eps = R.sec_output(vn, x, t, dtype)
                for outs in ((1, 1, 1), (0, 1, 0), (1, 0, 1)):
                    vb, xb, tb = dbuf(vn, dtype), inp(x), inp(t)
                    ob = [Buf(B * 3 * HW) if on else None for on in outs]
                    call("maua_secondary_output", vb.ptr, xb.ptr, tb.ptr, B, HW, dtype, *[b.ptr if b else None for b in ob])
                    checked([vb, xb, tb] + [b for b in ob if b], "secondary_output")
                    if ob[0]:
                        assert same(ob[0].get().reshape(B, 3, HW), want_v)
                    if ob[1]:
                        assert note("sec_output pred", R.judge(ob[1].get().reshape(B, 3, HW), e_pred)) <= 1, (B, HW, t0)
                    if ob[2]:
                        assert note("sec_output eps", R.judge(ob[2].get().reshape(B, 3, HW), e_eps)) <= 1, (B, HW, t0)
            gb, ob = inp(g), Buf(B * HW * 32, TD[dtype])
            call("maua_secondary_grad_layout", gb.ptr, B, HW, dtype, 1, ob.ptr)
            checked([gb, ob], "grad_layout in")
            assert R.judge(ob.get().reshape(B, HW, 32), ("exact", R.grad_to_nhwc(g, dtype))) <= 1
            vb, ob = dbuf(vn, dtype), Buf(B * 3 * HW)
            call("maua_secondary_grad_layout", vb.ptr, B, HW, dtype, 0, ob.ptr)
            checked([vb, ob], "grad_layout out")
            assert R.judge(ob.get().reshape(B, 3, HW), ("exact", R.grad_from_nhwc(vn, dtype))) <= 1


def test_secondary_glue_empty_and_refusals():
    a, out = inp(np.zeros(256)), Buf(64)
    call("maua_avgpool2_nhwc", a.ptr, 4, 0, 2, 2, 4, R.F32, out.ptr)
    call("maua_bilinear_up2_nhwc", a.ptr, 1, 0, 1, 4, R.F32, out.ptr, 4)
    call("maua_skip_grad_nhwc", a.ptr, a.ptr, 4, a.ptr, 1, 2, 0, 4, R.F32, out.ptr)
    call("maua_secondary_input", a.ptr, a.ptr, a.ptr, 1, 0, R.F32, out.ptr)
    call("maua_secondary_grad_layout", a.ptr, 0, 4, R.F32, 1, out.ptr)
    refused_with("maua_avgpool2_nhwc", "maua_avgpool2_nhwc", a.ptr, 4, 1, 3, 2, 4, R.F32, out.ptr)
    refused_with("maua_avgpool2_nhwc", "maua_avgpool2_nhwc", a.ptr, 3, 1, 2, 2, 4, R.F32, out.ptr)
    refused_with("maua_avgpool2_nhwc", "maua_avgpool2_nhwc", a.ptr, 4, -1, 2, 2, 4, R.F32, out.ptr)
    refused_with("maua_bilinear_up2_nhwc", "maua_bilinear_up2_nhwc", a.ptr, 1, 1, 1, 4, R.BF16, out.ptr, 8)
    refused_with("maua_bilinear_up2_nhwc_vjp", "maua_bilinear_up2_nhwc_vjp", a.ptr, 4, None, 1, 1, 1, 4, 7, out.ptr)
    refused_with("maua_skip_grad_nhwc", "maua_skip_grad_nhwc", a.ptr, a.ptr, 4, a.ptr, 1, 2, 3, 4, R.F32, out.ptr)
    refused_with("maua_relu_mask_nhwc", "maua_relu_mask_nhwc", out.ptr, a.ptr, 4, -1, 4, R.F32)
    refused_with("maua_secondary_output", "maua_secondary_output", a.ptr, a.ptr, a.ptr, -1, 4, R.F32, out.ptr, None, None)
    assert out.untouched()


def test_zz_report():
    for k in sorted(WORST):
        print(f"worst error / bound  {k:40s} {WORST[k]:.3f}")
