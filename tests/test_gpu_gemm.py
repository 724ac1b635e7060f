"""The four GEMM kernels behind launch_gemm_nt (csrc/gemm.hip, csrc/gemm_dma.hip), each forced through maua_gemm_nt_ex and through
production routing, against float64 references at their edges: M tails of every tile height, N tails, one / two / an odd number of K
chunks, two A sources split off chunk boundaries, bias and residual present or absent, row strides wider than the rows, batched
launches, the QuickGELU epilogues, and byte offsets past 2^31.

Main family: integer operands in [-8, 8] and integer biases.  Every partial sum stays below 2^24, so the f32 accumulation is exact in
any order and the expected output is exact: bf16(bf16(S + b) + r) for bf16, S + b + r for f32 (S = A W^T in float64), compared with
torch.equal.  K is chosen so that |S| often exceeds 256 and bf16's rounding (ties included) really runs.  Second family: Gaussian
operands, element-wise against float64 within 2u |ref| + K 2^-24 (|A| |W|^T + |b|), doubled with a residual (whose own rounding of
the bias-added value adds 2u |S + b| in bf16).

Guard regions: input padding and the 256 rows after M hold NaN, output padding and the rows after M a sentinel bit pattern; the
result must hold no NaN and every sentinel must survive (every address a kernel could touch is allocated)."""
import ctypes as C

import numpy as np
import pytest
import torch

from maua_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
TILE = {1: 64, 2: 128, 3: 256, 4: 256}
GUARD = 256                     # rows after M in every M-row buffer (a whole tile of the tallest kernel)
SENT = {torch.bfloat16: 0x5A5A, torch.float32: 0x5A5A5A5A}
IVIEW = {torch.bfloat16: torch.int16, torch.float32: torch.int32}
U = {torch.bfloat16: 2.0 ** -8, torch.float32: 2.0 ** -24}


def _dt_id(dt):
    return L.BF16 if dt == torch.bfloat16 else L.F32


def _launch(d, dt, dma, force):
    return L.lib().maua_gemm_nt_ex(L.ctx(), C.byref(d), _dt_id(dt), dma, force)


def _route_remap(d, dt, dma):
    remap = C.c_int(0)
    k = L.lib().maua_gemm_nt_route(C.byref(d), _dt_id(dt), dma, C.byref(remap))
    L.check(min(k, 0))
    return k, remap.value


def _route(d, dt, dma):
    return _route_remap(d, dt, dma)[0]


def _sync():
    torch.cuda.synchronize()


def _sent_fill(rows, cols, dt):
    t = torch.empty((rows, cols), dtype=dt, device=DEV)
    t.view(IVIEW[dt]).fill_(SENT[dt])
    return t


def _padded(x, ld, dt, guard=GUARD):
    """device copy of host [rows][cols] x in a [rows + guard][ld] buffer whose padding and guard rows hold NaN"""
    t = torch.full((x.shape[0] + guard, ld), float("nan"), dtype=dt, device=DEV)
    t[:x.shape[0], :x.shape[1]] = x.to(dt).to(DEV)
    return t


def _bits(t):
    return t.view(IVIEW[t.dtype])


class Problem:
    """host float64 operands, device buffers with guard regions, the exact / float64 reference"""

    def __init__(self, M, N, K0, K1=0, dt=torch.bfloat16, bias=True, res=True, pad=16, family="int", seed=0):
        g = torch.Generator().manual_seed(seed * 1000003 + M * 31 + N * 7 + K0 * 3 + K1)
        K = K0 + K1
        if family == "int":
            draw = lambda *s: torch.randint(-8, 9, s, generator=g).double()
            bdraw = lambda n: torch.randint(-64, 65, (n,), generator=g).double()
        else:
            draw = lambda *s: torch.randn(*s, generator=g).to(dt).double()
            bdraw = lambda n: torch.randn(n, generator=g).float().double()
        self.M, self.N, self.K0, self.K1, self.dt, self.family = M, N, K0, K1, dt, family
        self.A = draw(M, K)
        self.W = draw(N, K)
        self.b = bdraw(N) if bias else None
        self.r = draw(M, N) if res else None
        self.lda0, self.lda1, self.ldc, self.ldr = K0 + pad, K1 + pad, N + pad, N + 2 * pad
        self.a0 = _padded(self.A[:, :K0], self.lda0, dt)
        self.a1 = _padded(self.A[:, K0:], self.lda1, dt) if K1 else None
        self.w = self.W.to(dt).to(DEV).contiguous()
        self.bd = self.b.float().to(DEV) if bias else None
        self.rd = _padded(self.r, self.ldr, dt) if res else None
        self.c = _sent_fill(M + GUARD, self.ldc, dt)

    def desc(self, M=None, c=None, **kw):
        d = L.GemmDesc(a0=self.a0.data_ptr(), lda0=self.lda0, K0=self.K0,
                       a1=self.a1.data_ptr() if self.K1 else None, lda1=self.lda1, K1=self.K1, w=self.w.data_ptr(),
                       bias=self.bd.data_ptr() if self.bd is not None else None,
                       res=self.rd.data_ptr() if self.rd is not None else None, ldr=self.ldr,
                       c=(self.c if c is None else c).data_ptr(), ldc=self.ldc, M=self.M if M is None else M, N=self.N)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def sb(self, rows=slice(None)):
        s = self.A[rows] @ self.W.T
        return s + self.b if self.b is not None else s

    def want(self, rows=slice(None)):
        """exact expected output (integer family)"""
        v = self.sb(rows)
        if self.dt == torch.bfloat16:
            v = v.to(torch.bfloat16).double()
            return (v + self.r[rows]).to(torch.bfloat16) if self.r is not None else v.to(torch.bfloat16)
        return (v + self.r[rows]).float() if self.r is not None else v.float()

    def got(self, c=None):
        return (self.c if c is None else c)[:self.M, :self.N].cpu()

    def check_guards(self, c=None, M=None):
        c = self.c if c is None else c
        M = self.M if M is None else M
        assert not torch.isnan(c[:M, :self.N]).any(), "NaN in the result: a kernel read padding past K or past a row"
        bits = _bits(c).cpu()
        assert (bits[:M, self.N:] == SENT[self.dt]).all(), "a store past N"
        assert (bits[M:] == SENT[self.dt]).all(), "a store past M"

    def check_exact(self, c=None):
        got, want = self.got(c), self.want()
        if not torch.equal(got, want):
            bad = (got.double() != want.double()).nonzero()
            raise AssertionError(f"{len(bad)} of {got.numel()} outputs differ, first at {bad[0].tolist()}: "
                                 f"got {got[tuple(bad[0])].item()} want {want[tuple(bad[0])].item()}")

    def check_close(self, c=None):
        """Gaussian family: element-wise error bound against float64"""
        K = self.K0 + self.K1
        sb = self.sb()
        ref = sb + self.r if self.r is not None else sb
        mag = self.A.abs() @ self.W.abs().T + (self.b.abs() if self.b is not None else 0)
        u = U[self.dt]
        tol = 2 * u * ref.abs() + K * 2.0 ** -24 * mag
        if self.r is not None:
            tol = 2 * tol + (2 * u * sb.abs() if self.dt == torch.bfloat16 else 0)
        err = (self.got(c).double() - ref).abs()
        assert (err <= tol).all(), f"max excess {(err - tol).max().item()}"


def run(p, force, dma=0, **kw):
    d = p.desc(**kw)
    L.check(_launch(d, p.dt, dma, force))
    _sync()
    return d


# ---- every kernel, forced and through production routing, at its edges
SPLITS = {
    (1, torch.bfloat16): [(32, 0), (64, 0), (160, 0), (32, 64), (96, 160), (64, 32), (224, 96)],
    (1, torch.float32): [(16, 0), (32, 0), (80, 0), (48, 32), (16, 48)],
    (2, torch.bfloat16): [(64, 0), (128, 0), (320, 0), (64, 128), (192, 64)],
    (2, torch.float32): [(32, 0), (64, 0), (160, 0), (32, 64), (96, 32)],
    (3, torch.bfloat16): [(64, 0), (128, 0), (320, 0), (64, 128), (192, 64)],
    (4, torch.bfloat16): [(64, 0), (128, 0), (320, 0)],
}
NS = {1: [32, 96, 128, 160, 384, 1024, 1152], 2: [32, 96, 128, 160, 384, 1024, 1152], 3: [128, 384, 1024, 1152],
      4: [256, 1024, 512]}


def _edge_cases():
    out = []
    for (k, dt), splits in SPLITS.items():
        t = TILE[k]
        ms = [1, t - 1, t, t + 1, 11 * t + 37]
        for i in range(max(len(ms), len(NS[k]), len(splits))):
            K0, K1 = splits[i % len(splits)]
            out.append(pytest.param(k, dt, ms[i % len(ms)], NS[k][i % len(NS[k])], K0, K1, i % 2 == 0, (i // 2) % 2 == 0,
                                    0 if i == 0 else 8 * (1 + i % 3),
                                    id=f"k{k}-{str(dt)[6:]}-M{ms[i % len(ms)]}-N{NS[k][i % len(NS[k])]}-K{K0}+{K1}-"
                                       f"b{int(i % 2 == 0)}r{int((i // 2) % 2 == 0)}"))
    return out


@pytest.mark.parametrize("kernel,dt,M,N,K0,K1,bias,res,pad", _edge_cases())
def test_kernel_edges_exact(kernel, dt, M, N, K0, K1, bias, res, pad):
    p = Problem(M, N, K0, K1, dt, bias, res, pad)
    for force in (kernel, 0):
        p.c.view(IVIEW[dt]).fill_(SENT[dt])
        run(p, force, dma=1 if kernel >= 3 else 0)
        p.check_guards()
        p.check_exact()


@pytest.mark.parametrize("dt,K0,K1", [(torch.bfloat16, 128, 0), (torch.bfloat16, 64, 128), (torch.float32, 64, 0)])
@pytest.mark.parametrize("N", [256, 1024])
def test_kernel2_xcd_remap_exact(dt, K0, K1, N):
    """kernel 2 with its XCD remap on (2 .. 8 N tiles over >= 64 M tiles, as the UNet's batched 1x1 layers and the CLIP tower
    without the DMA kernels run it): 65 M tiles, so the remapped grid rounds up to 72 and its last row groups return early"""
    M = 64 * 128 + 37
    p = Problem(M, N, K0, K1, dt, True, True, 8)
    assert _route_remap(p.desc(), dt, 0) == (2, N // 128)
    for force in (2, 0):
        p.c.view(IVIEW[dt]).fill_(SENT[dt])
        run(p, force)
        p.check_guards()
        p.check_exact()


@pytest.mark.parametrize("kernel,dt", [(1, torch.float32), (2, torch.float32), (1, torch.bfloat16), (2, torch.bfloat16),
                                       (3, torch.bfloat16), (4, torch.bfloat16)])
@pytest.mark.parametrize("res", [False, True])
def test_kernel_gaussian_within_float64_bound(kernel, dt, res):
    t = TILE[kernel]
    K0, K1 = SPLITS[(kernel, dt)][-1 if kernel != 4 else 2]
    for M, N in ((t + 1, NS[kernel][-1]), (11 * t + 37, NS[kernel][1])):
        p = Problem(M, N, K0, K1, dt, True, res, 8, family="gauss", seed=1)
        run(p, kernel)
        p.check_guards()
        p.check_close()


def test_forced_kernels_refuse_what_they_cannot_compute():
    p = Problem(300, 384, 64, 0, torch.bfloat16, True, True, 8)
    for force in (2, 3, 4):                                              # kernels 2 - 4 read the residual in 16-byte pieces
        assert _launch(p.desc(ldr=p.N + 4), p.dt, 1, force) != 0
    assert _launch(p.desc(epi=1, c2=p.c.data_ptr(), ldc2=p.ldc), p.dt, 1, 1) != 0
    q = Problem(300, 384, 64, 64, torch.bfloat16, True, False, 8)
    assert _launch(q.desc(), q.dt, 1, 4) != 0                          # two A sources / N % 256
    assert _launch(q.desc(), q.dt, 1, 5) != 0
    f = Problem(300, 256, 64, 0, torch.float32, True, False, 8)
    assert _launch(f.desc(), f.dt, 1, 3) != 0
    assert _launch(f.desc(), f.dt, 1, 4) != 0
    _sync()
    for pr in (p, q, f):
        assert (_bits(pr.c).cpu() == _bits(_sent_fill(1, 1, pr.dt)).cpu()[0, 0]).all(), "a refused call launched"


# ---- agreement across kernels and across M
def test_all_kernels_give_the_same_bits():
    p = Problem(300, 256, 192, 0, torch.bfloat16, True, True, 8)
    outs = []
    for force in (1, 2, 3, 4):
        c = _sent_fill(*p.c.shape, p.dt)
        run(p, force, c=c)
        p.check_guards(c)
        outs.append(p.got(c))
    for k, o in enumerate(outs[1:], 2):
        assert torch.equal(o, outs[0]), f"kernel {k} differs from kernel 1"
    assert torch.equal(outs[0], p.want())
    f = Problem(300, 256, 96, 32, torch.float32, True, True, 8)
    c1, c2 = _sent_fill(*f.c.shape, f.dt), _sent_fill(*f.c.shape, f.dt)
    run(f, 1, c=c1)
    run(f, 2, c=c2)
    assert torch.equal(f.got(c1), f.got(c2))


def test_rows_do_not_depend_on_the_row_count():
    p = Problem(65537, 256, 128, 0, torch.bfloat16, True, True, 0)
    d = run(p, 0, dma=1)
    assert _route(d, p.dt, 1) == 4
    p.check_guards()
    p.check_exact()
    c = _sent_fill(300 + GUARD, p.ldc, p.dt)
    d300 = run(p, 0, dma=1, M=300, c=c)
    assert _route(d300, p.dt, 1) == 2
    assert torch.equal(c[:300, :p.N].cpu(), p.c[:300, :p.N].cpu())
    p.check_guards(c, 300)


# ---- batched launches (the perceptor's Gram head)
@pytest.mark.parametrize("kernel,dt,K", [(1, torch.bfloat16, 96), (2, torch.bfloat16, 128), (1, torch.float32, 48),
                                         (2, torch.float32, 64)])
def test_batched_launch_equals_single_launches(kernel, dt, K):
    B, M, N = 3, 200, 160
    lda, ldc = K + 8, N + 8
    a_bs, w_bs, c_bs = (M + 5) * lda, N * K + 64, (M + 3) * ldc    # non-contiguous products, gaps between them
    g = torch.Generator().manual_seed(kernel * 10 + K)
    A = torch.randint(-8, 9, (B, M, K), generator=g).double()
    Wt = torch.randint(-8, 9, (B, N, K), generator=g).double()
    a = torch.full((B * a_bs + GUARD * lda,), float("nan"), dtype=dt, device=DEV)
    w = torch.full((B * w_bs,), float("nan"), dtype=dt, device=DEV)
    for b in range(B):
        a[b * a_bs:b * a_bs + M * lda].view(M, lda)[:, :K] = A[b].to(dt).to(DEV)
        w[b * w_bs:b * w_bs + N * K] = Wt[b].reshape(-1).to(dt).to(DEV)
    cb = _sent_fill(1, B * c_bs + GUARD * ldc, dt).view(-1)
    d = L.GemmDesc(a0=a.data_ptr(), lda0=lda, K0=K, w=w.data_ptr(), c=cb.data_ptr(), ldc=ldc, M=M, N=N, batch=B,
                   a_bstride=a_bs, w_bstride=w_bs, c_bstride=c_bs)
    L.check(_launch(d, dt, 0, kernel))
    cs = _sent_fill(1, B * c_bs + GUARD * ldc, dt).view(-1)
    esize = a.element_size()
    for b in range(B):
        d1 = L.GemmDesc(a0=a.data_ptr() + b * a_bs * esize, lda0=lda, K0=K, w=w.data_ptr() + b * w_bs * esize,
                        c=cs.data_ptr() + b * c_bs * esize, ldc=ldc, M=M, N=N)
        L.check(_launch(d1, dt, 0, kernel))
    _sync()
    assert torch.equal(_bits(cb).cpu(), _bits(cs).cpu()), "batched and single launches differ (values or untouched gaps)"
    for b in range(B):
        got = cb[b * c_bs:b * c_bs + M * ldc].view(M, ldc)[:, :N].cpu()
        assert torch.equal(got, (A[b] @ Wt[b].T).to(dt)), f"product {b}"
    untouched = torch.ones(B * c_bs + GUARD * ldc, dtype=torch.bool)
    for b in range(B):
        untouched[b * c_bs:b * c_bs + M * ldc].view(M, ldc)[:, :N] = False
    assert (_bits(cb).cpu()[untouched] == _bits(_sent_fill(1, 1, dt)).cpu()[0, 0]).all()


# ---- the QuickGELU epilogues (kernels 3 and 4)
def _qgelu(x):
    return x / (1 + torch.exp(-1.702 * x))


def _qgelu_grad(x):
    s = 1 / (1 + torch.exp(-1.702 * x))
    return s * (1 + 1.702 * x * (1 - s))


def _ulp_bf16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.pow(2.0, e - 7)


@pytest.mark.parametrize("kernel,M,N", [(3, 257, 384), (3, 2853, 1152), (4, 257, 256), (4, 2853, 1024)])
@pytest.mark.parametrize("res", [False, True])
def test_quick_gelu_epilogues(kernel, M, N, res):
    p = Problem(M, N, 128, 0, torch.bfloat16, True, res, 8)
    ld2 = N + 8
    c2 = _sent_fill(M + GUARD, ld2, p.dt)
    run(p, kernel, epi=1, c2=c2.data_ptr(), ldc2=ld2)
    p.check_guards()
    p.check_exact()
    assert torch.equal(_bits(c2[M:]).cpu(), _bits(_sent_fill(GUARD, ld2, p.dt)).cpu()), "c2 store past M"
    assert torch.equal(_bits(c2[:M, N:]).cpu(), _bits(_sent_fill(M, ld2 - N, p.dt)).cpu()), "c2 store past N"
    # (plus |c| 2^-126: for c below about -51 the f32 sigmoid leaves f32's normal range, and x * sigmoid(1.702 x) ~ 1e-37 there
    # is whatever the f32 evaluation gives - in the element-wise kernel exactly as here)
    cd = p.got().double()
    ref = _qgelu(cd)
    err = (c2[:M, :N].cpu().double() - ref).abs()
    assert (err <= _ulp_bf16(ref) + cd.abs() * 2.0 ** -126).all(), f"QuickGELU off by {(err / _ulp_bf16(ref)).max().item()} ulp"

    g = torch.Generator().manual_seed(M + N)
    h = (torch.randn(M, N, generator=g) * 3).to(torch.bfloat16).double()
    aux = _padded(h, ld2, p.dt)
    p.c.view(IVIEW[p.dt]).fill_(SENT[p.dt])
    run(p, kernel, epi=2, aux=aux.data_ptr(), ldaux=ld2)
    p.check_guards()
    # (plus the f32 evaluation error of QuickGELU' where s + 1.702 h s (1 - s) nearly cancels)
    cw = p.want().double()
    ref = cw * _qgelu_grad(h)
    err = (p.got().double() - ref).abs()
    assert (err <= _ulp_bf16(ref) + cw.abs() * 2.0 ** -20).all(), \
        f"c * QuickGELU' off by {(err / _ulp_bf16(ref)).max().item()} ulp"


# ---- the public entry point on the DMA kernels (ctx option "linear_dma")
@pytest.mark.parametrize("M,N,K,kernel", [(16385, 1024, 128, 4), (7169, 1152, 64, 3)])
def test_linear_nt_with_linear_dma(M, N, K, kernel):
    p = Problem(M, N, K, 0, torch.bfloat16, True, True, 0)
    assert _route(p.desc(), p.dt, 1) == kernel
    ctx = L.ctx()
    L.check(L.lib().maua_ctx_set_option(ctx, b"linear_dma", 1))
    try:
        L.check(L.lib().maua_linear_nt(ctx, L.ptr(p.a0), L.ptr(p.w), L.ptr(p.bd), L.ptr(p.rd), L.ptr(p.c), C.c_long(M), N, K,
                                       L.BF16))
        _sync()
    finally:
        L.check(L.lib().maua_ctx_set_option(ctx, b"linear_dma", 0))
    p.check_guards()
    p.check_exact()


# ---- byte offsets past 2^31 (about 4 GiB of A, built on the device)
def _big_a_rows(rows, K):
    r = torch.as_tensor(rows, dtype=torch.int64)[:, None]
    k = torch.arange(K, dtype=torch.int64)[None]
    return (((r * 7 + k * 13) % 17) - 8).double()


def test_large_offsets_dma_and_fallback():
    K, N, MB = 1024, 128, 2 ** 21
    g = torch.Generator().manual_seed(5)
    Wt = torch.randint(-8, 9, (N, K), generator=g).double()
    b = torch.randint(-64, 65, (N,), generator=g).double()
    a = torch.empty((MB, K), dtype=torch.bfloat16, device=DEV)
    kk = torch.arange(K, dtype=torch.int32, device=DEV)[None]
    CH = 2 ** 17
    for r0 in range(0, MB, CH):
        rr = torch.arange(r0, r0 + CH, dtype=torch.int32, device=DEV)[:, None]
        a[r0:r0 + CH] = (((rr * 7 + kk * 13) % 17) - 8).to(torch.bfloat16)
    del rr, kk
    w, bd = Wt.to(torch.bfloat16).to(DEV), b.float().to(DEV)
    c = _sent_fill(MB, N, torch.bfloat16)
    try:
        for M, kernel in ((MB - 1, 3), (MB, 2)):
            c.view(torch.int16).fill_(SENT[torch.bfloat16])
            d = L.GemmDesc(a0=a.data_ptr(), lda0=K, K0=K, w=w.data_ptr(), bias=bd.data_ptr(), c=c.data_ptr(), ldc=N, M=M, N=N)
            assert _route(d, torch.bfloat16, 1) == kernel
            L.check(_launch(d, torch.bfloat16, 1, 0))
            _sync()
            for lo, hi in ((0, 300), (2 ** 20 - 150, 2 ** 20 + 150), (M - 300, M)):
                rows = np.arange(lo, hi)
                want = (_big_a_rows(rows, K) @ Wt.T + b).to(torch.bfloat16)
                assert torch.equal(c[lo:hi].cpu(), want), (M, lo)
            if M < MB:
                assert (c[M:].view(torch.int16).cpu() == SENT[torch.bfloat16]).all()
    finally:
        del a, c
        torch.cuda.empty_cache()
