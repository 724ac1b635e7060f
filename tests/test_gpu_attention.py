"""The fused attention kernels (csrc/attention.hip: forward and its causal variant; csrc/attention_vjp.hip: attn_delta_kernel and
attention_vjp_kernel modes 0 / 1), launched through maua_attention_ex / maua_attention_vjp_ex (csrc/attention_api.hip) with row strides,
scale, the causal flag and the gradient's `out` / `lse` operands chosen here, against float64 references - the method of
tests/test_gpu_gemm.py and tests/test_gpu_modconv.py: a family whose expected result is exact and compared with torch.equal, guard
regions around every buffer (NaN around inputs and in the padding of their rows, a sentinel pattern around outputs and in the padding
of theirs), and a Gaussian family inside a derived element-wise bound.

Exact family.  Scores are integers times a power-of-two scale (0.125), so `s * scale` is exact with or without FMA contraction.  Every
key a query does not select scores at least 128 below the ones it selects: its weight is exactly 0 in float32 (expf and __expf), the
selected weights are exactly 1, the row sum is the group size 2^m, the output the exact mean of 2^m rows of V = 8 * integers in
[-15, 15] (representable in bf16), lse = m + log(2^m).  Variants (each (sample, head) has its own keys, permutation, V and choices):
    scatter   random +-1 code vectors, one per group of 1 / 2 / 4 / 8 keys scattered by a permutation over the 32-key blocks, the
              128-query tiles and the ragged tail; other keys are zero rows; query i = c_i * code of its group, c_i in {1024, 2048,
              4096} (causal: a group that lies wholly at keys <= i)
    single    the same with singleton groups only: lse = the maximum, compared exactly
    asc/desc  every query c_i * ones, key j an integer row whose sum rises (falls) by one per key: the running maximum jumps by >= 128
              at every key, alpha = exp(-big) = 0 wipes the partial sums at every block (asc), or every later block adds exact zeros
              (desc); the top 2^m keys share the best sum.  Causal asc: every key above the diagonal scores higher than all the
              keys below it, query i returns V row i, and one leaked key returns row i + 1
Before torch.equal is trusted the CPU side asserts: the float64 result is representable in the storage type; the smallest gap between
a row's best and next score times scale is >= 128; all partial sums of the integer products stay below 2^24; a float32 emulation of the
kernel's 32-key block walk (running maximum, alpha, l, o) equals the float64 result bit for bit.
Gradient: one-hot P (singleton groups / asc), integer d_out, out and lse from the exact forward: dV[j] is the integer sum of the d_out
rows of the queries that chose key j (d_out rows come in +- pairs per key, so several hundred queries on one key still sum to a
bf16 value), dS, dQ and dK are exactly zero, delta an integer dot product.  The asc variant puts every score - hence lse - below -88:
exp(-lse) overflows, which is what the kernels' zeroing of rows past T has to keep out of the sums.

Gaussian family.  Operands rounded to the storage type, float64 reference on the rounded operands, scale 1 / sqrt(D); unit Gaussians,
Gaussians x 4 (peaked; the maximum jumps between blocks), keys sorted so the scores rise / fall with the key index.  Rounding points,
as read from the kernels (T = rounding to the storage type, u its unit: 2^-8 bf16, 2^-24 f32):
    forward, bf16   scores: exact products, f32 sums over D, one rounding by `* scale`; P = __expf(s - m) in f32, summed into l in
                    f32, then rounded to bf16 for PV (n = 1); o and l rescaled by alpha = __expf(m_old - m_new) once per block; f32 sums
                    over T; one division, T() at the store
    forward, f32    the same with exact products, expf, P not rounded (n = 0)
    lse             m + logf(l) in f32
    gradient        delta = f32 dot of d_out and the ROUNDED out it is given; P = exp(s * scale - lse) from the f32 lse it is given
                    (the compiler contracts this into one fma - see below); dS = P (dP - delta) scale; bf16: P and dS rounded to
                    bf16 (n = 1); f32 sums over T; T() at the store
Bounds, element-wise, A = sum_j P_ij |V_jc| (P the float64 softmax):
    E_i      = (D + 2) 2^-24 scale max_j sum_d |q_id k_jd|  +  8 dev  +  blocks 2^-23        relative error of a weight
    out      : u |ref| + (n u + 3 T 2^-24 + 2 E_i) A                  (3 T: the PV sum, the l sum, the rescales and the division)
    lse      : 2 E_i + (T + 4) 2^-24 + 2^-22 (|lse| + |lse - m|)
    eP       = max_i ((D + 2) 2^-24 scale max_j sum_d |q k| + bound(lse)_i + 4 dev)            the rebuilt weight
    delta    : sum_c |dO_ic| err(out)_ic + (D + 2) 2^-24 sum_c |dO_ic out_ic|,  err(out) = the forward bound (own forward) or u |out|
    errS_ij  = P_ij ((eP + n u + 4 2^-24) (|dP_ij| + |delta_i|) + (D + 2) 2^-24 sum_c |dO_ic V_jc| + bound(delta)_i)
    dQ       : u |ref| + scale (sum_j errS_ij |K_jd| + T 2^-24 sum_j |dS_ij| |K_jd|),  dK the same over i with Q
    dV       : u |ref| + (eP + n u + T 2^-24) sum_i P_ij |dO_ic|
dev is the one term not derived from the code: the error of the exponential itself.  It is measured on the reference - the largest
relative deviation of float32 exp on the CPU from float64 exp over the case's own arguments s - max >= -80 - and allowed 4 x (8 x
where the rescales repeat it): __expf is v_exp_f32(x log2 e), one more rounding of an argument of the same size than the CPU's, plus
the instruction's own ulp.  No other margin is applied.

Finding (FMA contraction).  The gfx950 object of attention_vjp.hip computes the rebuilt weight's argument as v_fma_f32(s, scale, -lse)
- one rounding - where the forward rounds s * scale first (v_mul_f32) and subtracts the maximum after.  The rebuilt P so differs from
the forward's by up to |s scale| 2^-24 relative, which E_i already counts ((D + 2) 2^-24 sum |q k| >= |s|); the Gaussian x 4 set stays
inside the bound with it, so the kernels are left alone."""
import ctypes as C
import math

import pytest
import torch

from maua_amd import _lib as L

pytestmark = pytest.mark.gpu

DEV = "cuda"
TDT = {"f32": torch.float32, "bf16": torch.bfloat16}
DTID = {"f32": L.F32, "bf16": L.BF16}
U = {"bf16": 2.0 ** -8, "f32": 2.0 ** -24}
SENT16, SENT32 = 0x5A5A, 0x5A5A5A5A
G = 4096                                            # guard elements on either side of every buffer
EXACT_SCALE = 0.125
T_LIST = (1, 31, 32, 33, 50, 77, 127, 128, 129, 197, 257, 300, 1024)
D_DT = ((32, "f32"), (64, "bf16"), (32, "bf16"), (64, "f32"))
B_HEADS = ((1, 1), (2, 3), (3, 12))
WORST = {}                                          # family -> worst error / bound seen (test_zz_report prints it)


def shape(iT, k, extra=0):
    """the thinned shape matrix: every T meets every (D, dtype), and the (B, heads) and stride choices rotate under them"""
    T, (D, dt) = T_LIST[iT], D_DT[k]
    r = iT + k + extra
    bh = B_HEADS[r % 3]
    if T >= 300 and bh == (3, 12):
        bh = B_HEADS[r % 2]
    return T, D, dt, bh[0], bh[1], (r // 3 + k) % 2


def _sync():
    torch.cuda.synchronize()


class Buf:
    """rows of `width` elements `ld` apart between guard regions.  Inputs (data given): NaN in the guards and in the rows' padding.
    Outputs: a sentinel bit pattern everywhere; check() wants guards and padding intact and every element of the body written."""

    def __init__(self, rows, width, ld=None, dtype=torch.float32, data=None):
        ld = width if ld is None else ld
        self.rows, self.width, self.ld, self.out = rows, width, ld, data is None
        self.full = torch.empty((2 * G + rows * ld,), dtype=dtype, device=DEV)
        if data is None:
            self._bits().fill_(SENT16 if self.full.element_size() == 2 else SENT32)
        else:
            body = torch.full((rows, ld), float("nan"), dtype=dtype)
            body[:, :width] = data.reshape(rows, width).to(dtype)
            self.full.fill_(float("nan"))
            self.full[G:G + rows * ld] = body.reshape(-1).to(DEV)
        self.ptr = self.full.data_ptr() + G * self.full.element_size()

    def _bits(self):
        return self.full.view(torch.int16 if self.full.element_size() == 2 else torch.int32)

    def get(self):
        return self.full[G:G + self.rows * self.ld].reshape(self.rows, self.ld)[:, :self.width].cpu()

    def check(self, what):
        s = SENT16 if self.full.element_size() == 2 else SENT32
        b = self._bits().cpu()
        assert (b[:G] == s).all() and (b[G + self.rows * self.ld:] == s).all(), f"{what}: a store outside the buffer"
        body = b[G:G + self.rows * self.ld].reshape(self.rows, self.ld)
        assert (body[:, self.width:] == s).all(), f"{what}: a store into the padding between the rows"
        assert (body[:, :self.width] != s).all(), f"{what}: elements of the result were never written"
        assert not torch.isnan(self.get().float()).any(), f"{what}: NaN in the result (a guard or a row's padding was read)"

    def untouched(self):
        s = SENT16 if self.full.element_size() == 2 else SENT32
        return bool((self._bits() == s).all())


class Case:
    """q, k, v: float64 [B][heads][T][D], representable in the storage type; the device tensor in the kernels' layout"""

    def __init__(self, q, k, v, dt, pad, scale, causal=0):
        self.q, self.k, self.v, self.dt, self.tdt, self.scale, self.causal = q, k, v, dt, TDT[dt], scale, causal
        self.B, self.h, self.T, self.D = q.shape
        for t in (q, k, v):
            assert torch.equal(t.to(self.tdt).double(), t), "operands must be representable in the storage type"
        self.ld_qkv = 3 * self.h * self.D + (16 if pad else 0)
        self.ld_out = self.h * self.D + (8 if pad else 0)
        qkv = torch.stack((q, k, v), 2).permute(0, 3, 1, 2, 4)                      # [B][T][heads][3][D]
        self.qkv = Buf(self.B * self.T, 3 * self.h * self.D, self.ld_qkv, self.tdt, data=qkv)

    def rows(self, t):
        """[B][heads][T][D] -> the kernels' [B T][heads D]"""
        return t.permute(0, 2, 1, 3).reshape(self.B * self.T, self.h * self.D)

    def heads_first(self, rows):
        return rows.reshape(self.B, self.T, self.h, self.D).permute(0, 2, 1, 3)

    def forward(self, lse=True):
        out = Buf(self.B * self.T, self.h * self.D, self.ld_out, self.tdt)
        ls = Buf(self.B * self.h, self.T) if lse else None
        d = L.AttnDesc(qkv=self.qkv.ptr, out=out.ptr, lse=ls.ptr if lse else None, B=self.B, T=self.T, heads=self.h, head_ch=self.D,
                       ld_qkv=self.ld_qkv, ld_out=self.ld_out, scale=self.scale, causal=self.causal, dtype=DTID[self.dt])
        L.check(L.lib().maua_attention_check(C.byref(d)))
        L.check(L.lib().maua_attention_ex(L.ctx(), C.byref(d)))
        _sync()
        out.check("out")
        if lse:
            ls.check("lse")
        return self.heads_first(out.get()), ls.get().reshape(self.B, self.h, self.T) if lse else None

    def gradient(self, out, lse, d_out):
        """out, d_out: [B][heads][T][D] (any float type, representable in the storage type); lse float32 [B][heads][T]"""
        ob = Buf(self.B * self.T, self.h * self.D, self.ld_out, self.tdt, data=self.rows(out))
        gb = Buf(self.B * self.T, self.h * self.D, self.ld_out, self.tdt, data=self.rows(d_out))
        lb = Buf(self.B * self.h, self.T, data=lse.float())
        dq = Buf(self.B * self.T, 3 * self.h * self.D, self.ld_qkv, self.tdt)
        de = Buf(self.B * self.h, self.T)
        d = L.AttnVjpDesc(qkv=self.qkv.ptr, out=ob.ptr, d_out=gb.ptr, lse=lb.ptr, d_qkv=dq.ptr, delta=de.ptr, B=self.B, T=self.T,
                          heads=self.h, head_ch=self.D, ld_qkv=self.ld_qkv, ld_out=self.ld_out, scale=self.scale, causal=0,
                          dtype=DTID[self.dt])
        L.check(L.lib().maua_attention_vjp_check(C.byref(d)))
        L.check(L.lib().maua_attention_vjp_ex(L.ctx(), C.byref(d)))
        _sync()
        dq.check("d_qkv")
        de.check("delta")
        g = dq.get().reshape(self.B, self.T, self.h, 3, self.D).permute(3, 0, 2, 1, 4)
        return g[0], g[1], g[2], de.get().reshape(self.B, self.h, self.T)

    # ---- float64 references
    def scores(self):
        s = self.q @ self.k.transpose(-1, -2) * self.scale
        if self.causal:
            s = s.masked_fill(torch.ones(self.T, self.T, dtype=torch.bool).triu(1), float("-inf"))
        return s

    def ref_forward(self):
        s = self.scores()
        m = s.max(-1, keepdim=True).values      # (s - m is exact for the exact family's scores, and exp(0) = 1: no rounding before l)
        p = torch.exp(s - m)
        l = p.sum(-1, keepdim=True)
        p = p / l
        return p @ self.v, (m + torch.log(l))[..., 0], p, s

    def ref_gradient(self, d_out):
        o, lse, p, s = self.ref_forward()
        dp = d_out @ self.v.transpose(-1, -2)
        delta = (d_out * o).sum(-1)
        ds = p * (dp - delta[..., None])
        return {"dq": ds @ self.k * self.scale, "dk": ds.transpose(-1, -2) @ self.q * self.scale, "dv": p.transpose(-1, -2) @ d_out,
                "delta": delta, "o": o, "lse": lse, "p": p, "s": s, "dp": dp, "ds": ds}

    def emulate_f32(self):
        """the kernel's walk over 32-key blocks in float32: running maximum, alpha, l and o, as attention.hip orders them"""
        q, k, v = self.q.float(), self.k.float(), self.v.float()
        B, h, T, D = q.shape
        m = torch.full((B, h, T), -1.0e30)
        l = torch.zeros(B, h, T)
        o = torch.zeros(B, h, T, D)
        qi = torch.arange(T)[:, None]
        for kb in range(0, T, 32):
            kk = torch.arange(kb, min(kb + 32, T))
            s = (q @ k[:, :, kk].transpose(-1, -2)) * torch.tensor(self.scale, dtype=torch.float32)
            if self.causal:
                s = s.masked_fill(kk[None, :] > qi, float("-inf"))
            m_new = torch.maximum(m, s.max(-1).values)
            alpha = torch.exp(m - m_new)
            p = torch.exp(s - m_new[..., None])
            l = l * alpha + p.sum(-1)
            o = o * alpha[..., None] + p @ v[:, :, kk]
            m = m_new
        return o * (1.0 / l)[..., None], m + torch.log(l), m


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 1000003 * int(x) for i, x in enumerate(key)) % (2 ** 31))


def exact_case(variant, B, h, T, D, dt, pad, causal, seed, hot=False, negative=False):
    """the exact family's operands; returns the case and, per (sample, head), the key every query selects first (its group's lowest)"""
    g = _gen(seed, B, h, T, D, causal, len(variant))
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).double()
    q, k = torch.zeros(B, h, T, D, dtype=torch.float64), torch.zeros(B, h, T, D, dtype=torch.float64)
    v = 8.0 * ri(-15, 15, B, h, T, D)
    for b in range(B):
        for hh in range(h):
            c = 1024.0 * 2.0 ** torch.randint(0, 3 if variant in ("scatter", "single") else 2, (T,), generator=g).double()
            if variant in ("scatter", "single"):
                perm = torch.randperm(T, generator=g)
                if causal or T == 1:      # key 0 is a singleton group, so every query has a group it sees whole
                    perm = torch.cat((torch.tensor([0]), perm[perm != 0]))
                sizes, used = [], 0
                while used < max(1, (3 * T) // 4):
                    sz = 1 if variant == "single" or not sizes else (1, 2, 4, 8)[len(sizes) % 4]
                    if used + sz > T:
                        break
                    sizes.append(sz)
                    used += sz
                codes = ri(0, 1, len(sizes), D) * 2.0 - 1.0
                while len(torch.unique(codes, dim=0)) < len(sizes):
                    codes = ri(0, 1, len(sizes), D) * 2.0 - 1.0
                last, first, off = [], [], 0
                for gi, sz in enumerate(sizes):
                    mem = perm[off:off + sz]
                    k[b, hh, mem] = codes[gi]
                    last.append(int(mem.max()))
                    first.append(int(mem.min()))
                    off += sz
                last = torch.tensor(last)
                if hot:                   # half of the queries on one key, half of the keys chosen by nobody
                    pool = torch.arange(0, len(sizes), 2)
                    choice = pool[torch.randint(0, len(pool), (T,), generator=g)]
                    choice[torch.randperm(T, generator=g)[:T // 2]] = 0
                elif causal:              # among the groups wholly at keys <= i
                    choice = torch.stack([torch.nonzero(last <= i)[:, 0][torch.randint(0, int((last <= i).sum()), (1,), generator=g)][0]
                                          for i in range(T)])
                else:
                    choice = torch.randint(0, len(sizes), (T,), generator=g)
                q[b, hh] = c[:, None] * codes[choice]
            else:                         # asc / desc: integer rows whose sums rise / fall by one per key
                m = 0 if causal or hot else (b + hh) % 4
                fill = (T - 1) % 32 + 1 if variant == "asc" else min(T, 32)
                while (1 << m) > fill:
                    m -= 1
                j = torch.arange(T) if variant == "asc" else torch.arange(T - 1, -1, -1)
                sums = torch.minimum(j, torch.tensor(T - (1 << m))) - (T + 200 if negative else (0, T // 2, T + 200)[(b + 2 * hh) % 3])
                base = torch.div(sums, D, rounding_mode="floor")
                rows = base[:, None].repeat(1, D).double()
                rows += (torch.arange(D)[None, :] < (sums - base * D)[:, None]).double()
                noise = ri(-4, 4, T, D)
                k[b, hh] = rows + noise - noise.roll(1, -1)
                assert torch.equal(k[b, hh].sum(-1), sums.double())
                q[b, hh] = c[:, None] * torch.ones(D, dtype=torch.float64)
    return Case(q, k, v, dt, pad, EXACT_SCALE, causal)


def check_exact(cs):
    """the conditions under which torch.equal may be trusted, asserted on the CPU; returns the float64 reference"""
    o, lse, p, s = cs.ref_forward()
    assert torch.equal(o.to(cs.tdt).double(), o.float().double()), "the float64 result is not representable in the storage type"
    assert float((cs.q.abs() @ cs.k.abs().transpose(-1, -2)).max()) < 2.0 ** 24, "partial sums of the scores may be inexact"
    best = s.max(-1, keepdim=True).values
    below = torch.where(s < best, s, torch.full_like(s, float("-inf"))).max(-1).values
    assert float((best[..., 0] - below).min()) >= 128.0, "a key that is not selected scores less than 128 below the selected ones"
    cnt = (s == best).sum(-1)
    assert bool(((cnt & (cnt - 1)) == 0).all()), "a selected group is not a power of two"
    eo, el, em = cs.emulate_f32()
    assert torch.equal(eo.double(), o.float().double()), "the float32 block-walk emulation differs from the float64 softmax"
    return o, lse, cnt, em.double(), el.double()


def _ulps(got, ref):
    """|got - ref| in units of float32's spacing at ref"""
    ulp = 2.0 ** (torch.floor(torch.log2(ref.abs().clamp(min=2.0 ** -126))) - 23)
    return ((got.double() - ref).abs() / ulp).max().item()


FWD_EXACT = [(iT, k, ("scatter", "single", "asc", "desc")[(iT + k + causal) % 4], causal)
             for iT in range(len(T_LIST)) for k in range(4) for causal in (0, 1)]


@pytest.mark.parametrize("iT,k,variant,causal", FWD_EXACT, ids=[f"T{T_LIST[i]}-D{D_DT[k][0]}-{D_DT[k][1]}-{v}{'-causal' if c else ''}"
                                                              for i, k, v, c in FWD_EXACT])
def test_forward_exact(iT, k, variant, causal):
    T, D, dt, B, h, pad = shape(iT, k, causal)
    cs = exact_case(variant, B, h, T, D, dt, pad, causal, seed=1)
    o, lse, cnt, m, _ = check_exact(cs)
    if variant == "scatter" and T >= 64 and not causal:   # the same maximum in several blocks: alpha is exactly 1 there
        s = cs.scores()
        blocks = ((s == s.max(-1, keepdim=True).values).reshape(B, h, T, -1)[..., :T // 32 * 32].reshape(B, h, T, T // 32, 32).any(-1)).sum(-1)
        assert int(blocks.max()) >= 2, "no selected group straddles two key blocks"
    if causal and variant == "asc" and T > 1:             # every key above the diagonal would win: a leak returns a different integer row
        free = Case(cs.q, cs.k, cs.v, dt, pad, EXACT_SCALE, 0).ref_forward()[0]
        assert float((free != o).any(-1).float().mean()) > 0.9
    got, got_lse = cs.forward()
    assert torch.equal(got.double(), o.to(cs.tdt).double()), f"out differs: {int((got.double() != o).any(-1).sum())} rows"
    if causal:
        assert torch.equal(got[:, :, 0].double(), cs.v[:, :, 0]), "query 0 must return V row 0"
    single = cnt == 1
    assert torch.equal(got_lse[single], lse.float()[single]) and torch.equal(lse.float()[single].double(), m[single]), "lse of one-hot rows"
    assert _ulps(got_lse, m + torch.log(cnt.double())) <= 2.0, "lse = m + log(2^m) within 2 ulp"
    # without lse the result is the same and nothing else is written
    again, _ = cs.forward(lse=False)
    assert torch.equal(again, got)


GRAD_EXACT = [(iT, k, ("single", "asc")[(iT + k) % 2]) for iT in range(len(T_LIST)) for k in range(4)]


def paired_d_out(sel, D, g):
    """integer rows in [-7, 7] that cancel in pairs among the queries that selected the same key: [T][D]"""
    T = sel.numel()
    order = torch.argsort(sel, stable=True)
    ss = sel[order]
    start = torch.cat((torch.tensor([True]), ss[1:] != ss[:-1]))
    run0 = torch.cummax(torch.where(start, torch.arange(T), torch.zeros(T, dtype=torch.long)), 0).values
    odd = (torch.arange(T) - run0) % 2 == 1
    rows = torch.randint(-7, 8, (T, D), generator=g).double()
    rows[odd] = -rows[torch.nonzero(odd)[:, 0] - 1]
    out = torch.empty_like(rows)
    out[order] = rows
    return out


@pytest.mark.parametrize("iT,k,variant", GRAD_EXACT, ids=[f"T{T_LIST[i]}-D{D_DT[k][0]}-{D_DT[k][1]}-{v}" for i, k, v in GRAD_EXACT])
def test_gradient_exact(iT, k, variant):
    T, D, dt, B, h, pad = shape(iT, k, 1)
    cs = exact_case(variant, B, h, T, D, dt, pad, 0, seed=2, hot=True, negative=True)
    o, lse, cnt, m, _ = check_exact(cs)
    assert bool((cnt == 1).all())
    s = cs.scores()
    sel = s.argmax(-1)
    g = _gen(3, B, h, T, D)
    d_out = torch.stack([torch.stack([paired_d_out(sel[b, hh], D, g) for hh in range(h)]) for b in range(B)])
    ref = cs.ref_gradient(d_out)
    per_key = torch.zeros(B, h, T, dtype=torch.long).scatter_add_(2, sel, torch.ones_like(sel))
    if T >= 128:
        assert int(per_key.max()) >= T // 2 and float((per_key == 0).float().mean()) >= 0.25
    if variant == "asc":
        assert float(lse.max()) < -88.0                    # exp(-lse) overflows float32
    assert float((ref["p"].transpose(-1, -2) @ d_out.abs()).max()) < 2.0 ** 24 and float((d_out.abs() * o.abs()).sum(-1).max()) < 2.0 ** 24
    for name in ("dq", "dk", "dv"):
        assert torch.equal(ref[name].to(cs.tdt).double(), ref[name].float().double()), f"{name} is not representable"
    assert not ref["dq"].float().any() and not ref["dk"].float().any()
    out, got_lse = cs.forward()
    assert torch.equal(out.double(), o.float().double()) and torch.equal(got_lse, lse.float())
    dq, dk, dv, delta = cs.gradient(out, got_lse, d_out)
    assert torch.equal(delta.double(), ref["delta"].float().double()), "delta"
    assert torch.equal(dv.double(), ref["dv"].float().double()), f"dV differs in {int((dv.double() != ref['dv']).any(-1).sum())} rows"
    assert torch.equal(dq.double(), torch.zeros_like(ref["dq"])), "dQ must be exactly zero"
    assert torch.equal(dk.double(), torch.zeros_like(ref["dk"])), "dK must be exactly zero"


# ---- Gaussian family
SETS = ("unit", "x4", "rise", "fall")


def gaussian_case(kind, B, h, T, D, dt, pad, causal, seed):
    g = _gen(seed, B, h, T, D, causal, SETS.index(kind))
    rn = lambda *s: torch.randn(*s, generator=g).double()
    amp = 4.0 if kind == "x4" else 1.0
    q, k, v = amp * rn(B, h, T, D), amp * rn(B, h, T, D), amp * rn(B, h, T, D)
    if kind in ("rise", "fall"):          # keys ordered along a direction every query leans to
        w = rn(B, h, 1, D)
        order = torch.argsort((k * w).sum(-1), -1, descending=kind == "fall")
        k = torch.gather(k, 2, order[..., None].expand(-1, -1, -1, D))
        q = q + 1.5 * w
    tdt = TDT[dt]
    rt = lambda t: t.to(tdt).double()
    cs = Case(rt(q), rt(k), rt(v), dt, pad, 1.0 / math.sqrt(D), causal)
    return cs, rt(amp * rn(B, h, T, D))


def forward_bounds(cs):
    o, lse, p, s = cs.ref_forward()
    m = s.max(-1).values
    x = s - m[..., None]
    x = torch.where(x >= -80.0, x, torch.zeros_like(x))
    dev = float((torch.exp(x.float()).double() / torch.exp(x) - 1.0).abs().max())
    smax = (cs.q.abs() @ cs.k.abs().transpose(-1, -2)).max(-1).values * cs.scale
    blocks = (cs.T + 31) // 32
    E = (cs.D + 2) * 2.0 ** -24 * smax + 8.0 * dev + blocks * 2.0 ** -23
    n, u = (1 if cs.dt == "bf16" else 0), U[cs.dt]
    A = p @ cs.v.abs()
    b_out = u * o.abs() + (n * u + 3 * cs.T * 2.0 ** -24 + 2.0 * E)[..., None] * A
    b_lse = 2.0 * E + (cs.T + 4) * 2.0 ** -24 + 2.0 ** -22 * (lse.abs() + (lse - m).abs())
    eP = float(((cs.D + 2) * 2.0 ** -24 * smax + b_lse + 4.0 * dev).max())
    return o, lse, p, b_out, b_lse, eP


def _ratio(family, got, ref, bound):
    r = float(((got.double() - ref).abs() / bound.clamp(min=1e-300)).max())
    WORST[family] = max(WORST.get(family, 0.0), r)
    return r


GAUSS = [(iT, k, SETS[(iT + k) % 4]) for iT in range(len(T_LIST)) for k in range(4)]
GAUSS_IDS = [f"T{T_LIST[i]}-D{D_DT[k][0]}-{D_DT[k][1]}-{s}" for i, k, s in GAUSS]


@pytest.mark.parametrize("iT,k,kind", GAUSS, ids=GAUSS_IDS)
def test_forward_gaussian_within_float64_bound(iT, k, kind):
    T, D, dt, B, h, pad = shape(iT, k, 2)
    for causal in (0, 1):
        cs, _ = gaussian_case(kind, B, h, T, D, dt, pad, causal, seed=4)
        o, lse, p, b_out, b_lse, _ = forward_bounds(cs)
        got, got_lse = cs.forward()
        fam = f"forward {dt}{' causal' if causal else ''}"
        r1, r2 = _ratio(fam, got, o, b_out), _ratio(fam + " lse", got_lse, lse, b_lse)
        print(f"{fam} {kind} T={T} D={D} B={B} heads={h}: out error / bound {r1:.3f}, lse {r2:.3f}")
        assert r1 <= 1.0, f"out: error / bound {r1:.3f}"
        assert r2 <= 1.0, f"lse: error / bound {r2:.3f}"


@pytest.mark.parametrize("iT,k,kind", GAUSS, ids=GAUSS_IDS)
def test_gradient_gaussian_within_float64_bound(iT, k, kind):
    T, D, dt, B, h, pad = shape(iT, k, 3)
    cs, d_out = gaussian_case(kind, B, h, T, D, dt, pad, 0, seed=5)
    o, lse, p, b_out, b_lse, eP = forward_bounds(cs)
    ref = cs.ref_gradient(d_out)
    n, u, e24 = (1 if dt == "bf16" else 0), U[dt], 2.0 ** -24
    own_out, own_lse = cs.forward()
    r0 = _ratio(f"forward {dt}", own_out, o, b_out)
    assert r0 <= 1.0, f"the forward under the gradient: error / bound {r0:.3f}"
    ds, dp, delta = ref["ds"], ref["dp"], ref["delta"]
    for mode, out_in, lse_in, err_o in (("own forward", own_out, own_lse, b_out),
                                        ("reference forward", o.to(cs.tdt), lse.float(), u * o.abs())):
        b_delta = (d_out.abs() * err_o).sum(-1) + (D + 2) * e24 * (d_out.abs() * o.abs()).sum(-1)
        errS = p * ((eP + n * u + 4 * e24) * (dp.abs() + delta.abs()[..., None]) + (D + 2) * e24 * (d_out.abs() @ cs.v.abs().transpose(-1, -2))
                    + b_delta[..., None])
        b_dq = u * ref["dq"].abs() + cs.scale * (errS @ cs.k.abs() + T * e24 * (ds.abs() @ cs.k.abs()))
        b_dk = u * ref["dk"].abs() + cs.scale * (errS.transpose(-1, -2) @ cs.q.abs() + T * e24 * (ds.abs().transpose(-1, -2) @ cs.q.abs()))
        b_dv = u * ref["dv"].abs() + (eP + n * u + T * e24) * (p.transpose(-1, -2) @ d_out.abs())
        dq, dk, dv, got_delta = cs.gradient(out_in, lse_in, d_out)
        fam = f"gradient {dt}, {mode}"
        rs = {"dQ": _ratio(fam + " dQ", dq, ref["dq"], b_dq), "dK": _ratio(fam + " dK", dk, ref["dk"], b_dk),
              "dV": _ratio(fam + " dV", dv, ref["dv"], b_dv), "delta": _ratio(fam + " delta", got_delta, delta, b_delta + e24 * delta.abs())}
        print(f"{fam} {kind} T={T} D={D} B={B} heads={h}: error / bound " + ", ".join(f"{a} {b:.3f}" for a, b in rs.items()))
        for name, r in rs.items():
            assert r <= 1.0, f"{name} ({mode}): error / bound {r:.3f}"


def test_refusals_launch_nothing():
    """what the checks refuse (tests/test_attention_host.py pins the texts) is refused by the launching entry points too, and B == 0
    returns at once: the sentinel-filled results stay untouched"""
    cs = exact_case("single", 1, 1, 33, 32, "bf16", 1, 0, seed=6)
    out, lse = Buf(33, 32, cs.ld_out, cs.tdt), Buf(1, 33)
    mk = lambda **kw: L.AttnDesc(**{**dict(qkv=cs.qkv.ptr, out=out.ptr, lse=lse.ptr, B=1, T=33, heads=1, head_ch=32, ld_qkv=cs.ld_qkv,
                                           ld_out=cs.ld_out, scale=0.125, causal=0, dtype=L.BF16), **kw})
    for kw, text in ((dict(qkv=cs.qkv.ptr + 2), "attention: qkv / out must be 16-byte aligned"),
                     (dict(out=out.ptr + 8), "attention: qkv / out must be 16-byte aligned"),
                     (dict(ld_out=cs.ld_out + 4), "attention: row strides must be whole 16-byte pieces"),
                     (dict(ld_qkv=64), "attention: row strides below the heads' channels"),
                     (dict(head_ch=48), "attention: head channels must be 32 or 64"),
                     (dict(T=0), "attention: bad shape"), (dict(dtype=L.F16), "attention: unsupported dtype")):
        assert L.lib().maua_attention_ex(L.ctx(), C.byref(mk(**kw))) == -1 and L.lib().maua_last_error().decode() == text
    assert L.lib().maua_attention_ex(L.ctx(), C.byref(mk(B=0))) == 0
    _sync()
    assert out.untouched() and lse.untouched()
    dq, de = Buf(33, 96, cs.ld_qkv, cs.tdt), Buf(1, 33)
    ob, gb, lb = Buf(33, 32, cs.ld_out, cs.tdt, data=torch.zeros(33, 32)), Buf(33, 32, cs.ld_out, cs.tdt, data=torch.zeros(33, 32)), Buf(1, 33, data=torch.zeros(33))
    mv = lambda **kw: L.AttnVjpDesc(**{**dict(qkv=cs.qkv.ptr, out=ob.ptr, d_out=gb.ptr, lse=lb.ptr, d_qkv=dq.ptr, delta=de.ptr, B=1, T=33,
                                              heads=1, head_ch=32, ld_qkv=cs.ld_qkv, ld_out=cs.ld_out, scale=0.125, causal=0, dtype=L.BF16), **kw})
    for kw, text in ((dict(causal=1), "attention_vjp: no gradient of the causal forward"),
                     (dict(d_qkv=dq.ptr + 4), "attention_vjp: qkv / out / d_out / d_qkv must be 16-byte aligned"),
                     (dict(delta=None), "attention_vjp: NULL argument"),
                     (dict(ld_qkv=cs.ld_qkv + 1), "attention_vjp: row strides must be whole 16-byte pieces")):
        assert L.lib().maua_attention_vjp_ex(L.ctx(), C.byref(mv(**kw))) == -1 and L.lib().maua_last_error().decode() == text
    assert L.lib().maua_attention_vjp_ex(L.ctx(), C.byref(mv(B=0))) == 0
    _sync()
    assert dq.untouched() and de.untouched()


def test_matrix_reaches_every_instantiation_and_shape():
    """the thinned matrix, statically: every kernel instantiation (D, dtype, causal; the gradient's three kernels per D and dtype), and under
    every family every T with both head sizes, both types, all three (B, heads) and both stride forms somewhere in the file"""
    fwd = {(shape(i, k, c)[1], shape(i, k, c)[2], c) for i, k, _, c in FWD_EXACT} | {(D_DT[k][0], D_DT[k][1], c) for _, k, _ in GAUSS for c in (0, 1)}
    assert fwd == {(D, dt, c) for D in (32, 64) for dt in ("f32", "bf16") for c in (0, 1)}
    assert {D_DT[k] for _, k, _ in GRAD_EXACT} == {D_DT[k] for _, k, _ in GAUSS} == set(D_DT)
    for cases, extra in (([(i, k, c) for i, k, _, c in FWD_EXACT], None), ([(i, k, 1) for i, k, _ in GRAD_EXACT], 1),
                         ([(i, k, 2) for i, k, _ in GAUSS], 2), ([(i, k, 3) for i, k, _ in GAUSS], 3)):
        shapes = [shape(*c) for c in cases]
        assert {s_[0] for s_ in shapes} == set(T_LIST)
        for T in T_LIST:
            assert {(s_[1], s_[2]) for s_ in shapes if s_[0] == T} == set(D_DT)
        assert {(s_[3], s_[4]) for s_ in shapes} == set(B_HEADS) and {s_[5] for s_ in shapes} == {0, 1}
    every = [shape(i, k, c) for i, k, _, c in FWD_EXACT] + [shape(i, k, e) for i, k, _ in GAUSS for e in (2, 3)] + [shape(i, k, 1) for i, k, _ in GRAD_EXACT]
    for T in (50, 197, 257):             # the CLIP towers' token counts under 12 heads
        assert any(s_[0] == T and s_[4] == 12 for s_ in every)


def test_zz_report():
    """the worst error / bound of each Gaussian family, printed for the record (after a whole run of this file)"""
    for fam in sorted(WORST):
        print(f"worst error / bound, {fam}: {WORST[fam]:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
