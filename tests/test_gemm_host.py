"""CPU-only: which GEMM kernel launch_gemm_nt (csrc/gemm.hip) picks for a shape, and what it refuses, through the host-only
maua_gemm_nt_route.  Kernels: 1 = 64 x 128 register-staged, 2 = 128 x 128 register-staged (+ XCD remap), 3 = 256 x 128 LDS-direct,
4 = 256 x 256 LDS-direct.  Every threshold is pinned on both sides; the real callers' shape families are pinned to the kernel they
take.  Pointers are fake (the route never dereferences them)."""
import ctypes as C

import pytest

from maua_amd import _lib as L

F32, BF16 = L.F32, L.BF16
A0, A1, W, BIAS, RES, CC, C2, AUX = (0x10000 * (i + 1) for i in range(8))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from maua_amd.build import build
    build()


def desc(M, N, K0, K1=0, *, lda0=None, lda1=None, ldc=None, bias=False, res=False, ldr=None, epi=0, batch=0, **kw):
    d = L.GemmDesc(a0=A0, lda0=K0 if lda0 is None else lda0, K0=K0, a1=A1 if K1 else None, lda1=K1 if lda1 is None else lda1,
                   K1=K1, w=W, bias=BIAS if bias else None, res=RES if res else None, ldr=N if ldr is None else ldr, c=CC,
                   ldc=N if ldc is None else ldc, M=M, N=N, epi=epi, c2=C2 if epi == 1 else None, ldc2=N,
                   aux=AUX if epi == 2 else None, ldaux=N, batch=batch)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def route(d, dtype=BF16, dma=0):
    """(kernel, remap_nt), or the refusal text."""
    remap = C.c_int(-1)
    rc = L.lib().maua_gemm_nt_route(C.byref(d), dtype, dma, C.byref(remap))
    if rc < 0:
        return L.lib().maua_last_error().decode()
    return rc, remap.value


def refused(d, dtype=BF16, dma=0):
    r = route(d, dtype, dma)
    return isinstance(r, str) and r.startswith("gemm_nt")


# ---- thresholds, each on both sides
@pytest.mark.parametrize("dtype,K", [(BF16, 64), (F32, 32)])
def test_m_threshold_of_the_128_row_kernel(dtype, K):
    assert route(desc(127, 128, K), dtype) == (1, 0)
    assert route(desc(128, 128, K), dtype) == (2, 0)


def test_k_chunks_of_the_128_row_kernel():
    # bf16: K parts in whole 64-channel (128-byte) chunks go to kernel 2, parts that are only whole 32-channel chunks to kernel 1
    assert route(desc(256, 128, 128)) == (2, 0)
    assert route(desc(256, 128, 96)) == (1, 0)
    assert route(desc(256, 128, 64, 96)) == (1, 0)
    assert route(desc(256, 128, 96, 64)) == (1, 0)
    assert route(desc(256, 128, 64, 128)) == (2, 0)
    assert route(desc(256, 128, 48), F32) == (1, 0)
    assert route(desc(256, 128, 64), F32) == (2, 0)


@pytest.mark.parametrize("N,nt", [(128, 1), (256, 2), (1024, 8), (1152, 9)])
@pytest.mark.parametrize("mtiles", [63, 64])
def test_xcd_remap_thresholds(N, nt, mtiles):
    M = 128 * (mtiles - 1) + 1
    want = nt if 2 <= nt <= 8 and mtiles >= 64 else 0
    assert route(desc(M, N, 128)) == (2, want)
    assert route(desc(M, N, 128), F32) == (2, want)
    assert route(desc(M, N, 64, batch=2, a_bstride=M * 64, c_bstride=M * N)) == (2, 0)   # batched launches are never remapped


def test_dma_tile_count_threshold():
    # N = 128: one 256 x 128 tile per 256 rows -> kernel 3 from 256 tiles on
    assert route(desc(255 * 256, 128, 64), dma=1) == (2, 0)
    assert route(desc(255 * 256 + 1, 128, 64), dma=1) == (3, 0)
    # N = 256: kernel 4 needs 256 tiles of 256 x 256 as well
    assert route(desc(128 * 256, 256, 64), dma=1) == (3, 0)
    assert route(desc(255 * 256, 256, 64), dma=1) == (3, 0)
    assert route(desc(255 * 256 + 1, 256, 64), dma=1) == (4, 0)
    # M >= 256 even with enough tiles
    assert route(desc(255, 32768, 64), dma=1) == (2, 0)
    assert route(desc(256, 32768, 64), dma=1) == (3, 0)
    assert route(desc(256, 65536, 64), dma=1) == (4, 0)
    # without prefer_dma, or in f32, never
    assert route(desc(65536, 1024, 64), dma=0) == (2, 8)
    assert route(desc(65536, 1024, 64), F32, dma=1) == (2, 8)


def test_n_and_second_source_choose_between_the_dma_kernels(monkeypatch):
    assert route(desc(65536, 1024, 128), dma=1) == (4, 0)
    assert route(desc(65536, 1152, 128), dma=1) == (3, 0)            # N % 128 only
    assert route(desc(65536, 1024, 64, 64), dma=1) == (3, 0)         # K1 > 0
    assert route(desc(65536, 1024, 64, 96), dma=1) == (1, 0)         # K1 not whole 64-channel chunks: no DMA, no kernel 2
    monkeypatch.setenv("MAUA_GEMM_DMA_128", "1")
    assert route(desc(65536, 1024, 128), dma=1) == (3, 0)


def test_32_bit_byte_offset_guards():
    # M lda0 2 = 2^32 - 2 lda0 (the last row's end is below 2^32) against exactly 2^32
    assert route(desc(2**21 - 1, 128, 1024), dma=1) == (3, 0)
    assert route(desc(2**21, 128, 1024), dma=1) == (2, 0)
    assert route(desc(2**20 - 1, 128, 1024, lda0=2048), dma=1) == (3, 0)
    assert route(desc(2**20, 128, 1024, lda0=2048), dma=1) == (2, 0)
    assert route(desc(2**20 - 1, 128, 64, 64, lda1=2048), dma=1) == (3, 0)
    assert route(desc(2**20, 128, 64, 64, lda1=2048), dma=1) == (2, 0)
    # N K 2 = 2^32 - 2^23 against exactly 2^32
    assert route(desc(256, 65536, 32768 - 64), dma=1) == (4, 0)
    assert route(desc(256, 65536, 32768), dma=1) == (2, 0)


# ---- refusals
def test_refuses_n_and_k_that_no_kernel_takes():
    assert refused(desc(256, 48, 64))
    assert refused(desc(256, 0, 64))
    assert refused(desc(256, 128, 48))
    assert refused(desc(256, 128, 64, 16))
    assert refused(desc(256, 128, 0))
    assert refused(desc(256, 128, 8), F32)
    assert refused(desc(256, 128, 64), dtype=L.F16)
    assert refused(desc(256, 128, 64, 64, a1=None))
    assert route(desc(256, 128, 16), F32) == (1, 0)


@pytest.mark.parametrize("field", ["a0", "a1", "w", "bias", "res", "c", "c2", "aux"])
def test_refuses_misaligned_pointers(field):
    base = dict(res=True, K1=64) if field in ("a1", "res") else {}
    epi = 1 if field == "c2" else 2 if field == "aux" else 0
    d = desc(65536, 1024, 64, base.get("K1", 0), res=base.get("res", False), bias=field == "bias", epi=epi)
    assert route(d, dma=1)[0] in (3, 4)
    setattr(d, field, getattr(d, field) + 8)
    assert refused(d, dma=1)


def test_refuses_strides_the_loads_cannot_take():
    assert refused(desc(256, 128, 64, lda0=68))                 # bf16 A rows: whole 16-byte pieces
    assert refused(desc(256, 128, 64, 64, lda1=68))
    assert refused(desc(256, 128, 64, lda0=66), F32)
    assert route(desc(256, 128, 32, lda0=36), F32) == (2, 0)      # (f32: 16 bytes = 4 elements)
    assert route(desc(256, 128, 64, lda0=72)) == (2, 0)           # (a row stride needs whole pieces, not whole chunks)
    assert refused(desc(256, 128, 64, ldc=130))
    # a residual row stride that is not whole 16-byte pieces leaves only the kernel that reads it element by element
    assert route(desc(256, 128, 64, res=True, ldr=132)) == (1, 0)
    assert route(desc(65536, 1024, 64, res=True, ldr=1028), dma=1) == (1, 0)
    assert route(desc(65536, 1024, 64, res=True, ldr=1032), dma=1) == (4, 0)


def test_refuses_batched_launches_it_cannot_run():
    ok = dict(batch=3, a_bstride=256 * 64, w_bstride=128 * 64, c_bstride=256 * 128)
    assert route(desc(256, 128, 64, **ok)) == (2, 0)
    assert route(desc(100, 128, 64, **ok)) == (1, 0)
    assert route(desc(65536, 1024, 64, **ok), dma=1) == (2, 0)   # never on the DMA kernels
    assert refused(desc(256, 128, 64, 64, **ok))
    assert refused(desc(256, 128, 64, res=True, **ok))
    assert refused(desc(256, 128, 64, bias=True, **ok))
    assert route(desc(256, 128, 64, **dict(ok, batch=65535))) == (2, 0)
    assert refused(desc(256, 128, 64, **dict(ok, batch=65536)))
    assert refused(desc(256, 128, 64, **dict(ok, a_bstride=256 * 64 + 4)))
    assert refused(desc(256, 128, 64, **dict(ok, c_bstride=256 * 128 + 4)))


def test_refuses_epilogues_off_the_dma_kernels():
    assert route(desc(65536, 1024, 64, epi=1), dma=1) == (4, 0)
    assert route(desc(65536, 1152, 64, epi=2), dma=1) == (3, 0)
    assert refused(desc(65536, 1024, 64, epi=1), dma=0)
    assert refused(desc(1024, 1024, 64, epi=1), dma=1)           # too few tiles
    assert refused(desc(65536, 1024, 64, epi=1), F32, dma=1)
    assert refused(desc(65536, 1024, 64, epi=3), dma=1)
    assert refused(desc(65536, 1024, 64, epi=1, c2=None), dma=1)
    assert refused(desc(65536, 1024, 64, epi=2, aux=None), dma=1)
    assert refused(desc(65536, 1024, 64, epi=1, ldc2=1028), dma=1)


# ---- the callers' shape families, pinned to the kernel each takes today
VIT_M, VIT_W = 1024 * 197, 768
CALLERS = [
    # CLIP ViT-B/16 image tower (transformer.hip block_gemm(), ctx option gemm_dma = 1): forward, then the backward's transposed products
    ("vit qkv", desc(VIT_M, 3 * VIT_W, VIT_W, bias=True), BF16, 1, (4, 0)),
    ("vit out_proj + residual", desc(VIT_M, VIT_W, VIT_W, bias=True, res=True), BF16, 1, (4, 0)),
    ("vit c_fc + QuickGELU", desc(VIT_M, 4 * VIT_W, VIT_W, bias=True, epi=1), BF16, 1, (4, 0)),
    ("vit c_proj + residual", desc(VIT_M, VIT_W, 4 * VIT_W, bias=True, res=True), BF16, 1, (4, 0)),
    ("vit d c_proj * QuickGELU'", desc(VIT_M, 4 * VIT_W, VIT_W, epi=2), BF16, 1, (4, 0)),
    ("vit d c_fc", desc(VIT_M, VIT_W, 4 * VIT_W), BF16, 1, (4, 0)),
    ("vit patch embedding", desc(1024 * 196, VIT_W, 768), BF16, 1, (4, 0)),
    ("vit qkv, gemm_dma 0", desc(VIT_M, 3 * VIT_W, VIT_W, bias=True), BF16, 0, (2, 0)),
    ("vit out_proj, gemm_dma 0", desc(VIT_M, VIT_W, VIT_W, bias=True, res=True), BF16, 0, (2, 6)),
    ("vit out_proj, f32", desc(VIT_M, VIT_W, VIT_W, bias=True, res=True), F32, 1, (2, 6)),
    ("vit few cutouts", desc(8 * 197, 3 * VIT_W, VIT_W, bias=True), BF16, 1, (2, 0)),
    # CLIP text tower (text_gemm, never DMA; at least 128 rows)
    ("text qkv", desc(128, 1536, 512, bias=True), BF16, 0, (2, 0)),
    ("text c_proj + residual", desc(4 * 77, 512, 2048, bias=True, res=True), BF16, 0, (2, 0)),
    # guided-diffusion UNet 1x1 layers (unet.hip, never DMA): 64^2 and 8^2 at batch 1 and 16
    ("unet 64^2 skip, virtual concat", desc(64 * 64, 256, 256, 256, bias=True), BF16, 0, (2, 0)),
    ("unet 64^2 skip, 96-channel part", desc(64 * 64, 128, 96, 160, bias=True), BF16, 0, (1, 0)),
    ("unet 64^2 b16 skip", desc(16 * 64 * 64, 256, 256, 256, bias=True), BF16, 0, (2, 2)),
    ("unet 64^2 b16 attention qkv", desc(16 * 64 * 64, 768, 256, bias=True), BF16, 0, (2, 6)),
    ("unet 64^2 b16 proj_out + residual", desc(16 * 64 * 64, 256, 256, bias=True, res=True), BF16, 0, (2, 2)),
    ("unet 8^2 attention qkv", desc(8 * 8, 3 * 512, 512, bias=True), BF16, 0, (1, 0)),
    ("unet 8^2 b16 skip", desc(16 * 8 * 8, 512, 1024, 512, bias=True), BF16, 0, (2, 0)),
    ("unet 8^2 f32 proj_out", desc(8 * 8, 512, 512, bias=True, res=True), F32, 0, (1, 0)),
    # perceptor Gram head: F_b (dG_b + dG_b^T), all images in one batched launch
    ("gram 224^2 C 64", desc(224 * 224, 64, 64, batch=4, a_bstride=224 * 224 * 64, w_bstride=64 * 64, c_bstride=224 * 224 * 64),
     BF16, 0, (2, 0)),
    ("gram 14^2 C 512 f32", desc(14 * 14, 512, 512, batch=4, a_bstride=196 * 512, w_bstride=512 * 512, c_bstride=196 * 512),
     F32, 0, (2, 0)),
    ("gram 7^2 C 512", desc(7 * 7, 512, 512, batch=4, a_bstride=49 * 512, w_bstride=512 * 512, c_bstride=49 * 512), BF16, 0, (1, 0)),
]


@pytest.mark.parametrize("name,d,dtype,dma,want", CALLERS, ids=[c[0] for c in CALLERS])
def test_caller_shape_families_keep_their_kernel(name, d, dtype, dma, want):
    assert route(d, dtype, dma) == want
