"""CPU-only: which kernel a plain 3x3 convolution runs on, with which tile and how many K slices, and what each kernel refuses,
through the host-only maua_conv3x3_route.  Kernels: 1 = generic (csrc/modconv.hip; variant = which of its tile rules fires, 1 .. 9),
2 = LDS-direct (csrc/modconv_dma.hip; variant = output channels per workgroup, + 1 odd-chunk form, + 2 piece sums), 3 = split-K gather GEMM
(csrc/modconv_lowres.hip; ksplit = its K slices).  Option 0 / 1 / 2 is the diffusion UNet's routing (Runner::conv, csrc/unet.hip) under
that "route" option; 100 + k forces kernel k.  Every threshold is pinned on both sides, and the real callers' shape families are pinned
to what they take: a routing change shows up as a diff of these tables.  Pointers are fake (the route never dereferences them)."""
import ctypes as C

import pytest

from maua_amd import _lib as L

F32, BF16, F16, SPLIT = L.F32, L.BF16, L.F16, L.F32_SPLIT
X, Wt, Y, RES, RES2, PSUM = (0x10000 * (i + 1) for i in range(6))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from maua_amd.build import build
    build()


def route(B, H, W, Ci, Co, dtype=BF16, opt=0, **kw):
    """(kernel, variant, ksplit), or the refusal text"""
    d = L.ConvDesc(x=X, w=Wt, y=Y, x_bstride=H * W * Ci, B=B, H=H, W=W, Ci=Ci, Co=Co, act=0, alpha=1.0, gain=1.0, clamp=-1.0)
    for k, v in kw.items():
        setattr(d, k, v)
    var, ks = C.c_int(-1), C.c_int(-1)
    rc = L.lib().maua_conv3x3_route(C.byref(d), dtype, opt, C.byref(var), C.byref(ks))
    if rc < 0:
        return L.lib().maua_last_error().decode()
    return rc, var.value, ks.value


def refused(prefix, *a, **kw):
    r = route(*a, **kw)
    return isinstance(r, str) and r.startswith(prefix)


# ---- the UNet's routing: workgroup thresholds 512 and 128, the gather GEMM's 1024 pixels
def test_wide_tile_workgroup_thresholds():
    # 64 x 64 pixels = 16 tiles of 8 x 32 per sample; Co = 256: one 256-channel tile each -> 16 B workgroups
    assert route(31, 64, 64, 256, 256) == (2, 128, 0)        # 496 < 512: 128-channel tiles, twice the workgroups
    assert route(32, 64, 64, 256, 256) == (2, 256, 0)        # 512
    # Co = 128 never divides by 256: the 128-channel tile whatever the count
    assert route(64, 64, 64, 256, 128) == (2, 128, 0)
    # 32 x 32 pixels = 4 tiles per sample, Co = 512 -> 8 B workgroups, doubled below 512 -> 16 B; the gather GEMM takes the layer below 128
    assert route(7, 32, 32, 512, 512) == (3, 0, 4)           # 112 workgroups
    assert route(8, 32, 32, 512, 512) == (2, 128, 0)         # 128
    assert route(7, 32, 32, 512, 512, opt=2) == (2, 128, 0)  # "route" 2: never the gather GEMM
    assert route(7, 32, 32, 512, 512, opt=1) == (1, 6, 0)    # "route" 1: always the generic kernel
    # Co = 128 at 32 x 32: 4 B workgroups, not doubled
    assert route(31, 32, 32, 512, 128) == (3, 0, 6)
    assert route(32, 32, 32, 512, 128) == (2, 128, 0)


def test_gather_pixel_threshold_and_its_shapes():
    assert route(1, 32, 32, 256, 256)[0] == 3                # 1024 pixels
    assert route(1, 32, 64, 256, 256) == (2, 128, 0)         # 2048: too few workgroups, but no gather GEMM to take it
    assert route(1, 33, 31, 256, 256)[0] == 3                # 1023 pixels
    assert route(1, 25, 41, 256, 256) == (1, 6, 0)           # 1025
    assert route(1, 16, 16, 256, 256) == (3, 0, 36)
    assert route(1, 16, 16, 256, 192) == (1, 8, 0)           # Co % 128
    assert route(1, 16, 16, 96, 256) == (1, 1, 0)            # bf16: Ci in whole 128-byte chunks
    assert route(1, 16, 16, 96, 256, F32) == (3, 0, 27)
    assert route(1, 16, 16, 256, 256, F16) == (1, 1, 0)      # bf16 / f32 only
    assert route(1, 16, 16, 256, 256, SPLIT) == (1, 1, 0)
    assert route(1, 64, 64, 256, 256, F32) == (1, 2, 0)      # float32 has no LDS-direct kernel


def test_narrow_tiles_in_the_unet_routing():
    assert route(1, 256, 256, 256, 32) == (2, 32, 0)
    assert route(1, 256, 256, 96, 32) == (2, 33, 0)
    assert route(1, 256, 256, 64, 64) == (2, 64, 0)
    assert route(1, 256, 256, 32, 32) == (1, 9, 0)           # one chunk: generic
    assert route(1, 7, 32, 64, 32) == (1, 9, 0)              # less than a tile
    assert route(1, 8, 31, 64, 32) == (1, 9, 0)


# ---- the generic kernel's tile rules
@pytest.mark.parametrize("dtype,k128,odd", [(BF16, 64, 96), (F16, 64, 96), (F32, 32, None), (SPLIT, 32, None)])
def test_generic_tile_boundaries(dtype, k128, odd):
    g = lambda H, W, Ci, Co: route(2, H, W, Ci, Co, dtype, 101)
    assert g(16, 16, k128, 128) == (1, 1, 0) and g(16, 17, k128, 128) == (1, 6, 0)          # H W <= 256 with Co % 128 == 0
    assert g(64, 64, k128, 128) == (1, 2, 0) and g(63, 65, k128, 128) == (1, 6, 0)          # H W >= 4096 (63 x 65 = 4095)
    if odd:
        assert g(64, 64, odd, 128) == (1, 3, 0)                                             # ... without whole 128-byte K chunks
    assert g(64, 64, k128, 64) == (1, 7, 0) and g(63, 65, k128, 64) == (1, 8, 0)            # 64 channels: large / small map
    assert g(64, 64, k128, 192) == (1, 7, 0) and g(16, 16, k128, 192) == (1, 8, 0)
    assert g(64, 64, k128, 96) == (1, 9, 0) and g(1, 1, k128, 32) == (1, 9, 0) and g(16, 16, k128, 160) == (1, 9, 0)


# ---- the LDS-direct kernel's tiles
def test_dma_tiles():
    d = lambda H, W, Ci, Co, dtype=BF16, **kw: route(2, H, W, Ci, Co, dtype, 102, **kw)
    assert d(8, 32, 64, 256) == (2, 256, 0) and d(8, 32, 64, 256, variant=128) == (2, 128, 0)
    assert d(8, 32, 64, 256, psum=PSUM) == (2, 258, 0) and d(8, 32, 64, 384, psum=PSUM) == (2, 130, 0)
    assert d(8, 32, 64, 128) == (2, 128, 0) and d(8, 32, 64, 384) == (2, 128, 0) and d(8, 32, 64, 512) == (2, 256, 0)
    assert d(8, 32, 64, 256, F16) == (2, 256, 0) and d(8, 32, 64, 128, F16) == (2, 128, 0)
    assert d(8, 32, 64, 64) == (2, 64, 0) and d(9, 33, 128, 32) == (2, 32, 0)
    assert d(9, 33, 96, 32) == (2, 33, 0) and d(9, 33, 160, 32) == (2, 33, 0)


# ---- the gather GEMM's K slices (lowres_geom): 9 Ci / (128 bytes) stages; the smallest divisor of that >= 256 / (64 x 128 tiles per sample),
# then the fewest slices that still give 2048 workgroups
def test_gather_ksplit_steps():
    k = lambda B, H, W, Ci, Co, dtype=BF16: route(B, H, W, Ci, Co, dtype, 103)[2]
    assert [k(B, 8, 8, 1024, 1024) for B in (1, 4, 8, 16, 32, 64)] == [36, 36, 36, 16, 8, 4]
    # 32 x 32, Co = 1024: 16 x 8 tiles per sample - 2048 tiles at batch 16 need one slice, 2047 two
    assert k(16, 32, 32, 128, 1024) == 1 and k(15, 32, 32, 128, 1024) == 2
    assert k(16, 32, 24, 128, 1024) == 2
    assert k(1, 8, 8, 1024, 128) == 144 and k(1, 8, 8, 64, 128) == 9                          # every stage its own slice
    assert k(1, 8, 8, 512, 128, F32) == 144 and k(1, 16, 16, 256, 256, F32) == 36
    assert k(1, 32, 32, 512, 512) == 4 and k(1, 16, 16, 512, 512) == 18 and k(1, 16, 16, 1024, 1024) == 8


# ---- refusals, with the launcher's own text
def test_refusals():
    assert refused("maua_conv3x3: unsupported dtype", 1, 8, 32, 64, 64, 7)
    assert refused("maua_conv3x3: bad shape", 1, 0, 32, 64, 64)
    assert refused("maua_conv3x3: NULL x / w / y", 1, 8, 32, 64, 64, y=None)
    assert refused("maua_conv3x3: res2 goes with res", 1, 8, 32, 64, 64, res2=RES2)
    assert refused("maua_conv3x3: bad strides / Ci_read", 1, 8, 32, 64, 64, Ci_read=65)
    assert refused("maua_conv3x3: kernel must be", 1, 8, 32, 64, 64, opt=3)
    assert refused("maua_conv3x3: kernel must be", 1, 8, 32, 64, 64, opt=104)
    # generic
    assert refused("modconv3x3: Ci must be a multiple of 32", 1, 8, 32, 48, 64, opt=101)
    assert refused("modconv3x3: Co must be a multiple of 32", 1, 8, 32, 64, 48, opt=101)
    assert refused("modconv3x3: grid too large", 65536, 8, 32, 64, 64, opt=101)
    for kw in (dict(x_up2=1), dict(psum=PSUM), dict(Ci_read=32)):
        assert refused("modconv3x3: no x_up2 / psum / Ci_read", 1, 8, 32, 64, 64, opt=101, **kw)
    # LDS-direct
    assert refused("modconv_dma: unsupported dtype", 1, 8, 32, 64, 128, F32, 102)
    assert refused("modconv_dma: unsupported shape", 1, 8, 32, 96, 64, opt=102)              # 64 channels with an odd chunk count
    assert refused("modconv_dma: unsupported shape", 1, 8, 32, 64, 96, opt=102)
    assert refused("modconv_dma: unsupported shape", 1, 9, 33, 64, 128, opt=102)             # the wide tiles do not overhang
    assert refused("modconv_dma: unsupported shape", 1, 7, 32, 64, 32, opt=102)
    assert refused("modconv_dma: unsupported shape", 1, 8, 32, 32, 32, opt=102)               # one 32-channel chunk
    assert refused("modconv_dma: grid too large", 65536, 8, 32, 64, 128, opt=102)
    assert refused("modconv_dma: x_up2 needs even output sizes", 1, 9, 33, 64, 32, opt=102, x_up2=1)
    assert refused("modconv_dma: a sample must stay below 4 GiB", 1, 8192, 8192, 64, 32, opt=102)
    assert refused("modconv_dma: the narrow tiles carry no", 1, 8, 32, 64, 32, opt=102, psum=PSUM)
    for kw in (dict(psum=PSUM), dict(x_up2=1)):
        assert refused("modconv_dma (f16): unsupported shape / arguments", 1, 8, 32, 64, 128, F16, 102, **kw)
    assert refused("modconv_dma (f16): unsupported shape / arguments", 1, 8, 32, 64, 64, F16, 102)   # no narrow f16 tiles
    # gather GEMM
    g = "conv_gather: unsupported shape / arguments"
    assert refused(g, 1, 33, 32, 64, 128, opt=103) and refused(g, 1, 8, 8, 64, 64, opt=103) and refused(g, 1, 8, 8, 32, 128, opt=103)
    assert refused(g, 1, 8, 8, 64, 128, F16, 103) and refused(g, 1, 8, 8, 64, 128, SPLIT, 103) and refused(g, 1, 8, 8, 16, 128, F32, 103)
    for kw in (dict(x_pstride=128), dict(res=RES, res2=RES2), dict(x_up2=1), dict(psum=PSUM), dict(Ci_read=32)):
        assert refused(g, 1, 8, 8, 64, 128, opt=103, **kw)
    assert refused("conv_gather: the input must be dense", 1, 8, 8, 64, 128, opt=103, x_bstride=8 * 8 * 64 + 64)
    assert refused("conv_gather: 32-bit pixel indices", 65536, 32, 32, 64, 128, opt=103)


# ---- the real callers' shape families
def _unet_convs(cfg):
    """(size, Ci, Co), padded to 32 channels, of every 3x3 convolution of a UNet (oracle.diffusion.unet_structure's walk)"""
    from oracle import diffusion as OD
    s, p32, out = OD.unet_structure(cfg), lambda c: (c + 31) // 32 * 32, []
    res = cfg["image_size"]
    out.append((res, p32(cfg["in_channels"]), p32(s["input"][0][0][2])))
    for layers in s["input"][1:] + [s["middle"]] + s["output"]:
        for l in layers:
            if l[0] == "res":
                res = res // 2 if l[3] == "down" else res * 2 if l[3] == "up" else res
                out += [(res, p32(l[1]), p32(l[2])), (res, p32(l[2]), p32(l[2]))]
    out.append((res, p32(s["final_ch"]), p32(cfg["out_channels"])))
    return sorted(set(out))


# size -> batch -> {resolution: what its convolutions take}.  "g3" = generic rule 3, "d256" / "d128" / "d32" = LDS-direct tile, "k36" = gather
# GEMM with 36 K slices; a level whose layers differ lists them by (Ci, Co)
def _tag(r):
    return f"g{r[1]}" if r[0] == 1 else f"d{r[1]}" if r[0] == 2 else f"k{r[2]}"


def _unet_table(size, B):
    from oracle import diffusion as OD
    t = {}
    for (s, Ci, Co) in _unet_convs(OD.unet_config(image_size=size)):
        t.setdefault(s, {})[(Ci, Co)] = _tag(route(B, s, s, Ci, Co))
    return {s: (set(v.values()).pop() if len(set(v.values())) == 1 else v) for s, v in t.items()}


UNET_256 = {1: {8: {(1024, 1024): 'k36', (2048, 1024): 'k32'},
     16: {(512, 512): 'k18', (512, 1024): 'k8', (1024, 1024): 'k8', (1536, 1024): 'k8', (2048, 1024): 'k8'},
     32: {(512, 512): 'k4', (1024, 512): 'k4', (1024, 1024): 'k2', (1536, 512): 'k4'},
     64: 'd128',
     128: 'd128',
     256: {(32, 256): 'g3', (256, 32): 'd32', (256, 256): 'd128', (512, 256): 'd128'}},
 4: {8: {(1024, 1024): 'k36', (2048, 1024): 'k32'},
     16: {(512, 512): 'k18', (512, 1024): 'k8', (1024, 1024): 'k8', (1536, 1024): 'k8', (2048, 1024): 'k8'},
     32: {(512, 512): 'k4', (1024, 512): 'k4', (1024, 1024): 'd128', (1536, 512): 'k4'},
     64: 'd128',
     128: {(256, 256): 'd128', (512, 256): 'd128', (512, 512): 'd256', (768, 256): 'd128'},
     256: {(32, 256): 'g3', (256, 32): 'd32', (256, 256): 'd256', (512, 256): 'd256'}}}


@pytest.mark.parametrize("B", [1, 4])
def test_unet_256_levels(B):
    got = _unet_table(256, B)
    assert got == UNET_256[B], got


@pytest.mark.parametrize("size,B,want", [
    (256, 1, {'d128': 11, 'd32': 1, 'g3': 1, 'k18': 1, 'k2': 1, 'k32': 1, 'k36': 1, 'k4': 3, 'k8': 4}),
    (256, 4, {'d128': 9, 'd256': 3, 'd32': 1, 'g3': 1, 'k18': 1, 'k32': 1, 'k36': 1, 'k4': 3, 'k8': 4}),
    (256, 16, {'d128': 5, 'd256': 10, 'd32': 1, 'g3': 1, 'k16': 2, 'k4': 4, 'k8': 1}),
    (256, 32, {'d128': 3, 'd256': 12, 'd32': 1, 'g3': 1, 'k2': 4, 'k4': 1, 'k8': 2}),
    (512, 1, {'d128': 17, 'd256': 1, 'd32': 1, 'g3': 1, 'k18': 1, 'k2': 1, 'k32': 1, 'k36': 1, 'k4': 3, 'k8': 4}),
    (512, 4, {'d128': 13, 'd256': 6, 'd32': 1, 'g3': 1, 'k18': 1, 'k32': 1, 'k36': 1, 'k4': 3, 'k8': 4}),
    (512, 16, {'d128': 9, 'd256': 13, 'd32': 1, 'g3': 1, 'k16': 2, 'k4': 4, 'k8': 1}),
    (512, 32, {'d128': 7, 'd256': 15, 'd32': 1, 'g3': 1, 'k2': 4, 'k4': 1, 'k8': 2}),
])
def test_unet_route_census(size, B, want):
    """every distinct 3x3 convolution of the default UNet of that size, counted by what it takes"""
    from oracle import diffusion as OD
    got = {}
    for (s, Ci, Co) in _unet_convs(OD.unet_config(image_size=size)):
        tag = _tag(route(B, s, s, Ci, Co))
        got[tag] = got.get(tag, 0) + 1
    assert got == want, got


def test_rrdb_trunk_at_1034():
    """RealESRGAN's RRDBNet(64 features, 32 growth) on a 1024^2 frame pre-padded to 1034 x 1034 (csrc/super.hip: the dense block's
    convolutions read 64 + 32 k channels, K padded to whole 64-channel chunks except where the 32-channel odd-chunk form takes it),
    bf16: all on the LDS-direct narrow tiles, which overhang the frame"""
    d = lambda Ci, Co, s=1034, x_pstride=192, **kw: route(1, s, s, Ci, Co, BF16, 102, x_pstride=x_pstride, **kw)
    assert [d(Ci, 32) for Ci in (64, 96, 128, 160)] == [(2, 32, 0), (2, 33, 0), (2, 32, 0), (2, 33, 0)]
    assert d(192, 64) == (2, 64, 0)                                       # conv5
    assert d(64, 64) == (2, 64, 0)                                        # conv_first's successor layers: conv_body, conv_hr
    assert d(64, 64, s=2068, x_up2=1, x_pstride=64) == (2, 64, 0)         # conv_up1 on the virtual x2 up-sampling
    assert d(64, 32, s=4136, x_pstride=64) == (2, 32, 0)                  # conv_last
    assert route(1, 1034, 1034, 32, 64, BF16, 101) == (1, 7, 0)           # conv_first (3 -> 64, one chunk): generic
    # float16 / float32 networks: the generic kernel throughout
    assert route(1, 1034, 1034, 96, 32, F16, 101) == (1, 9, 0) and route(1, 1034, 1034, 192, 64, F32, 101) == (1, 7, 0)


def test_secondary_model_at_256():
    """the secondary diffusion model (csrc/secondary.hip: always launch_modconv3x3, split float32 by default) at 256 x 256: channels
    64, 128, 128, 256, 256, 512 over six levels"""
    for dtype in (SPLIT, BF16):
        g = lambda s, Ci, Co: route(16, s, s, Ci, Co, dtype, 101)[1]
        assert [g(256, 32, 64), g(256, 64, 64), g(256, 128, 64), g(256, 64, 32)] == [7, 7, 7, 9]
        assert [g(128, 64, 128), g(128, 128, 128), g(128, 256, 128), g(128, 128, 64)] == [2, 2, 2, 7]
        assert [g(64, 128, 128), g(64, 256, 128)] == [2, 2]
        assert [g(32, 128, 256), g(32, 256, 256), g(32, 512, 256), g(32, 256, 128)] == [6, 6, 6, 6]
        assert [g(16, 256, 256), g(16, 512, 256)] == [1, 1]
        assert [g(8, 256, 512), g(8, 512, 512), g(8, 512, 256)] == [1, 1, 1]


@pytest.mark.parametrize("size", [224, 256])
def test_vgg_layers(size):
    """VGG-19's convolutions (csrc/perceptor.hip: bf16 on the LDS-direct kernel where its tiles fit, else generic)"""
    from maua_amd.perceptors import VGG19_CFG
    got, s, Ci = [], size, 32
    for v in VGG19_CFG:
        if v == "M":
            s //= 2
            continue
        wide, narrow = route(4, s, s, Ci, v, BF16, 102), route(4, s, s, Ci, v, BF16, 101)
        got.append((s, Ci, v, _tag(wide) if not isinstance(wide, str) else _tag(narrow)))
        Ci = v
    s0 = size
    want = [(s0, 32, 64, "g7"), (s0, 64, 64, "d64"), (s0 // 2, 64, 128, "d128" if size == 256 else "g2"),
            (s0 // 2, 128, 128, "d128" if size == 256 else "g2")]
    want += [(s0 // 4, 128 if i == 0 else 256, 256, "d256" if size == 256 else "g6") for i in range(4)]
    want += [(s0 // 8, 256 if i == 0 else 512, 512, "d256" if size == 256 else "g6") for i in range(4)]
    want += [(s0 // 16, 512, 512, "g1") for i in range(4)]
    assert got == want, got
