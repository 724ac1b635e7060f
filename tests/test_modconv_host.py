"""CPU-only: which routes of the synthesis forward (csrc/synth.hip's Route enum) can compute a modulated 3x3 layer, through the host-only
maua_modconv_route: every predicate's thresholds pinned on both sides, every refusal with the launcher's own text, and the tile / slice
choice the launcher would make.  Pointers are fake (the route never dereferences them; they are 16-byte aligned as the FIR / epilogue pass
asks).  The method of tests/test_conv_host.py."""
import ctypes as C

import pytest

from maua_amd import _lib as L

F32, BF16, F16 = L.F32, L.BF16, L.F16
R = L.ROUTES
X, Wt, S, D, Y, NZ, BIAS, OSC, YS, WM, RB, PREV, RGB, RGB8, T = (0x100000 * (i + 1) for i in range(15))


@pytest.fixture(scope="module", autouse=True)
def _built():
    from maua_amd.build import build
    build()


def desc(B, H, W, Ci, Co, up=1, **kw):
    d = L.ModconvDesc(x=X, x_bstride=H * W * Ci, w=Wt, s=S, d=D, noise=NZ, noise_bstride=H * up * W * up, noise_strength=1.0, bias=BIAS, y=Y,
                      B=B, H=H, W=W, Ci=Ci, Co=Co, up=up, act=2, alpha=0.25, gain=2.0, clamp=256.0, rgb_clamp=256.0)
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def route(name, B, H, W, Ci, Co, up=1, dtype=BF16, d1=None, **kw):
    """the tile / slice count the route reports, or the refusal text"""
    d = desc(B, H, W, Ci, Co, up, **kw)
    tile = C.c_int(-1)
    rc = L.lib().maua_modconv_route(C.byref(d), C.byref(d1) if d1 is not None else None, dtype, R[name], C.byref(tile))
    return L.lib().maua_last_error().decode() if rc else tile.value


def ok(*a, **kw):
    return not isinstance(route(*a, **kw), str)


def refused(prefix, *a, **kw):
    r = route(*a, **kw)
    return isinstance(r, str) and r.startswith(prefix)


RGBKW = dict(rgb_wmod=WM, rgb_bias=RB, rgb_prev=PREV, rgb_out=RGB)


def test_descriptor_checks():
    assert refused("maua_modconv: unsupported dtype", "generic", 1, 8, 8, 32, 32, dtype=3)
    assert refused("maua_modconv: no such route", "walk_done", 1, 8, 8, 32, 32)
    assert refused("maua_modconv: bad shape", "generic", 1, 0, 8, 32, 32)
    assert refused("maua_modconv: NULL x / w", "generic", 1, 8, 8, 32, 32, w=None)
    assert refused("maua_modconv: NULL styles", "generic", 1, 8, 8, 32, 32, s=None)
    assert refused("maua_modconv: up must be 1 or 2", "generic", 1, 8, 8, 32, 32, up=3)
    assert refused("maua_modconv: NULL y", "generic", 1, 8, 8, 32, 32, y=None)
    assert refused("maua_modconv: samples of x overlap", "generic", 2, 8, 8, 32, 32, x_bstride=8 * 8 * 32 - 32)
    assert refused("maua_modconv: a second layer goes with the fused walk only", "generic", 1, 8, 8, 32, 32, d1=desc(1, 8, 8, 32, 32))


def test_generic_route_and_tiles():
    g = lambda *a, **kw: route("generic", 2, *a, **kw)
    # modconv_tile with styles: up == 2 layers carry their four parities in N (cov = 4 Co), so rules 4 and 5 are reachable
    assert g(16, 16, 64, 128) == 1 and g(16, 17, 64, 128) == 6
    assert g(64, 64, 64, 128) == 2 and g(64, 64, 96, 128) == 3 and g(63, 65, 64, 128) == 6
    assert g(16, 16, 64, 32, up=2) == 4 and g(16, 16, 96, 32, up=2) == 6
    assert g(8, 8, 64, 32, up=2) == 5 and g(8, 8, 64, 64, up=2) == 5 and g(8, 8, 96, 64, up=2) == 6
    assert g(64, 64, 64, 64) == 7 and g(63, 65, 64, 64) == 8 and g(8, 8, 64, 32) == 9 and g(64, 64, 64, 96) == 9
    assert g(16, 16, 32, 128, dtype=F32) == 1 and g(64, 64, 32, 128, dtype=F32) == 2
    assert g(8, 8, 64, 32, x_bstride=0) == 9                                        # the const input
    assert refused("modconv3x3: Ci must be a multiple of 32", "generic", 1, 8, 8, 48, 32)
    assert refused("modconv3x3: Co must be a multiple of 32", "generic", 1, 8, 8, 32, 48)
    assert refused("modconv3x3: grid too large", "generic", 65536, 8, 8, 32, 32)
    assert refused("modconv3x3: no y_scaled", "generic", 1, 8, 8, 32, 32, out_scale=OSC, y_scaled=YS)
    # the fused toRGB: 16-bit types, up == 1, 128 channels on a 128-channel N tile (rules 2 .. 6: more than 256 pixels)
    assert ok("generic", 1, 64, 64, 64, 128, **RGBKW) and ok("generic", 1, 16, 18, 64, 128, **RGBKW)
    f = "modconv3x3: fused toRGB needs bf16, up == 1 and all output channels in one N tile"
    assert refused(f, "generic", 1, 16, 16, 64, 128, **RGBKW)                       # rule 1: 32-channel tiles
    assert refused(f, "generic", 1, 64, 64, 64, 256, **RGBKW) and refused(f, "generic", 1, 64, 64, 64, 64, **RGBKW)
    assert refused(f, "generic", 1, 64, 64, 32, 128, dtype=F32, **RGBKW)
    assert refused(f, "generic", 1, 32, 32, 64, 32, up=2, **RGBKW)
    assert refused(f, "generic", 1, 64, 64, 64, 128, **dict(RGBKW, rgb_wmod=None))
    assert refused("modconv3x3: fused toRGB and out_scale exclude each other", "generic", 1, 64, 64, 64, 128, out_scale=OSC, **RGBKW)


def test_lowres_route_and_slices():
    lo = lambda *a, **kw: route("lowres", *a, **kw)
    # 64 pixels; Ci in whole 128-byte chunks (bf16 64, f32 32 channels); Co % 32; whole tiles of 128 virtual output channels (any such Co with up == 2)
    assert ok("lowres", 1, 8, 8, 64, 128) and ok("lowres", 1, 4, 16, 64, 128) and ok("lowres", 1, 1, 64, 64, 128)
    u = "modconv_lowres: unsupported shape"
    assert refused(u, "lowres", 1, 5, 13, 64, 128) and refused(u, "lowres", 1, 8, 9, 64, 128)          # 65 / 72 pixels
    assert refused(u, "lowres", 1, 8, 8, 32, 128) and ok("lowres", 1, 8, 8, 32, 128, dtype=F32)
    assert refused(u, "lowres", 1, 8, 8, 48, 128, dtype=F32)
    assert refused(u, "lowres", 1, 8, 8, 64, 64) and ok("lowres", 1, 8, 8, 64, 32, up=2) and ok("lowres", 1, 8, 8, 64, 96, up=2)
    assert refused(u, "lowres", 1, 8, 8, 64, 128, dtype=F16)
    # K slices (lowres_geom, from the shape alone): 9 Ci / 64 stages; the smallest divisor >= max(2, 18 / tiles per sample)
    assert [lo(B, 4, 4, 512, 512) for B in (1, 2, 3, 32)] == [18, 18, 18, 18]
    assert lo(1, 8, 8, 512, 512) == 4 and lo(1, 4, 4, 512, 512, up=2) == 4 and lo(1, 8, 8, 512, 512, up=2) == 2
    assert lo(1, 8, 8, 64, 128) == 9 and lo(1, 2, 2, 128, 128) == 18 and lo(1, 8, 8, 64, 128, dtype=F32) == 18
    assert lo(1, 1, 7, 320, 128) == 45
    i = "modconv_lowres: no out_scale / y_scaled / fused toRGB"
    assert refused(i, "lowres", 1, 8, 8, 64, 128, out_scale=OSC) and refused(i, "lowres", 1, 8, 8, 64, 128, **RGBKW)
    assert refused("modconv_lowres: 32-bit pixel indices", "lowres", 1 << 20, 8, 8, 64, 128)


def test_dma_conv1_route_and_tiles():
    d = lambda *a, **kw: route("dma_conv1", 2, *a, **kw)
    assert d(8, 32, 64, 128) == 128 and d(8, 32, 64, 256) == 256 and d(8, 32, 64, 384) == 128 and d(8, 32, 64, 512) == 256
    assert d(8, 32, 64, 256, dtype=F16) == 256 and d(16, 64, 192, 128, dtype=F16) == 128
    u = "modconv_dma: unsupported shape"
    assert refused(u, "dma_conv1", 1, 8, 32, 32, 128) and refused(u, "dma_conv1", 1, 8, 32, 96, 128)      # Ci % 64
    assert refused(u, "dma_conv1", 1, 8, 32, 64, 64) and refused(u, "dma_conv1", 1, 8, 32, 64, 192)       # Co % 128 (no narrow tiles here)
    assert refused(u, "dma_conv1", 1, 7, 32, 64, 128) and refused(u, "dma_conv1", 1, 12, 32, 64, 128)     # H % 8
    assert refused(u, "dma_conv1", 1, 8, 31, 64, 128) and refused(u, "dma_conv1", 1, 8, 48, 64, 128)      # W % 32
    assert refused(u, "dma_conv1", 1, 8, 32, 64, 128, up=2)
    assert refused("modconv_dma: unsupported dtype", "dma_conv1", 1, 8, 32, 64, 128, dtype=F32)
    assert refused("modconv_dma: grid too large", "dma_conv1", 65536, 8, 32, 64, 128)
    assert refused("modconv_dma: y_scaled goes with out_scale", "dma_conv1", 1, 8, 32, 64, 128, y_scaled=YS)
    assert refused("modconv_dma (f16): unsupported shape / arguments", "dma_conv1", 1, 8, 32, 64, 128, dtype=F16, y_scaled=YS)
    assert ok("dma_conv1", 1, 8, 32, 64, 128, out_scale=OSC, y_scaled=YS) and ok("dma_conv1", 1, 8, 32, 64, 128, out_scale=OSC)
    assert refused("modconv_dma: a sample must stay below 4 GiB", "dma_conv1", 1, 4096, 8192, 64, 128)
    # dma_rgb_fusable: 128 or 256 channels (all of them in one N tile)
    assert ok("dma_conv1", 1, 8, 32, 64, 128, **RGBKW) and ok("dma_conv1", 1, 8, 32, 64, 256, **RGBKW)
    f = "modconv_dma: fused toRGB needs all channels in one N tile"
    assert refused(f, "dma_conv1", 1, 8, 32, 64, 384, **RGBKW) and refused(f, "dma_conv1", 1, 8, 32, 64, 512, **RGBKW)
    assert refused(f, "dma_conv1", 1, 8, 32, 64, 128, **dict(RGBKW, rgb_bias=None))


def test_hires_route():
    u = "modconv_hires: unsupported shape"
    # <32, 32, 1>: tiles of 8 x 32; <64, 64, 1> and <64, 32, 2>: 4 x 32
    assert ok("hires", 1, 8, 32, 32, 32) and refused(u, "hires", 1, 4, 32, 32, 32) and refused(u, "hires", 1, 12, 32, 32, 32)
    assert refused(u, "hires", 1, 8, 16, 32, 32) and refused(u, "hires", 1, 8, 48, 32, 32) and ok("hires", 1, 16, 64, 32, 32)
    assert ok("hires", 1, 4, 32, 64, 64) and ok("hires", 1, 12, 32, 64, 64) and refused(u, "hires", 1, 6, 32, 64, 64)
    assert refused(u, "hires", 1, 4, 33, 64, 64)
    assert ok("hires", 1, 4, 32, 64, 32, up=2) and refused(u, "hires", 1, 2, 32, 64, 32, up=2) and refused(u, "hires", 1, 4, 31, 64, 32, up=2)
    assert refused(u, "hires", 1, 8, 32, 64, 32) and refused(u, "hires", 1, 8, 32, 32, 64) and refused(u, "hires", 1, 8, 32, 32, 32, up=2)
    assert refused(u, "hires", 1, 8, 32, 32, 32, dtype=F32) and ok("hires", 1, 8, 32, 32, 32, dtype=F16)
    assert refused("modconv_hires: a sample must stay below 2 GiB", "hires", 1, 4096, 8192, 32, 32)
    assert refused("modconv_hires: lrelu / linear only", "hires", 1, 8, 32, 32, 32, act=1)
    assert ok("hires", 1, 8, 32, 32, 32, act=0, alpha=7.0)                          # linear: alpha is not read
    assert refused("modconv_hires: needs 0 <= alpha <= 1 and gain > 0", "hires", 1, 8, 32, 32, 32, alpha=1.5)
    assert refused("modconv_hires: needs 0 <= alpha <= 1 and gain > 0", "hires", 1, 8, 32, 32, 32, gain=0.0)
    assert refused("maua_modconv: NULL y", "hires", 1, 8, 32, 32, 32, y=None) and ok("hires", 1, 8, 32, 32, 32, y=None, **RGBKW)
    assert refused("modconv_hires: toRGB fusion is for conv1 layers", "hires", 1, 4, 32, 64, 32, up=2, **RGBKW)
    assert refused("modconv_hires: fused toRGB needs its weights and bias", "hires", 1, 8, 32, 32, 32, **dict(RGBKW, rgb_wmod=None))
    assert refused("modconv_hires: the u8 frame rides on the fused toRGB", "hires", 1, 8, 32, 32, 32, rgb8_out=RGB8)
    assert refused("modconv_hires: fused toRGB without an output", "hires", 1, 8, 32, 32, 32, rgb_skip_f32=1, **RGBKW)
    assert ok("hires", 1, 8, 32, 32, 32, rgb8_out=RGB8, rgb_skip_f32=1, **RGBKW)
    assert refused("maua_modconv: this route reads a dense input", "hires", 1, 8, 32, 32, 32, x_bstride=0)
    assert refused("maua_modconv: this route carries no out_scale / y_scaled", "hires", 1, 8, 32, 32, 32, out_scale=OSC)


def test_upwalk_routes():
    u = "upwalk: unsupported shape"
    # strips of 64 positions, at least two rows
    assert ok("upwalk", 1, 2, 64, 64, 32, up=2) and ok("upwalk", 1, 3, 128, 64, 32, up=2) and refused(u, "upwalk", 1, 1, 64, 64, 32, up=2)
    assert refused(u, "upwalk", 1, 2, 32, 64, 32, up=2) and refused(u, "upwalk", 1, 2, 96, 64, 32, up=2)
    assert refused(u, "upwalk", 1, 2, 64, 64, 32) and refused(u, "upwalk", 1, 2, 64, 32, 32, up=2) and refused(u, "upwalk", 1, 2, 64, 64, 64, up=2)
    assert refused(u, "upwalk", 1, 2, 64, 64, 32, up=2, dtype=F32) and ok("upwalk", 1, 2, 64, 64, 32, up=2, dtype=F16)
    assert refused("upwalk: lrelu / linear only", "upwalk", 1, 2, 64, 64, 32, up=2, act=1)
    assert refused("upwalk: needs 0 <= alpha <= 1 and gain > 0", "upwalk", 1, 2, 64, 64, 32, up=2, alpha=-0.5)
    assert refused("upwalk: features out, no toRGB fusion", "upwalk", 1, 2, 64, 64, 32, up=2, **RGBKW)
    assert refused("upwalk: grid too large", "upwalk", 65536, 2, 64, 64, 32, up=2)
    assert refused("upwalk: a sample must stay below 2 GiB", "upwalk", 1, 2048, 2048, 64, 32, up=2)

    def fused(h, w, Ci=64, Cm=32, dtype=BF16, up_kw={}, **c1_kw):
        c1 = desc(1, 2 * h, 2 * w, Cm, Cm, **RGBKW)
        for k, v in c1_kw.items():
            setattr(c1, k, v)
        return route("fused_walk", 1, h, w, Ci, Cm, up=2, dtype=dtype, d1=c1, **up_kw)

    f = "upwalk_fused: unsupported shapes"
    # any W >= 2 (strips of 126 output columns, the last one narrower), H >= 2
    assert fused(2, 2) == 0 and fused(3, 77) == 0 and fused(2, 64, dtype=F16) == 0
    assert str(fused(1, 64)).startswith(f) and str(fused(2, 1)).startswith(f) and str(fused(2, 64, dtype=F32)).startswith(f)
    assert str(fused(2, 64, Ci=32)).startswith(f) and str(fused(2, 64, Cm=64)).startswith(f)
    assert str(fused(2, 64, H=5)).startswith(f) and str(fused(2, 64, up=2)).startswith(f)
    assert str(fused(2, 64, rgb_out=None)).startswith("upwalk_fused: needs the block's toRGB")
    assert str(fused(2, 64, rgb_skip_f32=1)).startswith("upwalk_fused: no output") and fused(2, 64, rgb_skip_f32=1, rgb8_out=RGB8) == 0
    assert str(fused(2, 64, act=1)).startswith("upwalk_fused: lrelu / linear only")
    assert str(fused(2, 64, up_kw=dict(gain=-1.0))).startswith("upwalk_fused: needs 0 <= alpha <= 1 and gain > 0")
    assert str(fused(2, 64, out_scale=OSC)).startswith("maua_modconv: this route carries no out_scale / y_scaled")
    assert refused("maua_modconv: the fused walk needs the block's conv1", "fused_walk", 1, 2, 64, 64, 32, up=2)


def test_transposed_convolution_routes():
    e = "maua_modconv: the transposed-convolution routes"
    for r in ("tconv2", "tconv_dma", "tconv_fir"):
        assert refused(e + " are up-layers", r, 1, 16, 32, 64, 64)
        assert refused(e + " carry no toRGB / y_scaled", r, 1, 16, 32, 64, 64, up=2, **RGBKW)
        assert ok(r, 1, 16, 32, 64, 64, up=2, out_scale=OSC) and ok(r, 3, 16, 32, 64, 64, up=2, x_bstride=0, noise_bstride=0)
    # tconv2: any grid; channels in whole chunks of 64 bytes
    assert ok("tconv2", 1, 1, 1, 32, 32, up=2) and ok("tconv2", 1, 5, 7, 32, 64, up=2) and ok("tconv2", 1, 4, 4, 16, 32, up=2, dtype=F32)
    c = "tconv2: channel counts must be multiples of 32"
    assert refused(c, "tconv2", 1, 4, 4, 48, 32, up=2) and refused(c, "tconv2", 1, 4, 4, 32, 48, up=2) and refused(c, "tconv2", 1, 4, 4, 24, 32, up=2, dtype=F32)
    assert refused("tconv2: 32-bit offsets", "tconv2", 1, 8192, 8192, 32, 32, up=2)
    assert refused("tconv2: grid too large", "tconv2", 65536, 4, 4, 32, 32, up=2)
    # tconv_dma: tiles of 8 x 32 positions; 2^32-byte samples and weight sets
    u = "tconv_dma: unsupported shape"
    assert ok("tconv_dma", 1, 8, 32, 32, 32, up=2) and refused(u, "tconv_dma", 1, 4, 32, 32, 32, up=2) and refused(u, "tconv_dma", 1, 12, 32, 32, 32, up=2)
    assert refused(u, "tconv_dma", 1, 8, 16, 32, 32, up=2) and refused(u, "tconv_dma", 1, 8, 48, 32, 32, up=2)
    assert refused("tconv_edges: unsupported dtype", "tconv_dma", 1, 8, 32, 32, 32, up=2, dtype=F32) and ok("tconv_dma", 1, 8, 32, 32, 32, up=2, dtype=F16)
    assert ok("tconv_dma", 1, 2048, 2048, 32 * 15, 32, up=2, noise=None) and refused(u, "tconv_dma", 1, 2048, 2048, 512, 32, up=2, noise=None)   # H W Ci 2 < 2^32
    assert ok("tconv_dma", 1, 8, 32, 8192, 8192, up=2) and refused(u, "tconv_dma", 1, 8, 32, 8192, 16384, up=2)                          # 32 Co Ci < 2^32
    assert refused("tconv_edges: Ci % 16, Co % 32", "tconv_dma", 1, 8, 32, 32, 48, up=2)
    assert refused("tconv_dma: channel blocks must split into groups of 8", "tconv_dma", 1, 8, 32, 32, 32 * 9, up=2)
    assert ok("tconv_dma", 1, 8, 32, 32, 32 * 7, up=2) and ok("tconv_dma", 1, 8, 32, 32, 512, up=2)
    assert refused("tconv_edges: grid too large", "tconv_dma", 65536, 8, 32, 32, 32, up=2)
    # tconv_fir: H >= 16, W >= 32, any size from there; the lrelu epilogue only
    u = "tconv_fir: unsupported shape"
    assert ok("tconv_fir", 1, 16, 32, 32, 32, up=2) and ok("tconv_fir", 1, 17, 33, 32, 64, up=2) and ok("tconv_fir", 1, 16, 32, 32, 32, up=2, dtype=F16)
    assert refused(u, "tconv_fir", 1, 15, 32, 32, 32, up=2) and refused(u, "tconv_fir", 1, 16, 31, 32, 32, up=2)
    assert refused(u, "tconv_fir", 1, 16, 32, 48, 32, up=2) and refused(u, "tconv_fir", 1, 16, 32, 32, 32, up=2, dtype=F32)
    assert refused("tconv_fir: lrelu epilogue only", "tconv_fir", 1, 16, 32, 32, 32, up=2, act=0)
    assert refused("tconv_fir: lrelu epilogue only", "tconv_fir", 1, 16, 32, 32, 32, up=2, alpha=2.0)
    assert refused("tconv_fir: noise must be 8-byte aligned", "tconv_fir", 1, 16, 32, 32, 32, up=2, noise=NZ + 4)
    assert refused("tconv_fir: channel blocks must split into groups of 8", "tconv_fir", 1, 16, 32, 32, 32 * 9, up=2)


def test_upfir_pass():
    assert ok("upfir", 1, 1, 1, 32, 8, up=2) and ok("upfir", 2, 5, 7, 32, 40, up=2) and ok("upfir", 1, 3, 3, 32, 4, up=2, dtype=F32)
    c = "upfir_epilogue: Co must be a multiple of the 16-byte piece"
    assert refused(c, "upfir", 1, 4, 4, 32, 12, up=2) and refused(c, "upfir", 1, 4, 4, 32, 6, up=2, dtype=F32)
    assert refused("upfir_epilogue: out_scale must be 16-byte aligned", "upfir", 1, 4, 4, 32, 32, up=2, out_scale=OSC + 8)
    assert refused("upfir_epilogue: d and bias must be 16-byte aligned", "upfir", 1, 4, 4, 32, 32, up=2, d=D + 4)
    assert refused("upfir_epilogue: d and bias must be 16-byte aligned", "upfir", 1, 4, 4, 32, 32, up=2, bias=BIAS + 8)
    assert refused("upfir_epilogue: noise must be 8-byte aligned", "upfir", 1, 4, 4, 32, 32, up=2, noise=NZ + 4)
    assert refused("upfir_epilogue: noise must be 8-byte aligned", "upfir", 1, 4, 4, 32, 32, up=2, noise_bstride=63)
    assert refused("upfir_epilogue: a sample of t must stay below 2 GiB", "upfir", 1, 2048, 2048, 32, 64, up=2)
    assert refused("upfir_epilogue: grid too large", "upfir", 65536, 4, 4, 32, 32, up=2)
    assert refused("maua_modconv: unsupported dtype", "upfir", 1, 4, 4, 32, 32, up=2, dtype=3)
