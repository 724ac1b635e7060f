"""RealESRGAN x4 generator (RRDBNet) on the HIP device vs the oracle's PyTorch-CPU restatement of the published
architecture (first slice).  basicsr / realesrgan are un-vendored: parity unpinned; random-init
weights of the right shapes (there is no network for the released checkpoints)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _psnr(a, b):
    return 10 * torch.log10(1.0 / ((a - b) ** 2).mean().clamp_min(1e-30)).item()


@pytest.mark.parametrize("dt,blocks", [(torch.float32, 2), (torch.bfloat16, 3)])
def test_rrdbnet_matches_oracle(dt, blocks):
    from maua_amd.super import RRDBNet
    from oracle import super as OSR
    net = RRDBNet(num_block=blocks, dtype=dt, generator=torch.Generator().manual_seed(3))
    p = net.state_dict()
    g = torch.Generator().manual_seed(4)
    for k in p:  # non-trivial biases
        if k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p["conv_last.bias"] = torch.full((3,), 0.5)  # keep the output inside (0, 1) so that the clamp is not the whole test
    p["conv_last.weight"] = p["conv_last.weight"] * 0.1
    net.load_state_dict(p)
    x = torch.rand(2, 3, 24, 40, generator=g)
    y = net(x).cpu()
    ref = OSR.rrdbnet(p, x, blocks)
    assert y.shape == ref.shape == (2, 3, 96, 160)
    inside = ((ref > 0) & (ref < 1)).float().mean()
    assert 0.02 < float(ref.std()) and float(inside) > 0.6, (float(ref.std()), float(inside))
    if dt == torch.float32:
        assert float((y - ref).abs().max()) <= 2e-5
    else:
        assert _psnr(y, ref) >= 40.0, _psnr(y, ref)
    # the u8 frame of the same call: round(255 y), HWC
    u8 = torch.empty((2, 96, 160, 3), dtype=torch.uint8, device="cuda")
    y2 = torch.empty_like(y, device="cuda")
    net(x, out=y2, rgb8_out=u8)
    assert torch.equal(y2.cpu(), y)
    want = y.mul(255).round().byte().permute(0, 2, 3, 1)
    assert int((u8.cpu().int() - want.int()).abs().max()) <= (1 if dt == torch.bfloat16 else 0)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_full_depth_rrdbnet_matches_oracle(dt):
    """configs[4]'s generator at its released depth (RealESRGAN_x4plus: 23 RRDB blocks = 345 trunk convolutions) on a
    non-square 96 x 136 image -> 384 x 544, against the oracle (a few seconds of CPU)."""
    from maua_amd.super import RRDBNet
    from oracle import super as OSR
    net = RRDBNet(num_block=23, dtype=dt, generator=torch.Generator().manual_seed(7))
    p = net.state_dict()
    g = torch.Generator().manual_seed(8)
    for k in p:
        if k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p["conv_last.bias"] = torch.full((3,), 0.5)
    p["conv_last.weight"] = p["conv_last.weight"] * 0.1
    net.load_state_dict(p)
    x = torch.rand(1, 3, 96, 136, generator=g)
    y = net(x, clamp=False).cpu()        # the raw output (random weights of this depth leave [0, 1]; RealESRGANer clamps later)
    with torch.no_grad():
        ref = OSR.rrdbnet_raw(p, x, 23)
    assert y.shape == ref.shape == (1, 3, 384, 544) and bool(torch.isfinite(ref).all()) and float(ref.std()) > 1e-3
    scale = float(ref.abs().max())
    if dt == torch.float32:
        assert float((y - ref).abs().max()) <= 1e-4 * scale, float((y - ref).abs().max()) / scale
    else:
        mse = float(((y - ref) ** 2).mean())
        rng = float(ref.max() - ref.min())
        assert 10 * np.log10(rng * rng / mse) >= 38.0, 10 * np.log10(rng * rng / mse)


def test_realesrgan_wrapper_and_render_pipeline():
    """The reference's call shapes (load_model / upscale, realesrgan.py:22-49) and the configs[4] pipeline: StyleGAN2
    frames -> [0,1] -> 4x up-scaler -> u8, per frame on the device.  A missing checkpoint is an error (the reference
    downloads it), not a silent random network."""
    from maua.super.image.models.realesrgan import load_model, upscale
    from maua_amd.stylegan2 import SynthesisNetwork
    with pytest.raises(FileNotFoundError):
        load_model("x4plus-anime")
    with pytest.raises(KeyError):
        load_model("no-such-model", allow_random_init=True)
    model = load_model("x4plus-anime", allow_random_init=True)                       # 6 RRDB blocks, seeded random init
    assert model.model.num_block == 6 and model.pre_pad == 10 and model.tile_size == 0
    net = SynthesisNetwork(64, 64, 3, channel_base=2048, channel_max=64, generator=torch.Generator().manual_seed(0))
    ws = torch.randn(2, net.num_ws, 64, generator=torch.Generator().manual_seed(1))
    frames = net(ws).add(1).div(2).clamp(0, 1)               # [2, 3, 64, 64] in [0, 1]
    outs = list(upscale([f[None] for f in frames], model))
    assert len(outs) == 2 and tuple(outs[0].shape) == (1, 3, 256, 256)
    assert float(outs[0].min()) >= 0.0 and float(outs[0].max()) <= 1.0


@pytest.mark.parametrize("name,tile", [("x4plus-anime", 0), ("x4plus-anime", 24), ("xsx4-animevideo", 0), ("xsx4-animevideo", 20)])
def test_realesrganer_enhance_matches_published_chain(name, tile):
    """RealESRGANer.enhance as the reference calls it - /255, BGR2RGB flip, reflect pre_pad 10 (right, bottom), network on
    the whole image or on tile_pad-padded tiles, crop, clamp, flip back, round - against the oracle's restatement of the
    published code (realesrgan un-vendored: parity unpinned), exact-f32 mode: u8 images differ by at most 1 on <= 0.1 % of
    the values.  The channel flip is folded into the first / last convolution on the device."""
    from maua_amd.super import load_model
    from oracle import super as OSR
    model = load_model(name, dtype=torch.float32, allow_random_init=True, tile=tile)
    p = model.model.state_dict()
    g = torch.Generator().manual_seed(11)
    img = (torch.rand(37, 50, 3, generator=g) * 255).numpy()          # RGB HWC in [0, 255], odd sizes
    got, mode = model.enhance(img)
    assert mode == "RGB" and got.shape == (148, 200, 3) and got.dtype == np.uint8
    if name == "xsx4-animevideo":
        ref_net = lambda x: OSR.srvgg_compact(p, x)
    else:
        ref_net = lambda x: OSR.rrdbnet_raw(p, x, 6)
    want = OSR.realesrganer_enhance(ref_net, img, tile=tile)
    d = np.abs(got.astype(int) - want.astype(int))
    assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (d.max(), (d > 0).mean())
    # the flips matter (a network is not colour-symmetric) and so does the pre-pad
    plain = OSR.realesrganer_enhance(lambda x: ref_net(x[:, [2, 1, 0]])[:, [2, 1, 0]], img, tile=tile)
    assert np.abs(plain.astype(int) - want.astype(int)).max() > 1
    assert np.abs(OSR.realesrganer_enhance(ref_net, img, tile=tile, pre_pad=0).astype(int) - want.astype(int)).max() > 0


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_srvgg_compact_matches_oracle(dt):
    """SRVGGNetCompact ("xsx4-animevideo": 16 convolutions + PReLU, PixelShuffle 4, + nearest base): f32 <= 2e-5, bf16
    PSNR >= 40 dB; on the LDS-direct narrow tiles (64 x 32 k) and on the generic kernel (odd sizes)."""
    from maua_amd.super import SRVGGNetCompact
    from oracle import super as OSR
    net = SRVGGNetCompact(dtype=dt, generator=torch.Generator().manual_seed(4))
    p = net.state_dict()
    assert len(p) == 18 * 2 + 17 and tuple(p["body.34.weight"].shape) == (48, 64, 3, 3)
    for shape in [(2, 3, 16, 32), (1, 3, 21, 19)]:
        x = torch.rand(shape, generator=torch.Generator().manual_seed(5))
        want = OSR.srvgg_compact(p, x)
        got = net(x, clamp=False).cpu()
        if dt == torch.float32:
            assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max()), shape
        else:
            mse = float(((got - want) ** 2).mean())
            rng = float(want.max() - want.min())
            assert 10 * np.log10(rng * rng / mse) >= 40.0, shape
        u8 = torch.empty((shape[0], 4 * shape[2], 4 * shape[3], 3), dtype=torch.uint8, device="cuda")
        net(x, rgb8_out=u8)
        want8 = got.clamp(0, 1).mul(255).round().byte().permute(0, 2, 3, 1)
        assert int((u8.cpu().int() - want8.int()).abs().max()) <= 1


def _srvgg_load_into(net, params):
    """maua_srvgg_load on the module's LIVE handle (load_state_dict would destroy it and build a new one)"""
    import ctypes as C
    from maua_amd import _lib as L
    h = net._handle()
    for k, v in params.items():
        a = np.ascontiguousarray(v.numpy(), dtype=np.float32)
        L.check(L.lib().maua_srvgg_load(h, k.encode(), a.ctypes.data_as(C.c_void_p), C.c_size_t(a.size)))


def test_srvgg_reload_writes_in_place():
    """bf16, num_feat 32 (first layer Ci 3 -> 32, last layer Co 48 -> 64: both padded), B = 1 at 8 x 8: weights A, weights B, weights A
    again loaded into ONE handle back to back.  The third result is the first bit for bit (every load zeroes the prepared buffer and
    rewrites all of it, the staging buffer of one load leaves nothing behind for the next), the second differs."""
    from maua_amd.super import SRVGGNetCompact, init_srvgg_params
    net = SRVGGNetCompact(num_feat=32, num_conv=2, upscale=4, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(11))
    pa = net.state_dict()
    pb = init_srvgg_params(32, 2, 4, torch.Generator().manual_seed(12))
    x = torch.rand(1, 3, 8, 8, generator=torch.Generator().manual_seed(13))
    outs = []
    for p in (pa, pb, pa):
        _srvgg_load_into(net, p)
        outs.append(net(x, clamp=False).cpu())
    assert outs[0].shape == (1, 3, 32, 32) and float(outs[0].std()) > 0
    assert torch.equal(outs[2], outs[0])
    assert not torch.equal(outs[1], outs[0])


def test_srvgg_unit_styles_grow_with_the_batch():
    """float32 at 16 x 16: every convolution on the generic kernel, which reads the handle's unit styles.  One handle at B = 1, 3, 1
    (filled, regrown, kept): each result is a fresh handle's bit for bit."""
    from maua_amd.super import SRVGGNetCompact
    mk = lambda: SRVGGNetCompact(num_feat=32, num_conv=2, upscale=4, dtype=torch.float32, generator=torch.Generator().manual_seed(14))   # noqa: E731
    one = mk()
    for j, B in enumerate((1, 3, 1)):
        x = torch.rand(B, 3, 16, 16, generator=torch.Generator().manual_seed(20 + j))
        got, want = one(x, clamp=False).cpu(), mk()(x, clamp=False).cpu()
        assert float(want.std()) > 0
        assert torch.equal(got, want), f"B = {B} (step {j})"


def test_rrdb_trunk_on_lds_direct_kernel_matches_generic_and_oracle(monkeypatch):
    """bf16, image sizes the LDS-direct kernel takes (H % 8 == 0, W % 32 == 0): every 3x3 convolution of the trunk and the
    up-sampling tail runs on modconv_dma's narrow N tiles (32 / 64 output channels, channel-sliced dense-block operands,
    residual in the copy-out) - against the generic MFMA kernel on the same weights and the fp32 oracle."""
    from maua_amd.super import RRDBNet
    from oracle import super as OSR
    g = torch.Generator().manual_seed(8)
    blocks = 2
    ref_net = RRDBNet(num_block=blocks, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(5))
    p = ref_net.state_dict()
    for k in p:
        if k.endswith(".bias"):
            p[k] = torch.randn(p[k].shape, generator=g) * 0.05
    p["conv_last.bias"] = torch.full((3,), 0.5)
    p["conv_last.weight"] = p["conv_last.weight"] * 0.1
    x = torch.rand(2, 3, 32, 64, generator=g)
    outs = {}
    for mode in ("1", "0"):
        monkeypatch.setenv("MAUA_RRDB_DMA", mode)
        net = RRDBNet(num_block=blocks, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(5))
        net.load_state_dict(p)
        outs[mode] = net(x).cpu()
        del net
    ref = OSR.rrdbnet(p, x, blocks)
    assert outs["1"].shape == ref.shape == (2, 3, 128, 256)
    assert _psnr(outs["1"], ref) >= 40.0 and _psnr(outs["0"], ref) >= 40.0, (_psnr(outs["1"], ref), _psnr(outs["0"], ref))
    assert _psnr(outs["1"], outs["0"]) >= 50.0, _psnr(outs["1"], outs["0"])   # same bf16 operands, residual rounded once more


def test_enhance_frames_equals_enhance_per_frame_on_ragged_sizes():
    """RealESRGANer.enhance_frames (the batched device form configs[4]'s fused pipeline calls) gives, frame by frame, the u8
    image of enhance() - f32 and bf16, on sizes that are no multiple of the LDS-direct kernel's 8 x 32 tile once pre_pad = 10 is
    added (72 + 10 = 82 rows, 96 + 10 = 106 columns: overhanging tiles with masked stores in bf16), whole-image and tiled.  The
    batch changes which tile shapes / split-K routes the convolutions take, i.e. the order of the f32 sums, so values that sit on
    a rounding boundary may land on the other side: exact-f32 mode <= 1 LSB on <= 0.1 % of the values; in bf16 every layer's
    output is rounded, a flipped rounding travels through the 90 layers behind it: PSNR >= 35 dB between the two u8 images (the
    bar bf16 meets against the fp32 oracle is 38 dB).  The bf16 result on such a size agrees the same way with the generic
    kernel's (MAUA_RRDB_DMA=0)."""

    def close8(a, b, frac):
        d = (a.int() - b.int()).abs()
        if frac is not None:
            assert int(d.max()) <= 1 and float((d > 0).float().mean()) <= frac, (int(d.max()), float((d > 0).float().mean()))
        else:
            ps = 10 * np.log10(255.0 ** 2 / max(float((d.float() ** 2).mean()), 1e-12))
            print("bf16 u8 PSNR between two summation orders:", ps)
            assert ps >= 35.0, ps
    import os
    from maua_amd.super import load_model
    g = torch.Generator().manual_seed(5)
    frames = (torch.rand(3, 72, 96, 3, generator=g) * 255).round().byte()
    for dt in (torch.float32, torch.bfloat16):
        for tile in (0, 40):
            model = load_model("x4plus-anime", dtype=dt, allow_random_init=True, tile=tile)
            got = model.enhance_frames(frames.cuda()).cpu()
            assert tuple(got.shape) == (3, 288, 384, 3) and got.dtype == torch.uint8
            for i in range(3):
                want = torch.from_numpy(model.enhance(frames[i].float().numpy())[0])
                close8(got[i], want, 1e-3 if dt == torch.float32 else None)
    # the compact network (SRVGGNetCompact, "xsx4-animevideo") through the same entry
    vgg = load_model("xsx4-animevideo", dtype=torch.float32, allow_random_init=True)
    got = vgg.enhance_frames(frames.cuda()).cpu()
    for i in range(3):
        close8(got[i], torch.from_numpy(vgg.enhance(frames[i].float().numpy())[0]), 1e-3)
    model = load_model("x4plus-anime", dtype=torch.bfloat16, allow_random_init=True)
    a = model.enhance_frames(frames.cuda()).cpu()
    os.environ["MAUA_RRDB_DMA"] = "0"
    try:
        generic = load_model("x4plus-anime", dtype=torch.bfloat16, allow_random_init=True)
        b = generic.enhance_frames(frames.cuda()).cpu()
    finally:
        del os.environ["MAUA_RRDB_DMA"]
    close8(a, b, None)


def test_full_size_upscale_1024_to_4096_u8():
    """configs[4] at its real shape: one 1024^2 StyleGAN2 frame -> RealESRGAN x4plus (23 blocks, bf16) -> 4096^2 u8
    through the product call (enhance_frames: pre_pad 10 -> 1034^2 input, overhanging tiles).  Checked (i) against oracle/super.py
    on a 256 x 256 crop of the INPUT that contains the frame's top-left corner: the network is convolutional, so the crop's output
    equals the full frame's wherever the crop's other borders are further away than the information that reaches a pixel - compared
    on the 512 x 512 output block at the corner, bf16 vs the fp32 oracle: PSNR >= 45 dB (measured 51.4), <= 0.2 % of the u8 values off by
    more than 2 (measured 0.014 %);
    (ii) tiling invariance at full size: enhance_frames with tile = 512 (tile_pad 10) agrees with the whole-image pass away from
    tile seams the same way (PSNR >= 60 dB over the frame, measured 76.8; identical where no seam is within reach is not guaranteed by the
    published tiling either); (iii) the frame is not saturated or constant."""
    from maua_amd.stylegan2 import SynthesisNetwork
    from maua_amd.super import load_model
    from oracle import super as OSR
    G = SynthesisNetwork(512, 1024, 3, dtype=torch.bfloat16, generator=torch.Generator().manual_seed(0))
    ws = torch.randn(1, G.num_ws, 512, generator=torch.Generator().manual_seed(1))
    u8 = torch.empty((1, 1024, 1024, 3), dtype=torch.uint8, device="cuda")
    img = torch.empty((1, 3, 1024, 1024), device="cuda")
    G(ws, out=img, rgb8_out=u8)
    # (a random-init generator's image is heavy-tailed: rescale into the u8 range like the non-saturating test of the render)
    frame = (img[0] / (3 * img.std())).clamp(-1, 1).add(1).mul(127.5).round().byte().permute(1, 2, 0).contiguous()[None]
    assert 20 < float(frame.float().std()) and float(((frame > 0) & (frame < 255)).float().mean()) > 0.9
    model = load_model("x4plus", dtype=torch.bfloat16, allow_random_init=True)
    # a random-init up-scaler saturates its output; the last convolution is rescaled (the image is linear in it) so that the
    # 4096^2 frame sits inside the u8 range: mean 0.5, standard deviation 0.15
    p = model.model.state_dict()
    probe = model.model(frame[:, :128, :128].permute(0, 3, 1, 2).float().div(255).cuda(), clamp=False)
    k = 0.15 / float(probe.std())
    p["conv_last.weight"] = p["conv_last.weight"] * k
    p["conv_last.bias"] = p["conv_last.bias"] * k + (0.5 - k * float(probe.mean()))
    model.model.load_state_dict(p)
    model.model.set_channel_flip(True)
    big = model.enhance_frames(frame)
    assert tuple(big.shape) == (1, 4096, 4096, 3) and big.dtype == torch.uint8
    assert float(big.float().std()) > 5 and float(((big > 0) & (big < 255)).float().mean()) > 0.5

    def psnr8(a, b):
        mse = float(((a.float() - b.float()) ** 2).mean())
        return 10 * np.log10(255.0 ** 2 / max(mse, 1e-12))
    # (i) the corner block against the fp32 oracle on a crop (the crop's right / bottom borders are 128 input pixels from the block)
    crop = frame[0, :256, :256].float().cpu().numpy()
    torch.set_num_threads(min(32, torch.get_num_threads()))
    want = OSR.realesrganer_enhance(lambda x: OSR.rrdbnet_raw(p, x, 23), crop, tile=0, pre_pad=0)   # the far borders are not the frame's
    got = big[0, :512, :512].cpu()
    w = torch.from_numpy(want[:512, :512])
    d = (got.int() - w.int()).abs()
    print("4096^2 corner block vs fp32 oracle: PSNR", psnr8(got, w), "fraction off by > 2 LSB", float((d > 2).float().mean()))
    assert psnr8(got, w) >= 45.0 and float((d > 2).float().mean()) <= 0.002, (psnr8(got, w), float((d > 2).float().mean()))
    # (ii) tiled vs whole image at full size
    tm = load_model("x4plus", dtype=torch.bfloat16, allow_random_init=True, tile=512)
    tm.model.load_state_dict(p)
    tm.model.set_channel_flip(True)
    tiled = tm.enhance_frames(frame)
    print("tiled vs whole image at 4096^2: PSNR", psnr8(tiled, big))
    assert tuple(tiled.shape) == (1, 4096, 4096, 3) and psnr8(tiled, big) >= 60.0, psnr8(tiled, big)
