"""BASELINE configs[3] (second half): guided-diffusion UNet forward + DDIM sampler on the HIP device against
the CPU oracle's restatement of the published algorithm (oracle/diffusion.py; the guided_diffusion submodule is empty in the
reference checkout: PARITY UNPINNED - the oracle and the device agree with each other and with torch's own ops, nothing
here was produced by the reference).  Tolerances: exact-f32 mode <= 2e-5 of the reference's maximum per operator, <= 1e-4
end to end on a small UNet (40+ chained layers); bf16 PSNR >= 40 dB."""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import diffusion as OD

pytestmark = pytest.mark.gpu


def rel(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max()) / max(1e-20, float(b.abs().max()))


def psnr(a, b):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    mse = float(((a - b) ** 2).mean())
    rng = float(b.max() - b.min())
    return 10 * math.log10(rng * rng / max(mse, 1e-30))


def _nhwc(x, dt):
    return x.permute(0, 2, 3, 1).contiguous().to(device="cuda", dtype=dt)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,heads,ch", [(2, 64, 2, 32), (1, 256, 4, 64), (2, 48, 1, 64), (1, 1024, 2, 64), (3, 16, 2, 32)])
def test_attention_matches_legacy_qkv_attention(dt, B, T, heads, ch):
    """QKVAttentionLegacy.forward on [N, 3 * H * C, T] vs maua_attention_legacy on the NHWC form (T not a multiple of 32,
    several key blocks, one and several query tiles)."""
    from maua_amd import _lib as L
    g = torch.Generator().manual_seed(T + heads)
    qkv = torch.randn(B, 3 * heads * ch, T, generator=g)
    if dt == torch.bfloat16:
        qkv = qkv.bfloat16().float()
    q, k, v = qkv.reshape(B * heads, ch * 3, T).split(ch, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale).float(), dim=-1)
    want = torch.einsum("bts,bcs->bct", w, v).reshape(B, -1, T)          # [B, heads * ch, T]
    x = qkv.permute(0, 2, 1).contiguous().to(device="cuda", dtype=dt)        # [B, T, 3 * heads * ch]
    out = torch.empty((B, T, heads * ch), dtype=dt, device="cuda")
    L.check(L.lib().maua_attention_legacy(L.ctx(), L.ptr(x), L.ptr(out), B, T, heads, ch, L.dtype_id(dt)))
    got = out.float().cpu().permute(0, 2, 1)
    assert rel(got, want) <= (2e-5 if dt == torch.float32 else 2e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M,N,K", [(70, 96, 64), (1024, 256, 512), (5, 32, 32), (300, 1536, 512), (65600, 256, 128), (66000, 512, 64), (65537, 256, 192), (70000, 128, 64), (40000, 384, 512)])
def test_linear_nt_matches_torch(dt, M, N, K):
    from maua_amd import _lib as L
    g = torch.Generator().manual_seed(M + N)
    a, w, b, r = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g), \
        torch.randn(M, N, generator=g)
    if dt == torch.bfloat16:
        a, w, r = a.bfloat16().float(), w.bfloat16().float(), r.bfloat16().float()
    want = F.linear(a, w, b) + r
    ad, wd, rd = (t.to(device="cuda", dtype=dt).contiguous() for t in (a, w, r))
    c = torch.empty((M, N), dtype=dt, device="cuda")
    bd = b.cuda()
    L.check(L.lib().maua_linear_nt(L.ctx(), L.ptr(ad), L.ptr(wd), L.ptr(bd), L.ptr(rd), L.ptr(c), C.c_long(M), N, K,
                                   L.dtype_id(dt)))
    assert rel(c, want) <= (1e-5 if dt == torch.float32 else 1e-2)
    L.check(L.lib().maua_linear_nt(L.ctx(), L.ptr(ad), L.ptr(wd), None, None, L.ptr(c), C.c_long(M), N, K, L.dtype_id(dt)))
    assert rel(c, F.linear(a, w)) <= (1e-5 if dt == torch.float32 else 1e-2)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C_,H,W", [(2, 32, 8, 8), (1, 256, 32, 32), (2, 96, 5, 7), (1, 768, 16, 16), (1, 2048, 8, 8)])
def test_group_norm_matches_torch(dt, B, C_, H, W):
    """GroupNorm32 (+ scale-shift, + SiLU) incl. a large mean / small spread input (float64 statistics)."""
    from maua_amd import _lib as L
    g = torch.Generator().manual_seed(C_ + H)
    x = torch.randn(B, C_, H, W, generator=g) * 0.5 + 30.0 * torch.randn(1, C_, 1, 1, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    ss = 0.3 * torch.randn(B, 2 * C_, generator=g)
    if dt == torch.bfloat16:
        x = x.bfloat16().float()
    xd = _nhwc(x, dt)
    y = torch.empty_like(xd)
    gd, bd, ssd = gamma.cuda(), beta.cuda(), ss.cuda()   # (kept alive: the library gets raw pointers)
    for use_ss, silu in ((False, False), (True, True), (False, True)):
        want = F.group_norm(x, 32, gamma, beta, eps=1e-5)
        if use_ss:
            want = want * (1 + ss[:, :C_, None, None]) + ss[:, C_:, None, None]
        if silu:
            want = F.silu(want)
        L.check(L.lib().maua_group_norm_nhwc(L.ctx(), L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(ssd) if use_ss else None,
                                             int(silu), B, H, W, C_, L.dtype_id(dt), L.ptr(y)))
        got = y.float().cpu().permute(0, 3, 1, 2)
        assert rel(got, want) <= (2e-5 if dt == torch.float32 else 1e-2), (use_ss, silu)


SMALL = dict(image_size=64, model_channels=32, num_res_blocks=1, attention_resolutions=(16, 8), channel_mult=(1, 2, 2),
             num_head_channels=32)
WIDE = dict(image_size=64, model_channels=128, num_res_blocks=1, attention_resolutions=(32,), channel_mult=(1, 2),
            num_head_channels=64)


def _build(cfgkw, dt, seed=0):
    from maua_amd.diffusion import UNetModel
    cfg = OD.unet_config(**cfgkw)
    p = OD.init_unet_params(cfg, torch.Generator().manual_seed(seed))
    net = UNetModel(image_size=cfg["image_size"], in_channels=3, model_channels=cfg["model_channels"],
                    out_channels=cfg["out_channels"], num_res_blocks=cfg["num_res_blocks"],
                    attention_resolutions=cfg["attention_ds"], channel_mult=cfg["channel_mult"],
                    num_head_channels=cfg["num_head_channels"], use_scale_shift_norm=True, resblock_updown=True, dtype=dt)
    net.load_state_dict(p)
    return cfg, p, net


@pytest.mark.parametrize("cfgkw,hw", [(SMALL, (64, 64)), (SMALL, (32, 96)), (WIDE, (64, 64))], ids=["small", "small-32x96", "wide"])
def test_unet_forward_matches_oracle(cfgkw, hw):
    """UNetModel.forward (ResBlocks with scale-shift norm and up / down resampling, legacy attention, virtual skip
    concatenation, timestep MLP) against the oracle: f32 <= 1e-4 of the output's maximum, bf16 PSNR >= 40 dB; every
    convolution route (LDS-direct kernel / split-K gather GEMM / generic kernel) gives the same f32 answer."""
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, *hw, generator=g)
    t = torch.tensor([990.0, 120.0])
    cfg, p, net = _build(cfgkw, torch.float32)
    want = OD.unet_forward(p, cfg, x, t)
    got = net(x, t)
    assert rel(got, want) <= 1e-4
    net.set_route(1)
    assert rel(net(x, t), want) <= 1e-4
    net.set_route(0)
    one = net(x[1:], t[1:])                       # a sample does not depend on its batch neighbours
    assert rel(one, want[1:]) <= 1e-4
    _, _, net16 = _build(cfgkw, torch.bfloat16)
    got16 = net16(x, t)
    assert psnr(got16, want) >= 40.0, psnr(got16, want)
    net16.set_route(1)
    assert psnr(net16(x, t), want) >= 40.0
    # GroupNorm statistics from the convolution epilogues' piece sums (the LDS-direct route of the wide network) vs the separate
    # statistics pass: the same f64 statistics up to the f32 rounding of per-tile partial sums
    net16.set_route(0)
    net16.set_option("psum_off", 1)
    sep = net16(x, t)
    net16.set_option("psum_off", 0)
    assert psnr(sep, got16) >= 60.0, psnr(sep, got16)


def test_full_size_unet_matches_oracle():
    """configs[3]'s own network - guided.py:171-190 at image_size 256: 552.8 M parameters, six levels, attention at 32 / 16 / 8,
    18 + 18 blocks - one forward at 256 x 256 against the CPU oracle (5 s of host time): exact-f32 mode <= 2e-4 of the output's
    maximum through ~330 chained layers, bf16 PSNR >= 40 dB, the graph-captured sampler step equal to the eager one."""
    from maua_amd.diffusion import SpacedDiffusion, UNetModel, space_timesteps
    cfg = OD.unet_config()
    p = OD.init_unet_params(cfg, torch.Generator().manual_seed(0))
    assert sum(v.numel() for v in p.values()) == 552_814_086
    g = torch.Generator().manual_seed(4)
    x = torch.randn(1, 3, 256, 256, generator=g)
    t = torch.tensor([470.0])
    with torch.no_grad():
        want = OD.unet_forward(p, cfg, x, t)

    def build(dt):
        net = UNetModel(image_size=256, in_channels=3, model_channels=256, out_channels=6, num_res_blocks=2,
                        attention_resolutions=cfg["attention_ds"], channel_mult=cfg["channel_mult"], num_head_channels=64,
                        use_scale_shift_norm=True, resblock_updown=True, dtype=dt)
        net.load_state_dict(p)
        return net
    net = build(torch.float32)
    got = net(x, t)
    assert rel(got, want) <= 2e-4, rel(got, want)
    # ... and its input gradient (speed "regular", guided.py:250-272: eps = the first three output channels) against torch.autograd
    # through the oracle's full-size network: there and back through ~330 layers each way
    g_out = torch.zeros(1, 6, 256, 256)
    g_out[:, :3] = torch.randn(1, 3, 256, 256, generator=g)
    want_vjp = OD.unet_input_vjp(p, cfg, x, t, g_out)
    net.forward_keep(x, t)
    got_vjp = net.vjp(g_out).cpu()
    l2 = float((got_vjp - want_vjp).norm() / want_vjp.norm())
    print("full-size UNet input gradient, f32: l2", l2, "max", rel(got_vjp, want_vjp))
    assert l2 <= 2e-4 and rel(got_vjp, want_vjp) <= 1e-3, (l2, rel(got_vjp, want_vjp))
    del net
    torch.cuda.empty_cache()
    net16 = build(torch.bfloat16)
    got16 = net16(x, t)
    assert psnr(got16, want) >= 40.0, psnr(got16, want)
    net16.forward_keep(x, t)
    v16 = net16.vjp(g_out).cpu()
    cos16 = float((v16 * want_vjp).sum() / (v16.norm() * want_vjp.norm()))
    print("full-size UNet input gradient, bf16: cosine", cos16, "l2", float((v16 - want_vjp).norm() / want_vjp.norm()))
    assert cos16 >= 0.98, cos16
    # two sampler steps inside the library (hipGraph) == the same two steps issued one by one
    sd = SpacedDiffusion(space_timesteps(1000, "ddim100"), OD.linear_betas(1000), rescale_timesteps=True)
    xa, xb = x.cuda().clone(), x.cuda().clone()
    _, pa = sd.ddim_sample_loop(net16, xa, 60, 2, use_graph=True)
    _, pb = sd.ddim_sample_loop(net16, xb, 60, 2, use_graph=False)
    assert torch.equal(pa, pb) and torch.equal(xa, xb)


def test_default_512_configuration_matches_oracle():
    """guided.py:282's default checkpoint is the 512 x 512 model: seven levels with channel_mult (0.5, 1, 1, 2, 2, 4, 4) (a
    128-channel first level), attention at ds 16 / 32 / 64, 558.0 M parameters.  create_models builds it; one forward on a
    256 x 256 input (the network is convolutional; a quarter of the oracle's CPU time) against the oracle."""
    from maua_amd.diffusion import create_models
    model, diffusion, _ = create_models("uncondImageNet512", "ddim100", allow_random_init=True, dtype=torch.float32,
                                        generator=torch.Generator().manual_seed(0))
    assert model.channel_mult == (0.5, 1, 1, 2, 2, 4, 4) and tuple(model.attention_resolutions) == (16, 32, 64)
    p = {k: v.float() for k, v in model.state_dict().items()}
    assert sum(v.numel() for v in p.values()) == 557_973_638
    cfg = OD.unet_config(image_size=512)
    x = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(1))
    t = torch.tensor([300.0])
    with torch.no_grad():
        want = OD.unet_forward(p, cfg, x, t)
    assert rel(model(x, t), want) <= 2e-4
    del model
    torch.cuda.empty_cache()
    m16, _, _ = create_models("uncondImageNet512", "ddim100", allow_random_init=True, generator=torch.Generator().manual_seed(0))
    assert psnr(m16(x, t), want) >= 40.0


def test_schedule_and_ddim_step_match_oracle():
    """SpacedDiffusion("ddim100") tables, model timesteps, q_sample and one ddim step (with and without a conditioning
    gradient) vs the oracle's float64 / float32 restatement."""
    from maua_amd.diffusion import SpacedDiffusion, space_timesteps
    sch = OD.Schedule(1000, "ddim100", True)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim100"), OD.linear_betas(1000), rescale_timesteps=True)
    assert sd.timestep_map == sch.timestep_map and sd.num_timesteps == 100
    for name in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod"):
        assert np.array_equal(getattr(sd, name), getattr(sch, name)), name
    t = torch.tensor([99, 37, 0])
    assert torch.equal(sd.model_timesteps(t), sch.model_timesteps(t))
    assert space_timesteps(1000, "100") == OD.space_timesteps(1000, "100") and len(space_timesteps(1000, "10,15,20")) == 45
    g = torch.Generator().manual_seed(5)
    x0, nz = torch.randn(3, 3, 16, 16, generator=g), torch.randn(3, 3, 16, 16, generator=g)
    assert rel(sd.q_sample(x0, t, nz), OD.q_sample(sch, x0, t, nz)) <= 1e-6
    mo, grad = torch.randn(3, 6, 16, 16, generator=g), 0.1 * torch.randn(3, 3, 16, 16, generator=g)

    class Fixed:
        def __call__(self, x, ts):
            return mo.cuda()
    for gr in (None, grad):
        out = sd.ddim_sample(Fixed(), x0, t, cond_fn=None if gr is None else (lambda x, ts: gr.cuda()))
        ws, wp = OD.ddim_step(sch, mo, x0, t, gr)
        assert rel(out["sample"], ws) <= 2e-6 and rel(out["pred_xstart"], wp) <= 2e-6


def test_p_and_plms_samplers_match_oracle():
    """guided.py:302-311: the "p" (ancestral, learned-range variance, condition_mean) and "plms" (pseudo linear multistep,
    orders 1-4, improved-Euler start, condition_score) samplers, step by step against the oracle's restatements with a
    fixed-output model, then "plms" / "p" chains on a small UNet through GuidedDiffusion."""
    from maua_amd.diffusion import GuidedDiffusion, SpacedDiffusion, space_timesteps
    sch = OD.Schedule(1000, "50", True)
    sd = SpacedDiffusion(space_timesteps(1000, "50"), OD.linear_betas(1000), rescale_timesteps=True)
    for name in ("posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2"):
        assert np.array_equal(getattr(sd, name), getattr(sch, name)), name
    g = torch.Generator().manual_seed(11)
    t = torch.tensor([49, 20, 0])
    x, nz = torch.randn(3, 3, 16, 16, generator=g), torch.randn(3, 3, 16, 16, generator=g)
    grad = 0.1 * torch.randn(3, 3, 16, 16, generator=g)
    outs = {}

    def model_cpu(xx, tt):     # a deterministic "network": a per-step pattern + a linear function of its input
        key = tuple(int(v) for v in torch.as_tensor(tt).reshape(-1))
        if key not in outs:
            gg = torch.Generator().manual_seed(sum((i + 1) * (v + 7) for i, v in enumerate(key)))
            outs[key] = torch.randn(xx.shape[0], 6, 16, 16, generator=gg) * 0.7
        return outs[key] + 0.1 * torch.cat([xx, -xx], 1)

    class Dev:
        def __call__(self, xx, ts):
            idx = torch.tensor([sch.timestep_map.index(int(round(float(v) * sch.original_num_steps / 1000.0))) for v in ts.cpu()])
            return model_cpu(xx.cpu(), idx).cuda()
    for gr in (None, grad):
        cond = None if gr is None else (lambda xx, ts: gr.cuda())
        out = sd.p_sample(Dev(), x, t, cond_fn=cond, noise=nz)
        ws, wp = OD.p_sample_step(sch, model_cpu(x, t), x, t, nz, gr)
        assert rel(out["sample"], ws) <= 3e-6 and rel(out["pred_xstart"], wp) <= 2e-6
    # plms: chains of five steps at every order (t stays > 0 except for the last sample of the batch at order 1)
    for order in (1, 2, 3, 4):
        for gr in (None, grad):
            cond_d = None if gr is None else (lambda xx, ts: gr.cuda())
            cond_o = None if gr is None else (lambda xx, ts: gr)
            tt, xd, xo, od, oo = torch.tensor([30, 12, 6]), x.clone(), x.clone(), None, None
            for step in range(5):
                od = sd.plms_sample(Dev(), xd, tt, cond_fn=cond_d, order=order, old_out=od)
                oo = OD.plms_sample(sch, model_cpu, xo, tt, cond_fn=cond_o, order=order, old_out=oo)
                assert len(od["old_eps"]) == len(oo["old_eps"])
                assert rel(od["sample"], oo["sample"]) <= 2e-5 and rel(od["pred_xstart"], oo["pred_xstart"]) <= 2e-5, (order, step)
                xd, xo, tt = od["sample"], oo["sample"].clone(), tt - 1
    # through GuidedDiffusion on a small UNet (exact-f32 mode): "plms" order 2 and "p" against the oracle's chain
    cfg, p, net = _build(SMALL, torch.float32)
    sch2 = OD.Schedule(1000, "20", True)
    sd2 = SpacedDiffusion(space_timesteps(1000, "20"), OD.linear_betas(1000), rescale_timesteps=True)
    img, nz2 = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    gd = GuidedDiffusion([], sampler="plms", timesteps=20, model=net, diffusion=sd2, plms_order=2)
    got = gd.forward(img, [], 0.4, t_end=0.7, noise=nz2)            # start_step 8, 6 steps
    tt = torch.tensor([8, 8])
    xo, oo = OD.q_sample(sch2, img, tt, nz2), None
    fn = lambda xx, t_: OD.unet_forward(p, cfg, xx, sch2.model_timesteps(t_))
    with torch.no_grad():
        for _ in range(6):
            oo = OD.plms_sample(sch2, fn, xo, tt, order=2, old_out=oo)
            xo, tt = oo["sample"], tt - 1
    assert rel(got, oo["pred_xstart"]) <= 5e-4
    with pytest.raises(NotImplementedError):
        GuidedDiffusion([], sampler="euler", timesteps=20, model=net, diffusion=sd2)


def test_guided_diffusion_forward_and_sampler_loop():
    """GuidedDiffusion.forward with the reference's start / step arithmetic on a small UNet: the in-library loop (one
    hipGraph), the eager step-by-step path and the oracle agree; a conditioning gradient (speed="hyper") changes the
    result the way the oracle says."""
    from maua_amd.diffusion import GuidedDiffusion, ImageTarget, MSEGuide, SpacedDiffusion, space_timesteps
    cfg, p, net = _build(SMALL, torch.float32)
    sch = OD.Schedule(1000, "ddim20", True)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    g = torch.Generator().manual_seed(9)
    img, nz = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    gd = GuidedDiffusion([], timesteps=20, model=net, diffusion=sd)
    want = OD.guided_diffusion_forward(p, cfg, sch, img, 0.3, noise=nz)          # start_step 6, 13 steps: t = 6 .. -6
    got = gd.forward(img, [], 0.3, noise=nz)
    assert rel(got, want) <= 5e-4          # 13 chained network evaluations
    again = gd.forward(img, [], 0.3, noise=nz)                                    # graph replay
    assert torch.equal(got, again)
    assert net.graph_active(), "the sampler loop did not capture into a hipGraph"
    x = sd.q_sample(img, torch.tensor([6, 6]), nz)
    eager = sd.ddim_sample_loop(net, x.clone(), 6, 13, use_graph=False)[1]
    assert torch.equal(eager, got)
    # conditioning
    target = torch.randn(3, 64, 64, generator=g).clamp(-1, 1)
    guide = MSEGuide(scale=500.0)
    gdc = GuidedDiffusion([guide], timesteps=20, model=net, diffusion=sd, speed="hyper")

    def cond_fn(x, ts):   # the oracle's restatement of guided.py:238-274 with speed "hyper"
        idx = torch.tensor([sch.timestep_map.index(int(v)) for v in ts.long()])
        a = torch.from_numpy(sch.sqrt_alphas_cumprod).float()[idx].reshape(-1, 1, 1, 1)
        s = torch.from_numpy(sch.sqrt_one_minus_alphas_cumprod).float()[idx].reshape(-1, 1, 1, 1)
        est = (x - s * nz) / a
        return -(2.0 * 500.0 / est[0].numel()) * (est - target) / a
    want_c = OD.guided_diffusion_forward(p, cfg, sch, img, 0.3, t_end=0.6, noise=nz, cond_fn=cond_fn)
    got_c = gdc.forward(img, [ImageTarget(target)], 0.3, t_end=0.6, noise=nz)
    assert rel(got_c, want_c) <= 5e-4
    assert rel(got_c, OD.guided_diffusion_forward(p, cfg, sch, img, 0.3, t_end=0.6, noise=nz)) > 1e-3   # the gradient matters


def test_onset_prompt_schedule_and_sample():
    """configs[3]'s audio coupling: the active prompt advances at the onset peaks of the clip (bit-exact onset bins of the
    render path), frames with the same prompt share a sampler batch; frames are reproducible from the seed."""
    from maua_amd import audio as A
    from maua_amd.diffusion import ImageTarget, MSEGuide, SpacedDiffusion, onset_prompt_schedule, sample, space_timesteps
    from maua_amd.pipeline import synthetic_audio
    from oracle import audio as OA, signal as OSG
    fps, n = 30, 48
    wav = synthetic_audio(n * 1024, 1024 * fps, seed=2)
    idx = onset_prompt_schedule(wav, 1024 * fps, fps, 3)
    env = OA.onsets(wav, 1024 * fps).squeeze(-1)
    thr = OSG.percentile(env, 90)
    peak = torch.zeros(n, dtype=torch.bool)
    peak[1:-1] = (env[1:-1] > env[:-2]) & (env[1:-1] >= env[2:]) & (env[1:-1] > thr)
    assert idx.dtype == torch.int64 and torch.equal(idx, torch.cumsum(peak.long(), 0) % 3) and int(idx.max()) >= 1
    cfg, p, net = _build(SMALL, torch.bfloat16)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim5"), OD.linear_betas(1000), rescale_timesteps=True)
    g = torch.Generator().manual_seed(1)
    prompts = [ImageTarget(torch.randn(3, 64, 64, generator=g).clamp(-1, 1)) for _ in range(3)]
    a, ia = sample(prompts, wav, 1024 * fps, fps, n_frames=6, size=(64, 64), timesteps=5, model=net, diffusion=sd,
                   grad_modules=[MSEGuide(100.0)], seed=4)
    b, _ = sample(prompts, wav, 1024 * fps, fps, n_frames=6, size=(64, 64), timesteps=5, model=net, diffusion=sd,
                  grad_modules=[MSEGuide(100.0)], seed=4)
    assert tuple(a.shape) == (6, 3, 64, 64) and torch.equal(ia, idx[:6]) and torch.equal(a, b) and bool(torch.isfinite(a).all())
    # a frame's x0 / noise draws do not depend on how the frames were batched: another batch size gives the same frames up
    # to the kernels' batch-dependent summation order
    c, _ = sample(prompts, wav, 1024 * fps, fps, n_frames=6, size=(64, 64), timesteps=5, model=net, diffusion=sd,
                  grad_modules=[MSEGuide(100.0)], seed=4, batch=2)
    assert float((a - c).abs().max()) <= 0.05 * float(a.abs().max())


# ------------------------------------------------------------------------------------------------ secondary model / "fast" guidance
def _secondary(dt, seed, exact=True):
    from maua_amd.diffusion import SecondaryDiffusionImageNet2
    net = SecondaryDiffusionImageNet2(dtype=dt, exact=exact)
    p = OD.secondary_random_params(seed)
    net.load_state_dict(p, strict=True)       # the reference's own state-dict keys (pinned by g28's strict load into its class)
    return net, p


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_secondary_model_forward_matches_the_reference_fixture(golden, dt):
    """SecondaryDiffusionImageNet2.forward on the device against g28 = the outputs of the REFERENCE's class (guided.py:68-143) on the
    same weights (64 x 96 input: every level has a non-square grid, the bottleneck is 2 x 3).  exact-f32 mode <= 1e-4 of the
    output's maximum over 24 chained convolutions, bf16 PSNR >= 40 dB."""
    g = golden("g28_secondary")
    net, _ = _secondary(dt, int(g["seed"]))
    out = net(g["x"], g["t"])
    for got, want in ((out.v, g["v"]), (out.pred, g["pred"]), (out.eps, g["eps"])):
        if dt == torch.float32:
            assert rel(got, want) <= 1e-4
        else:
            assert psnr(got, want) >= 40.0
    if dt == torch.float32:   # MAUA_F32_SPLIT (three bf16 split products per product, ~2^-17 each): the same bar over the 24-layer chain
        split, _ = _secondary(dt, int(g["seed"]), exact=False)
        out = split(g["x"], g["t"])
        for got, want in ((out.v, g["v"]), (out.pred, g["pred"]), (out.eps, g["eps"])):
            print("split-f32 secondary forward vs the reference:", rel(got, want))
            assert rel(got, want) <= 1e-4


def test_secondary_model_vjp_matches_autograd_on_the_oracle():
    """maua_secondary_vjp = (d v / d x)^T g evaluated on the transposed network against torch.autograd on the restatement (which
    g28 pins to the reference): random upstream gradient, two shapes, exact-f32 <= 2e-4; and a second vjp on the same forward state
    gives the same answer (the stored activations are not consumed); bf16 cosine similarity >= 0.99 (measured 0.997: ReLU masks
    of activations within a bf16 ulp of zero flip)."""
    from maua_amd.diffusion import SecondaryDiffusionImageNet2
    p = OD.secondary_random_params(3)
    for (B, H, W) in ((1, 32, 32), (2, 64, 96)):
        g = torch.Generator().manual_seed(H + W)
        x, t, gv = torch.randn(B, 3, H, W, generator=g), torch.rand(B, generator=g), torch.randn(B, 3, H, W, generator=g)
        with torch.enable_grad():
            xx = x.clone().requires_grad_()
            v = OD.secondary_forward(p, xx, t)[0]
            want = torch.autograd.grad(v, xx, gv)[0]
        for dt in (torch.float32, torch.bfloat16):
            net = SecondaryDiffusionImageNet2(dtype=dt)
            net.load_state_dict(p)
            net(x, t)
            got = net.vjp(gv).cpu()
            if dt == torch.float32:
                assert rel(got, want) <= 2e-4, (B, H, W, rel(got, want))
                assert torch.equal(net.vjp(gv).cpu(), got)
            else:
                cos = float((got * want).sum() / (got.norm() * want.norm()))
                assert cos >= 0.99, (B, H, W, cos)
    with pytest.raises(Exception):
        net.vjp(torch.zeros(1, 3, 32, 32))     # not the shape of the last forward


@pytest.mark.parametrize("dt,exact", [(torch.float32, False), (torch.bfloat16, True)])
def test_secondary_reload_writes_in_place(dt, exact):
    """MAUA_F32_SPLIT and bf16, B = 1 at 32 x 32 (first layer Ci 19 -> 32, last layer Co 3 -> 32: both padded): weights A, weights B,
    weights A again loaded into ONE handle back to back (maua_secondary_load on the live handle), forward and vjp after each.  The
    third v and gradient are the first bit for bit - every load zeroes both prepared buffers and rewrites them whole (the forward's
    and the transposed network's, split again where the dtype asks), and one load's staging leaves nothing for the next - and
    the second differ."""
    from maua_amd import _lib as L
    from maua_amd.diffusion import SecondaryDiffusionImageNet2
    pa, pb = OD.secondary_random_params(21), OD.secondary_random_params(22)
    net = SecondaryDiffusionImageNet2(dtype=dt, exact=exact)
    net.load_state_dict(pa)
    g = torch.Generator().manual_seed(23)
    x, t, gv = torch.randn(1, 3, 32, 32, generator=g), torch.rand(1, generator=g), torch.randn(1, 3, 32, 32, generator=g)

    def load(p):
        h = net._handle()
        for i, k in enumerate(net._keys):
            for what, a in ((0, p[k + ".weight"]), (1, p[k + ".bias"])):
                a = a.contiguous().float()
                L.check(L.lib().maua_secondary_load(h, i, what, C.c_void_p(a.data_ptr()), C.c_size_t(a.numel())))

    outs = []
    for p in (pa, pb, pa):
        load(p)
        outs.append((net(x, t).v.cpu(), net.vjp(gv).cpu()))
    for k in range(2):
        assert float(outs[0][k].std()) > 0
        assert torch.equal(outs[2][k], outs[0][k]), k
        assert not torch.equal(outs[1][k], outs[0][k]), k


def test_fast_conditioning_matches_the_reference_gradient(golden):
    """GradientGuidedConditioning(speed="fast") - the reference's default - against g28's cond_grad, which the REFERENCE's own
    GradientGuidedConditioning.forward computed with torch.autograd through its secondary model (guided.py:236-272): same weights,
    same x_t, same timesteps, an MSE grad module of the same scale.  48 chained convolutions (forward + transposed network): the
    exact-f32 mode lands at 4e-4 of the gradient's norm, 1.6e-3 of its maximum; the DEFAULT of create_models / GuidedDiffusion - float32
    tensors with every product as three bf16 split products on the bf16 matrix cores (MAUA_F32_SPLIT, ~2^-17 per product) - must meet
    the same bars; bf16 3.5 % of the norm (bar 7 %)."""
    from maua_amd.diffusion import GradientGuidedConditioning, ImageTarget, MSEGuide, SpacedDiffusion, space_timesteps
    g = golden("g28_secondary")
    sd = SpacedDiffusion(space_timesteps(1000, "ddim100"), OD.linear_betas(1000), rescale_timesteps=True)
    for dt, exact, tol_l2, tol_max in ((torch.float32, True, 1e-3, 5e-3), (torch.float32, False, 1e-3, 5e-3), (torch.bfloat16, True, 7e-2, 0.25)):
        net, _ = _secondary(dt, int(g["seed"]), exact)
        guide = MSEGuide(scale=float(g["mse_scale"]))
        cond = GradientGuidedConditioning(sd, net, [guide], speed="fast")
        cond.set_targets([ImageTarget(g["target"])], torch.zeros_like(g["xt"]))
        got = cond(g["xt"], g["t_model"]).cpu()
        want = g["cond_grad"]
        l2 = float((got - want).norm() / want.norm())
        print("fast conditioning vs the reference's gradient", dt, "exact" if exact else "split", "l2", l2, "max", rel(got, want))
        assert l2 <= tol_l2 and rel(got, want) <= tol_max, (dt, l2, rel(got, want))


def test_guided_diffusion_reference_defaults_and_grad_module_contract():
    """GuidedDiffusion with the reference's DEFAULT arguments (sampler "ddim", speed "fast": guided.py:277-288) runs end to end with
    a stand-in perceptor that follows maua/grad.py:15-25's contract on the device (scale / set_targets(prompts) / __call__(img, t)
    -> d loss / d img): the module sees device images of the sampler's shape and the respaced model timesteps, a zero-scale module
    is dropped (:299), the guided result differs from the unguided one and moves TOWARDS the module's target, and the "fast" and
    "hyper" speeds agree on the direction of the first step's gradient."""
    from maua_amd.diffusion import GuidedDiffusion, SpacedDiffusion, SecondaryDiffusionImageNet2, space_timesteps
    cfg, p, net = _build(SMALL, torch.float32)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    sec = SecondaryDiffusionImageNet2(dtype=torch.float32)
    sec.load_state_dict(OD.secondary_random_params(1))
    calls = []

    class StandInPerceptor:    # "CLIPGrads" shaped: a fixed random linear embedding of the image, pulled towards the prompt's embedding
        def __init__(self, scale):
            self.scale = scale
            self.proj = torch.randn(16, 3 * 64 * 64, generator=torch.Generator().manual_seed(3)).cuda() / 110.0
            self.target = None

        def set_targets(self, prompts):
            self.target = torch.stack([pr.embedding for pr in prompts]).mean(0).cuda()

        def __call__(self, img, t):
            assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape[1:]) == (3, 64, 64)
            calls.append([int(v) for v in t])
            e = img.reshape(img.shape[0], -1) @ self.proj.T                    # the "perceptor"
            return (self.scale * 2.0 * (e - self.target) @ self.proj).reshape(img.shape)

    class Prompt:
        def __init__(self, emb):
            self.embedding = emb

        def to(self, *_a, **_k):
            return self
    g = torch.Generator().manual_seed(4)
    img, nz = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    emb = torch.randn(16, generator=g)
    per, off = StandInPerceptor(0.05), StandInPerceptor(0.0)
    gd = GuidedDiffusion([per, off], timesteps=20, model=net, diffusion=sd, secondary_model=sec)     # defaults: ddim, speed="fast"
    assert gd.conditioning.speed == "fast" and gd.conditioning.grad_modules == [per]
    guided = gd.forward(img, [Prompt(emb)], 0.3, t_end=0.6, noise=nz)
    plain = GuidedDiffusion([], timesteps=20, model=net, diffusion=sd).forward(img, [], 0.3, t_end=0.6, noise=nz)
    assert torch.isfinite(guided).all() and len(calls) == 6 and all(len(c) == 2 for c in calls)
    assert all(c[0] in sd.timestep_map for c in calls) and calls[0][0] > calls[-1][0]      # model timesteps, descending
    dist = lambda im: float(((im.reshape(2, -1) @ per.proj.T) - per.target).norm())
    assert dist(guided) < dist(plain)
    fast = gd.conditioning(sd.q_sample(img, torch.tensor([6, 6]), nz), torch.tensor([float(sd.timestep_map[6])] * 2))
    hyp = GuidedDiffusion([per], timesteps=20, model=net, diffusion=sd, speed="hyper")
    hyp.conditioning.set_targets([Prompt(emb)], L_dev(nz))
    hg = hyp.conditioning(sd.q_sample(img, torch.tensor([6, 6]), nz), torch.tensor([float(sd.timestep_map[6])] * 2))
    cos = float((fast * hg).sum() / (fast.norm() * hg.norm()))
    assert cos > 0.0, cos


@pytest.mark.parametrize("sec_dt,sec_exact", [(torch.float32, True), (torch.float32, False), (torch.bfloat16, True)],
                         ids=["f32-secondary", "split-f32-secondary", "bf16-secondary"])
def test_guided_loop_as_one_graph_equals_the_step_by_step_loop(sec_dt, sec_exact):
    """Round 5: configs[3]'s GUIDED loop - UNet forward, secondary forward, image-MSE grad module, secondary VJP,
    DDIM update per step (guided.py:236-272, 302-311, 333-337) - inside the library as one hipGraph (maua_ddim_guided_loop) against
    the step-by-step path that calls the same operators from Python (ddim_sample + GradientGuidedConditioning.forward): identical
    bits.  One capture serves other targets and scales; per-sample targets; a NaN target means "no guidance" (:262-265)."""
    from maua_amd.diffusion import (GuidedDiffusion, ImageTarget, MSEGuide, SecondaryDiffusionImageNet2, SpacedDiffusion,
                                    space_timesteps)
    cfg, p, net = _build(SMALL, torch.float32)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    sec = SecondaryDiffusionImageNet2(dtype=sec_dt, exact=sec_exact)
    sec.load_state_dict(OD.secondary_random_params(1))
    g = torch.Generator().manual_seed(11)
    img, nz = torch.randn(2, 3, 64, 64, generator=g), torch.randn(2, 3, 64, 64, generator=g)
    t1, t2 = (torch.randn(3, 64, 64, generator=g).clamp(-1, 1) for _ in range(2))
    guide = MSEGuide(scale=800.0)
    gd = GuidedDiffusion([guide], timesteps=20, model=net, diffusion=sd, secondary_model=sec)
    assert gd.conditioning.speed == "fast"
    res = {}
    for tgt, name in ((t1, "a"), (t2, "b")):
        gd.use_graph = True
        res[name] = gd.forward(img, [ImageTarget(tgt)], 0.3, t_end=0.8, noise=nz)      # start_step 6, 10 steps
        assert net.guided_graph_active(), "the guided loop did not capture into a hipGraph"
        gd.use_graph = False
        assert torch.equal(res[name], gd.forward(img, [ImageTarget(tgt)], 0.3, t_end=0.8, noise=nz)), name
    assert not torch.equal(res["a"], res["b"])
    plain = GuidedDiffusion([], timesteps=20, model=net, diffusion=sd).forward(img, [], 0.3, t_end=0.8, noise=nz)
    assert rel(res["a"], plain) > 1e-4                                                  # the guidance acts
    # another scale through the same capture
    guide.scale = 100.0
    gd.use_graph = True
    r100 = gd.forward(img, [ImageTarget(t1)], 0.3, t_end=0.8, noise=nz)
    gd.use_graph = False
    assert torch.equal(r100, gd.forward(img, [ImageTarget(t1)], 0.3, t_end=0.8, noise=nz)) and not torch.equal(r100, res["a"])
    # one target per sample (the operator and the loop take a [B, C, H, W] target)
    guide.target = torch.stack([t1, t2]).cuda()
    x = sd.q_sample(img, torch.tensor([6, 6]), nz)
    gd.conditioning.noise = None
    per = sd.ddim_guided_loop(net, gd.conditioning, x.clone(), 6, 10)[1]
    xs, t = x.clone(), torch.tensor([6, 6])
    for _ in range(10):
        o = sd.ddim_sample(net, xs, t, cond_fn=gd.conditioning)
        xs, t = o["sample"], t - 1
    assert torch.equal(per, o["pred_xstart"])
    # a grad module whose output holds a NaN contributes nothing: the loop equals the unguided one
    guide.scale = 800.0
    bad = t1.clone()
    bad[1, 5, 7] = float("nan")
    gd.use_graph = True
    nan_g = gd.forward(img, [ImageTarget(bad)], 0.3, t_end=0.8, noise=nz)
    gd.use_graph = False
    assert torch.equal(nan_g, gd.forward(img, [ImageTarget(bad)], 0.3, t_end=0.8, noise=nz))
    # (a zero gradient still takes condition_score's eps -> pred round trip: equal to the unguided loop up to that rounding)
    assert bool(torch.isfinite(nan_g).all()) and rel(nan_g, plain) <= 1e-5 and rel(res["a"], plain) > 100 * rel(nan_g, plain)
    # the guidance branch runs BESIDE the UNet forward (a parallel branch of the graph / a side stream); behind it (option
    # "guided_fork" = 0: one stream, a new capture) the loop gives the same bits, as a graph and launch by launch
    guide.target = t1.cuda()
    net.set_option("guided_fork", 0)
    for use_graph in (True, False):
        gd.use_graph = use_graph
        assert torch.equal(res["a"], gd.forward(img, [ImageTarget(t1)], 0.3, t_end=0.8, noise=nz)), use_graph
    net.set_option("guided_fork", 1)
    gd.use_graph = True
    assert torch.equal(res["a"], gd.forward(img, [ImageTarget(t1)], 0.3, t_end=0.8, noise=nz)) and net.guided_graph_active()
    # before any forward the secondary model has nothing to differentiate
    with pytest.raises(RuntimeError):
        SecondaryDiffusionImageNet2(dtype=torch.float32).vjp(torch.zeros(1, 3, 64, 64))


def test_both_sampler_graphs_on_one_network_are_dropped_and_recaptured_together():
    """One network carries both captured loops (maua_ddim_sample_loop's and maua_ddim_guided_loop's executables, csrc/sampler.hip).  A
    larger batch regrows the arena and the per-step tables they point into: both are dropped and captured again; back at the first
    batch likewise.  At every stage each loop - unguided, guided speed "fast" (secondary model, image-MSE target) and speed "regular"
    (through the network itself) - replays a graph and gives the bits of the same loop run launch by launch.  32 x 32 is the smallest
    legal size (three levels, attention still at 8 x 8); equality only, so no tolerance."""
    from maua_amd.diffusion import GradientGuidedConditioning, ImageTarget, MSEGuide, SpacedDiffusion, space_timesteps
    cfg, p, net = _build(SMALL, torch.float32)
    net.enable_vjp()                                   # (before the weights load: the library object is created on first use)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    sec, _ = _secondary(torch.float32, 1)
    g = torch.Generator().manual_seed(23)
    target = torch.randn(3, 32, 32, generator=g).clamp(-1, 1)
    fast = GradientGuidedConditioning(sd, sec, [MSEGuide(scale=800.0)], speed="fast")
    regular = GradientGuidedConditioning(sd, net, [MSEGuide(scale=800.0)], speed="regular")
    for cond in (fast, regular):
        cond.set_targets([ImageTarget(target)], None)
    loops = {"unguided": (lambda x, ug: sd.ddim_sample_loop(net, x, 6, 4, use_graph=ug), net.graph_active),
             "fast": (lambda x, ug: sd.ddim_guided_loop(net, fast, x, 6, 4, use_graph=ug), net.guided_graph_active),
             "regular": (lambda x, ug: sd.ddim_guided_loop(net, regular, x, 6, 4, use_graph=ug), net.guided_graph_active)}
    xs = {B: torch.randn(B, 3, 32, 32, generator=g) for B in (1, 3)}
    for stage, B in enumerate((1, 3, 1)):
        for name, (loop, active) in loops.items():
            sample, pred = loop(xs[B].clone(), True)
            assert active(), (stage, B, name)
            sample_e, pred_e = loop(xs[B].clone(), False)
            assert torch.equal(sample, sample_e) and torch.equal(pred, pred_e), (stage, B, name)


def L_dev(t):
    from maua_amd import _lib as L
    return L.dev_tensor(t, torch.float32)


def test_full_size_100_step_ddim_bf16_drift_and_onset_switched_sampling():
    """configs[3] at its real size: the 552.8 M-parameter UNet at 256 x 256.
    (i) the WHOLE 100-step DDIM loop (guided.py:333-337, one hipGraph) in bf16 against the same loop in exact-f32 mode from the same
    x_T and weights: the per-step rounding noise of bf16 does not grow without bound over 100 chained network evaluations -
    PSNR(pred_xstart bf16, f32) >= 50 dB after 10, 50 and 100 steps (measured 71.3 / 73.1 / 73.1 dB: the loop contracts the
    rounding noise rather than accumulating it), everything finite.  (ii) ``sample()`` at 256 x 256 with the reference's default "fast" guidance (secondary model) and an
    onset-switched prompt schedule: the prompt index follows the clip's onset peaks, the run is reproducible from its seed, and
    the ACTIVE prompt is the one that acts: replacing the second prompt changes exactly the frames behind the first switch (a
    random-init UNet is no denoiser, so "moves towards the target" is not testable here; "which frames react to which prompt" is)."""
    from maua_amd.diffusion import (ImageTarget, MSEGuide, SecondaryDiffusionImageNet2, SpacedDiffusion, UNetModel,
                                    onset_prompt_schedule, sample, space_timesteps)
    from maua_amd.pipeline import synthetic_audio
    cfg = OD.unet_config()
    p = OD.init_unet_params(cfg, torch.Generator().manual_seed(0))

    def build(dt):
        net = UNetModel(image_size=256, in_channels=3, model_channels=256, out_channels=6, num_res_blocks=2,
                        attention_resolutions=cfg["attention_ds"], channel_mult=cfg["channel_mult"], num_head_channels=64,
                        use_scale_shift_norm=True, resblock_updown=True, dtype=dt)
        net.load_state_dict(p)
        return net
    sd = SpacedDiffusion(space_timesteps(1000, "ddim100"), OD.linear_betas(1000), rescale_timesteps=True)
    xT = torch.randn(1, 3, 256, 256, generator=torch.Generator().manual_seed(8)).cuda()
    preds = {}
    for dt in (torch.float32, torch.bfloat16):
        net = build(dt)
        for n in (10, 50, 100):
            x = xT.clone()
            _, pred = sd.ddim_sample_loop(net, x, 99, n)
            assert bool(torch.isfinite(pred).all()) and bool(torch.isfinite(x).all())
            preds[(dt, n)] = pred.cpu()
        if dt == torch.float32:
            del net
            torch.cuda.empty_cache()
    drift = {n: psnr(preds[(torch.bfloat16, n)], preds[(torch.float32, n)]) for n in (10, 50, 100)}
    print("bf16 vs f32 pred_xstart PSNR after 10 / 50 / 100 DDIM steps:", drift)
    assert min(drift.values()) >= 50.0, drift
    # (ii) onset-switched sampling with the default guidance speed, bf16 network from (i)
    fps, n = 30, 48
    wav = synthetic_audio(n * 1024, 1024 * fps, seed=2)
    idx = onset_prompt_schedule(wav, 1024 * fps, fps, 2)
    first_switch = int((idx != idx[0]).nonzero()[0])
    lo = max(0, first_switch - 2)
    g = torch.Generator().manual_seed(1)
    prompts = [ImageTarget(torch.randn(3, 256, 256, generator=g).clamp(-1, 1) * 0.5 + s) for s in (-0.4, 0.4)]
    sec = SecondaryDiffusionImageNet2(dtype=torch.bfloat16)
    sec.load_state_dict(OD.secondary_random_params(2))
    sd8 = SpacedDiffusion(space_timesteps(1000, "ddim8"), OD.linear_betas(1000), rescale_timesteps=True)
    kw = dict(n_frames=first_switch + 2, size=(256, 256), timesteps=8, model=net, diffusion=sd8, grad_modules=[MSEGuide(2000.0)],
              seed=4, batch=2, speed="fast", secondary_model=sec)
    a, ia = sample(prompts, wav, 1024 * fps, fps, **kw)
    b, _ = sample(prompts, wav, 1024 * fps, fps, **kw)
    assert tuple(a.shape) == (first_switch + 2, 3, 256, 256) and torch.equal(ia, idx[:first_switch + 2]) and torch.equal(a, b)
    assert bool(torch.isfinite(a).all())
    other = [prompts[0], ImageTarget(-prompts[1].target)] if int(idx[0]) == 0 else [ImageTarget(-prompts[0].target), prompts[1]]
    c, _ = sample(other, wav, 1024 * fps, fps, **kw)
    same = [bool(torch.equal(a[f], c[f])) for f in range(first_switch + 2)]
    assert all(same[:first_switch]) and not any(same[first_switch:]), same

# ------------------------------------------------------------------------------------ speed "regular": the UNet's input gradient
@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,C_,H,W", [(2, 32, 8, 8), (1, 256, 16, 16), (2, 96, 6, 10), (1, 1024, 8, 8)])
def test_group_norm_input_gradient_matches_autograd(dt, B, C_, H, W):
    """maua_group_norm_nhwc_vjp against torch.autograd through GroupNorm32 -> [scale-shift] -> [SiLU] -> [avg_pool 2 | nearest x2]
    (ResBlock.in_layers + h_upd, out_layers, AttentionBlock.norm), with and without the residual branch's gradient (x_upd / the
    identity skip) joining at the input.  f32: <= 5e-5 of the gradient's maximum; bf16 (x, dy and dx rounded): <= 2e-2."""
    from maua_amd import _lib as L
    g = torch.Generator().manual_seed(C_ + H)
    x = torch.randn(B, C_, H, W, generator=g) * 0.7 + 2.0 * torch.randn(1, C_, 1, 1, generator=g)
    gamma, beta = 1 + 0.1 * torch.randn(C_, generator=g), 0.1 * torch.randn(C_, generator=g)
    ss = 0.3 * torch.randn(B, 2 * C_, generator=g)
    if dt == torch.bfloat16:
        x = x.bfloat16().float()
    xd = _nhwc(x, dt)
    gd, bd, ssd = gamma.cuda(), beta.cuda(), ss.cuda()
    resample = {0: (lambda t: t), 1: (lambda t: F.avg_pool2d(t, 2, 2)), 2: (lambda t: F.interpolate(t, scale_factor=2, mode="nearest"))}
    for use_ss, silu, mode, with_res in ((False, False, 0, True), (True, True, 0, False), (False, True, 1, True), (False, True, 2, True),
                                         (True, False, 2, False)):
        xx = x.clone().requires_grad_()
        y = F.group_norm(xx, 32, gamma, beta, eps=1e-5)
        if use_ss:
            y = y * (1 + ss[:, :C_, None, None]) + ss[:, C_:, None, None]
        if silu:
            y = F.silu(y)
        y = resample[mode](y)
        dy = torch.randn(y.shape, generator=g)
        dres = torch.randn(y.shape, generator=g) if with_res else None
        if dt == torch.bfloat16:
            dy = dy.bfloat16().float()
            dres = dres.bfloat16().float() if with_res else None
        total = (y * dy).sum() + ((resample[mode](xx) * dres).sum() if with_res else 0.0)
        want = torch.autograd.grad(total, xx)[0]
        dyd = _nhwc(dy, dt)
        drd = _nhwc(dres, dt) if with_res else None
        dx = torch.empty_like(xd)
        L.check(L.lib().maua_group_norm_nhwc_vjp(L.ctx(), L.ptr(xd), L.ptr(gd), L.ptr(bd), L.ptr(ssd) if use_ss else None, int(silu), mode,
                                                 L.ptr(dyd), L.ptr(drd) if with_res else None, B, H, W, C_, L.dtype_id(dt), L.ptr(dx)))
        got = dx.float().cpu().permute(0, 3, 1, 2)
        assert rel(got, want) <= (5e-5 if dt == torch.float32 else 2e-2), (use_ss, silu, mode, with_res, rel(got, want))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("B,T,heads,ch", [(2, 64, 2, 32), (1, 256, 4, 64), (2, 48, 1, 64), (1, 1024, 2, 64), (3, 16, 2, 32), (1, 200, 2, 64)])
def test_attention_input_gradient_matches_autograd(dt, B, T, heads, ch):
    """maua_attention_legacy_vjp against torch.autograd through QKVAttentionLegacy.forward (T not a multiple of 32 or of the
    128-row tile, one and several blocks on both sides).  P and dS are rebuilt from the forward's log-sum-exp rows; in bf16 they are
    rounded before the second products, like the forward rounds P."""
    from maua_amd import _lib as L
    g = torch.Generator().manual_seed(T + 3 * heads)
    qkv = torch.randn(B, 3 * heads * ch, T, generator=g)
    d_out = torch.randn(B, heads * ch, T, generator=g)
    if dt == torch.bfloat16:
        qkv, d_out = qkv.bfloat16().float(), d_out.bfloat16().float()
    qq = qkv.clone().requires_grad_()
    q, k, v = qq.reshape(B * heads, ch * 3, T).split(ch, dim=1)
    scale = 1 / math.sqrt(math.sqrt(ch))
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * scale, k * scale).float(), dim=-1)
    a = torch.einsum("bts,bcs->bct", w, v).reshape(B, -1, T)
    want = torch.autograd.grad(a, qq, d_out)[0]                                   # [B, 3 * heads * ch, T]
    x = qkv.permute(0, 2, 1).contiguous().to(device="cuda", dtype=dt)
    dod = d_out.permute(0, 2, 1).contiguous().to(device="cuda", dtype=dt)
    dq = torch.empty_like(x)
    L.check(L.lib().maua_attention_legacy_vjp(L.ctx(), L.ptr(x), L.ptr(dod), L.ptr(dq), B, T, heads, ch, L.dtype_id(dt)))
    got = dq.float().cpu().permute(0, 2, 1)
    assert rel(got, want) <= (5e-5 if dt == torch.float32 else 3e-2), rel(got, want)


@pytest.mark.parametrize("cfgkw,hw", [(SMALL, (64, 64)), (SMALL, (32, 96)), (WIDE, (64, 64))], ids=["small", "small-32x96", "wide"])
def test_unet_input_gradient_matches_autograd_on_the_oracle(cfgkw, hw):
    """UNetModel.forward_keep + vjp (maua_unet_forward_keep / maua_unet_vjp: the network walked backwards inside the library - transposed
    MFMA convolutions and GEMMs, GroupNorm / SiLU / resampling and attention input-gradient kernels, the skip connections' two
    consumers added up) against torch.autograd.grad through the oracle's UNet - what guided.py:268 computes for speed "regular".
    f32: <= 2e-4 of the gradient's maximum over the whole 40-layer chain there and back; bf16: cosine >= 0.99, L2 <= 12 %.  The kept
    forward returns what the plain forward returns; a vjp without its forward is refused."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, *hw, generator=g)
    t = torch.tensor([870.0, 240.0])
    cfg, p, net = _build(cfgkw, torch.float32)
    g_out = torch.randn(2, cfg["out_channels"], *hw, generator=g)
    want = OD.unet_input_vjp(p, cfg, x, t, g_out)
    plain = net(x, t)
    with pytest.raises(RuntimeError):
        net.vjp(g_out)
    kept = net.forward_keep(x, t)
    assert torch.equal(kept, net(x, t)) and rel(kept, plain) <= 1e-6
    net.forward_keep(x, t)
    got = net.vjp(g_out)
    assert rel(got, want) <= 2e-4, rel(got, want)
    again = net.vjp(g_out)                             # the kept tensors are read, not consumed
    assert torch.equal(got, again)
    net.forward_keep(x[1:], t[1:])                     # a sample's gradient does not depend on its batch neighbours
    assert rel(net.vjp(g_out[1:]), want[1:]) <= 2e-4
    net.set_route(1)                                   # ... nor on the convolution route
    net.forward_keep(x, t)
    assert rel(net.vjp(g_out), want) <= 2e-4
    _, _, net16 = _build(cfgkw, torch.bfloat16)
    net16.forward_keep(x, t)
    got16 = net16.vjp(g_out).cpu()
    cos = float((got16 * want).sum() / (got16.norm() * want.norm()))
    l2 = float((got16 - want).norm() / want.norm())
    print("bf16 UNet input gradient vs f32 autograd: cosine", cos, "l2", l2)
    assert cos >= 0.99 and l2 <= 0.12, (cos, l2)


def test_regular_speed_conditioning_matches_the_reference_class_fixture(golden):
    """g32 = the gradient the REFERENCE's own GradientGuidedConditioning.forward computed for speed "regular" (its timestep mapping,
    img mix, grad-module sum, sign and torch.autograd.grad around the restated network: tests/golden/make_golden.py regular) against
    GradientGuidedConditioning(speed="regular") here - UNetModel.forward_keep + vjp behind the C ABI.  f32 network: 2e-4 in L2."""
    from maua_amd.diffusion import GradientGuidedConditioning, ImageTarget, MSEGuide, SpacedDiffusion, space_timesteps
    g = golden("g32_regular_conditioning")
    assert int(g["unet_seed"]) == 0
    cfg, p, net = _build(SMALL, torch.float32, seed=0)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    guide = MSEGuide(scale=float(g["mse_scale"]))
    cond = GradientGuidedConditioning(sd, net, [guide], speed="regular")
    cond.set_targets([ImageTarget(g["target"])], torch.zeros_like(g["xt"]))
    got = cond(g["xt"], g["t_model"]).cpu()
    want = g["cond_grad"]
    l2 = float((got - want).norm() / want.norm())
    print("regular conditioning vs the reference class's gradient: l2", l2, "max", rel(got, want))
    assert l2 <= 2e-4 and rel(got, want) <= 5e-4, (l2, rel(got, want))
    _, _, net16 = _build(SMALL, torch.bfloat16, seed=0)
    cond16 = GradientGuidedConditioning(sd, net16, [guide], speed="regular")
    cond16.set_targets([ImageTarget(g["target"])], torch.zeros_like(g["xt"]))
    got16 = cond16(g["xt"], g["t_model"]).cpu()
    cos = float((got16 * want).sum() / (got16.norm() * want.norm()))
    print("  bf16 network: cosine", cos)
    assert cos >= 0.99, cos


def test_regular_speed_conditioning_matches_the_oracle_and_guides_the_sampler():
    """GradientGuidedConditioning(speed="regular") - guided.py:214-218, :250-252: the loss gradient through p_mean_variance's
    pred_xstart, i.e. through the diffusion UNet - against oracle.diffusion.regular_conditioning (torch autograd on the restated
    network and schedule); GuidedDiffusion(speed="regular") then runs the DDIM loop with it and moves the result towards the target."""
    from maua_amd.diffusion import GradientGuidedConditioning, GuidedDiffusion, ImageTarget, MSEGuide, SpacedDiffusion, space_timesteps
    cfg, p, net = _build(SMALL, torch.float32)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim20"), OD.linear_betas(1000), rescale_timesteps=True)
    sch = OD.Schedule(1000, "ddim20")
    g = torch.Generator().manual_seed(9)
    img, nz, target = (torch.randn(2, 3, 64, 64, generator=g) for _ in range(3))
    xt = OD.q_sample(sch, img, torch.tensor([12, 5]), nz)
    t_model = torch.tensor([float(sd.timestep_map[12]), float(sd.timestep_map[5])])
    guide = MSEGuide(scale=500.0)
    cond = GradientGuidedConditioning(sd, net, [guide], speed="regular")
    cond.set_targets([ImageTarget(target)], torch.zeros_like(xt))
    got = cond(xt, t_model).cpu()
    k = guide.factor(target[0].numel())
    want = OD.regular_conditioning(p, cfg, sch, lambda im, _t: k * (im - target), xt, t_model)
    l2 = float((got - want).norm() / want.norm())
    print("regular conditioning vs oracle autograd: l2", l2, "max", rel(got, want))
    assert l2 <= 2e-4 and rel(got, want) <= 5e-4, (l2, rel(got, want))
    gd = GuidedDiffusion([MSEGuide(scale=2000.0)], timesteps=20, model=net, diffusion=sd, speed="regular")
    assert gd.conditioning.speed == "regular"
    guided = gd.forward(img, [ImageTarget(target)], 0.3, t_end=0.6, noise=nz).cpu()
    # that ran inside the library as ONE hipGraph (maua_ddim_guided_loop without a secondary model: kept forward, img, grad module,
    # input gradient, DDIM update per step) ...
    assert gd.conditioning.graphable() and net.guided_graph_active()
    plain = GuidedDiffusion([], timesteps=20, model=net, diffusion=sd).forward(img, [], 0.3, t_end=0.6, noise=nz).cpu()
    assert torch.isfinite(guided).all()
    assert float((guided - target).norm()) < float((plain - target).norm())
    # ... launch by launch from Python (ddim_sample + the conditioning) it gives the same bits
    gd.use_graph = False
    stepwise = gd.forward(img, [ImageTarget(target)], 0.3, t_end=0.6, noise=nz).cpu()
    assert torch.equal(stepwise, guided)
    # the sampler hands its own (kept) evaluation of the network to the conditioning; the reference evaluates it twice per step
    # (guided.py:251 inside cond_fn): the same bits either way
    sd._model_output = lambda model, x, mt, cond_fn: model(x, mt)
    twice = gd.forward(img, [ImageTarget(target)], 0.3, t_end=0.6, noise=nz).cpu()      # (use_graph is still False: the Python loop)
    del sd._model_output
    assert torch.equal(twice, guided)
    # the other two samplers of guided.py:302-311 take the same conditioning (plms evaluates the model - and cond_fn - twice in its first step)
    for sampler in ("plms", "p"):
        sdk = SpacedDiffusion(space_timesteps(1000, "20"), OD.linear_betas(1000), rescale_timesteps=True)
        gk = GuidedDiffusion([MSEGuide(scale=2000.0)], sampler=sampler, timesteps=20, model=net, diffusion=sdk, speed="regular")
        torch.manual_seed(3)
        a = gk.forward(img, [ImageTarget(target)], 0.3, t_end=0.6, noise=nz).cpu()
        sdk._model_output = lambda model, x, mt, cond_fn: model(x, mt)
        torch.manual_seed(3)
        b = gk.forward(img, [ImageTarget(target)], 0.3, t_end=0.6, noise=nz).cpu()
        assert torch.isfinite(a).all() and torch.equal(a, b), sampler


def test_full_size_unet_samples_across_batch_sizes():
    """The 552.8 M-parameter UNet at 256 x 256: a sample's output alone and inside a batch of 16.  NOT bit-identical - the UNet's kernels are
    chosen by workgroup count (LDS-direct or gather convolution, the gather kernel's K slices), so the summation order differs with the
    batch - but equal to bf16 rounding: PSNR >= 50 dB (measured: see the printed value), unlike the synthesis network, whose frames are
    bit-identical wherever they are rendered (tests/test_gpu_synth.py)."""
    from maua_amd.diffusion import create_models
    model, _, _ = create_models("uncondImageNet256", "ddim20", allow_random_init=True, generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(16, 3, 256, 256, generator=g).cuda()
    t = torch.tensor([900.0, 700.0, 500.0, 300.0] * 4).cuda()
    big = model(x, t).clone()
    assert bool(torch.isfinite(big).all())
    for k in (0, 5, 15):
        one = model(x[k:k + 1].contiguous(), t[k:k + 1].contiguous())[0]
        print("sample", k, "alone vs in a batch of 16: PSNR", psnr(one, big[k]), "dB, max rel", rel(one, big[k]))
        assert psnr(one, big[k]) >= 50.0, k
    assert torch.equal(model(x, t), big)                      # the same batch again: the same bits
