"""CLIP's text tower on the device: the causal attention kernel (maua_attention_causal), the tower (maua_clip_text_*) against a CPU
restatement of CLIP's published ``encode_text`` (float32, torch.nn.MultiheadAttention under build_attention_mask - parity with CLIP
itself is unpinned: no vocabulary, no checkpoint), causality and batch independence bit for bit, the host checks, the string cache,
and text prompts through CLIPGrads and the onset-switched sampler."""
import gzip

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from maua_amd import _lib as L  # noqa: E402
from maua_amd import clip as CL  # noqa: E402


def rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-30)


def cos(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu().reshape(-1), torch.as_tensor(b).detach().double().cpu().reshape(-1)
    return float((a @ b) / (a.norm() * b.norm()).clamp_min(1e-300))


# ------------------------------------------------------------------------------------------------ causal attention
def causal_attention_ref(qkv, B, T, heads, hc):
    """softmax(Q K^T / sqrt(hc) + triu(-inf, 1)) V in float64, legacy layout: channel = head * 3 hc + {q | k | v} * hc + c."""
    x = qkv.double().cpu().reshape(B, T, heads, 3, hc)
    q, k, v = x[:, :, :, 0].transpose(1, 2), x[:, :, :, 1].transpose(1, 2), x[:, :, :, 2].transpose(1, 2)   # [B][heads][T][hc]
    s = q @ k.transpose(-1, -2) / hc ** 0.5 + torch.full((T, T), float("-inf"), dtype=torch.float64).triu(1)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, T, heads * hc)


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("hc", [32, 64])
@pytest.mark.parametrize("T", [1, 31, 77, 129, 300])
def test_causal_attention_matches_masked_softmax(dt, hc, T):
    B, heads = 2, 3
    g = torch.Generator().manual_seed(T * 100 + hc)
    qkv = (2.0 * torch.randn(B, T, heads * 3 * hc, generator=g)).to(dt).cuda()
    out = torch.full((B, T, heads * hc), float("nan"), dtype=dt, device="cuda")
    L.check(L.lib().maua_attention_causal(L.ctx(), L.ptr(qkv), L.ptr(out), B, T, heads, hc, L.dtype_id(dt)))
    torch.cuda.synchronize()
    want = causal_attention_ref(qkv, B, T, heads, hc)
    if dt == torch.float32:
        assert rel(out, want) <= 1e-5
        # query 0 sees key 0 only: its output is V row 0 of its head, exactly
        v0 = qkv.reshape(B, T, heads, 3, hc)[:, 0, :, 2].reshape(B, heads * hc)
        assert torch.equal(out[:, 0], v0)
    else:
        assert cos(out, want) >= 0.9999
    # the mask matters (beyond the first query)
    if T > 1:
        full = torch.empty_like(out)
        L.check(L.lib().maua_attention_legacy(L.ctx(), L.ptr(qkv), L.ptr(full), B, T, heads, hc, L.dtype_id(dt)))
        torch.cuda.synchronize()
        assert not torch.equal(full[:, 1:], out[:, 1:])


# ------------------------------------------------------------------------------------------------ the tower
def text_params(cfg, seed):
    """CLIP's initialisation (TextTransformer's), with LayerNorm gains / biases and the block biases drawn too so they count."""
    g = torch.Generator().manual_seed(seed)
    p = CL.TextTransformer(*cfg, generator=g).state_dict()
    for k in p:
        if k.endswith(("ln_1.weight", "ln_2.weight", "ln_final.weight")):
            p[k] = 1.0 + 0.1 * torch.randn(p[k].shape, generator=g)
        elif k.endswith("bias"):
            p[k] = 0.02 * torch.randn(p[k].shape, generator=g)
    return p


def encode_text_ref(p, cfg, tokens):
    """clip/model.py CLIP.encode_text restated in float32 on the CPU: token embedding + positional embedding, ResidualAttentionBlocks
    (nn.MultiheadAttention with build_attention_mask(), LayerNorm, c_fc, QuickGELU, c_proj), ln_final, the EOT row
    (argmax of the ids) @ text_projection."""
    ctx, vocab, w, layers, heads, E = cfg
    tokens = tokens.long().cpu()
    with torch.no_grad():
        x = p["token_embedding.weight"][tokens] + p["positional_embedding"]
        mask = torch.empty(ctx, ctx).fill_(float("-inf")).triu_(1)
        x = x.permute(1, 0, 2)   # NLD -> LND
        for i in range(layers):
            b = f"transformer.resblocks.{i}."
            mha = torch.nn.MultiheadAttention(w, heads)
            mha.in_proj_weight.copy_(p[b + "attn.in_proj_weight"])
            mha.in_proj_bias.copy_(p[b + "attn.in_proj_bias"])
            mha.out_proj.weight.copy_(p[b + "attn.out_proj.weight"])
            mha.out_proj.bias.copy_(p[b + "attn.out_proj.bias"])
            h = F.layer_norm(x, (w,), p[b + "ln_1.weight"], p[b + "ln_1.bias"], 1e-5)
            x = x + mha(h, h, h, need_weights=False, attn_mask=mask)[0]
            h = F.layer_norm(x, (w,), p[b + "ln_2.weight"], p[b + "ln_2.bias"], 1e-5)
            h = F.linear(h, p[b + "mlp.c_fc.weight"], p[b + "mlp.c_fc.bias"])
            h = h * torch.sigmoid(1.702 * h)
            x = x + F.linear(h, p[b + "mlp.c_proj.weight"], p[b + "mlp.c_proj.bias"])
        x = F.layer_norm(x.permute(1, 0, 2), (w,), p["ln_final.weight"], p["ln_final.bias"], 1e-5)
        return x[torch.arange(x.shape[0]), tokens.argmax(dim=-1)] @ p["text_projection"]


def make_tokens(cfg, eots, seed):
    """Rows sot .. eot with the eot (the largest id, vocab - 1) at the given positions; ids after it are zero padding."""
    ctx, vocab = cfg[0], cfg[1]
    g = torch.Generator().manual_seed(seed)
    t = torch.zeros(len(eots), ctx, dtype=torch.int32)
    for r, e in enumerate(eots):
        t[r, 0] = vocab - 2
        t[r, 1:e] = torch.randint(1, vocab - 2, (max(e - 1, 0),), generator=g, dtype=torch.int32)
        t[r, e] = vocab - 1
    return t


def tower(cfg, dt, p):
    tt = CL.TextTransformer(*cfg, dtype=dt)
    tt.load_state_dict(p)
    return tt


SMALL_CFGS = [(77, 600, 64, 2, 2, 32), (77, 700, 128, 2, 2, 48), (40, 600, 128, 2, 4, 64)]
B16 = CL.TEXT_CONFIGS["ViT-B/16"]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("cfg", SMALL_CFGS + [B16], ids=["w64h32", "w128h64", "ctx40w128h32", "ViT-B16"])
def test_text_tower_matches_the_restatement(cfg, dt):
    p = text_params(cfg, seed=cfg[2] + cfg[0])
    tt = tower(cfg, dt, p)
    ctx = cfg[0]
    for eots in ([5], [ctx - 1, 3, 17, 1, ctx // 2]):
        tokens = make_tokens(cfg, eots, seed=len(eots))
        got = tt(tokens)
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(eots), cfg[5]) and got.is_cuda
        want = encode_text_ref(p, cfg, tokens)
        if dt == torch.float32:
            assert rel(got, want) <= 1e-4
        else:
            assert cos(got, want) >= 0.999
        # int64 host tokens and int32 device tokens give the same bits
        assert torch.equal(tt(tokens.long()), tt(tokens.cuda()))


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
def test_text_tower_causality_and_batch_independence(dt):
    cfg = (77, 600, 64, 2, 2, 32)
    tt = tower(cfg, dt, text_params(cfg, 5))
    tokens = make_tokens(cfg, [7, 76, 30, 2, 51], seed=3)
    base = tt(tokens)
    # ids after a row's eot do not reach its embedding (they stay below the eot id, so argmax is unchanged)
    after = tokens.clone()
    g = torch.Generator().manual_seed(11)
    for r, e in enumerate([7, 76, 30, 2, 51]):
        after[r, e + 1:] = torch.randint(1, 598, (76 - e,), generator=g, dtype=torch.int32)
    assert not torch.equal(after, tokens)
    assert torch.equal(tt(after), base)
    # an id before the eot does
    before = tokens.clone()
    before[2, 10] = (before[2, 10] + 1) % 598 + 1
    got = tt(before)
    assert not torch.equal(got[2], base[2]) and torch.equal(got[[0, 1, 3, 4]], base[[0, 1, 3, 4]])
    # the rows of a batch are independent: a permutation of the rows permutes the embeddings bit for bit
    perm = torch.tensor([3, 0, 4, 2, 1])
    assert torch.equal(tt(tokens[perm]), base[perm])
    assert torch.equal(tt(tokens[1:2]), base[1:2])


def test_bad_tokens_are_value_errors_before_any_launch():
    cfg = (77, 600, 64, 2, 2, 32)
    tt = tower(cfg, torch.bfloat16, text_params(cfg, 1))
    for bad in (torch.full((2, 77), 600, dtype=torch.int32), torch.full((2, 77), 600, dtype=torch.int32).cuda(),
                torch.full((1, 77), -3, dtype=torch.int64), torch.zeros(1, 76, dtype=torch.int32), torch.zeros(2, 40, dtype=torch.int32).cuda(),
                torch.zeros(77, dtype=torch.int32)):
        with pytest.raises(ValueError):
            tt(bad)
    assert tt._h is None   # nothing was created on the device, let alone launched
    ok = make_tokens(cfg, [4], 0)
    assert bool(torch.isfinite(tt(ok)).all()) and tt._h is not None


# ------------------------------------------------------------------------------------------------ strings, the cache, CLIPGrads
MERGES = ["h e", "l l", "he ll", "hell o</w>", "t h", "th e</w>", "c i", "ci t", "cit y</w>", "f r", "fr a", "fra c"]


@pytest.fixture
def vocab(tmp_path):
    path = tmp_path / "merges.txt.gz"
    path.write_bytes(gzip.compress(("#version: synthetic\n" + "\n".join(MERGES) + "\n").encode()))
    return str(path)


SMALL_VIT = dict(input_resolution=32, patch_size=8, width=64, layers=2, heads=2, output_dim=32)
TEXT_SMALL = (77, 600, 64, 2, 2, 32)   # (the synthetic vocabulary has 526 entries)


def small_model(dt=torch.bfloat16, seed=2):
    from oracle import clip as OC
    vt = CL.VisionTransformer(*SMALL_VIT.values(), dtype=dt)
    vt.load_state_dict(OC.init_vit_params(SMALL_VIT, torch.Generator().manual_seed(seed)), strict=True)
    return CL.CLIPImageModel(vt, text=tower(TEXT_SMALL, dt, text_params(TEXT_SMALL, seed)))


def test_string_prompts_go_through_the_cache(vocab, monkeypatch):
    m = small_model()
    m.bpe_path = vocab
    texts = ["a fractal city", "hello the city", "a fractal city"]
    tokens = CL.tokenize(texts, truncate=True, bpe_path=vocab)
    want = m.text(tokens)
    calls = []
    fwd = m.text.forward
    monkeypatch.setattr(m.text, "forward", lambda t: calls.append(t.shape[0]) or fwd(t))
    first = m.encode_text(texts)
    assert calls == [2] and torch.equal(first, want)          # the repeated string runs once
    second = m.encode_text(texts[:2])
    assert calls == [2] and torch.equal(second, want[:2])     # nothing new: the tower does not run
    assert torch.equal(m.encode_text("hello the city"), want[1:2])
    m.text.load_state_dict(m.text.state_dict())               # new weights (here: the same) invalidate the cache
    assert torch.equal(m.encode_text(texts[:1]), want[:1]) and calls == [2, 1]
    # tokens go straight to the tower, as clip's encode_text takes them
    assert torch.equal(m.encode_text(tokens[:2]), want[:2]) and calls == [2, 1, 2]


def test_clip_grads_text_prompts_equal_their_embeddings(vocab):
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt, TextPrompt
    m = small_model()
    a, b = "a fractal city", "hello the city"
    gm = CLIPGrads(scale=50.0, clip_models=[m], cutout_kwargs=dict(cutn=8), cutout_batches=2, bpe_path=vocab)
    assert m.bpe_path == vocab
    gm.set_targets([TextPrompt(a, 1.0), TextPrompt(b, 3.0)])
    emb = m.encode_text(CL.tokenize([a, b], truncate=True, bpe_path=vocab)).cpu()
    assert torch.equal(gm.targets[0][0], emb) and torch.equal(gm.weights[0], torch.tensor([0.25, 0.75]))
    ref = CLIPGrads(scale=50.0, clip_models=[small_model()], cutout_kwargs=dict(cutn=8), cutout_batches=2)
    ref.set_targets([EmbeddingPrompt(emb[0], 1.0), EmbeddingPrompt(emb[1], 3.0)])
    g = torch.Generator().manual_seed(4)
    img = (torch.rand(2, 3, 48, 48, generator=g) * 2 - 1).cuda()
    t = torch.tensor([400, 400])
    torch.manual_seed(7)
    got = gm(img, t)
    torch.manual_seed(7)
    want = ref(img, t)
    assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0 and torch.equal(got, want)


def test_onset_switched_text_prompts_through_the_sampler(vocab, monkeypatch):
    """configs[3] as written: sample([TextPrompt(a), TextPrompt(b)], audio) with CLIPGrads built by get_diffusion_model(clip_kwargs=...)
    - the frames equal the same call with the prompts' embeddings, the prompt per frame follows the onsets, and the captured loop
    equals the step-by-step one."""
    from maua_amd.diffusion import (GuidedDiffusion, SecondaryDiffusionImageNet2, SpacedDiffusion, UNetModel, get_diffusion_model,
                                    onset_prompt_schedule, sample, space_timesteps)
    from maua_amd.grad import CLIPGrads, EmbeddingPrompt, TextPrompt
    from maua_amd.pipeline import synthetic_audio
    from oracle import diffusion as OD
    fps = 30
    wav = synthetic_audio(48 * 1024, 1024 * fps, seed=2)
    idx = onset_prompt_schedule(wav, 1024 * fps, fps, 2)
    switch = int((idx != idx[0]).nonzero()[0])            # the first frame after a prompt switch
    n_frames = switch + 2
    g = torch.Generator().manual_seed(3)
    net = UNetModel(image_size=64, in_channels=3, model_channels=32, out_channels=6, num_res_blocks=1, attention_resolutions=(4, 8),
                    channel_mult=(1, 2, 2), num_head_channels=32, use_scale_shift_norm=True, resblock_updown=True, dtype=torch.bfloat16,
                    generator=g)
    sec = SecondaryDiffusionImageNet2(dtype=torch.float32, generator=g, exact=False)
    sd = SpacedDiffusion(space_timesteps(1000, "ddim4"), OD.linear_betas(1000), rescale_timesteps=True)
    m = small_model()
    clip_kwargs = dict(clip_models=[m], bpe_path=vocab, cutout_kwargs=dict(cutn=8), cutout_batches=1, clamp_gradient=0.05)
    gdm = get_diffusion_model(timesteps=4, sampler="ddim", clip_scale=500.0,
                              guided_kwargs=dict(model=net, diffusion=sd, secondary_model=sec, clip_kwargs=clip_kwargs))
    gm = gdm.conditioning.grad_modules[0]
    assert isinstance(gm, CLIPGrads) and gm.clip_models[0] is m and m.bpe_path == vocab
    a, b = "a fractal city", "hello the city"
    kw = dict(audio=wav, sr=1024 * fps, fps=fps, n_frames=n_frames, size=(64, 64), timesteps=4, model=net, diffusion=sd,
              grad_modules=[gm], seed=5, batch=4, speed="fast", secondary_model=sec)
    torch.manual_seed(21)   # (the cutouts are drawn from torch's global generator)
    frames, pidx = sample([TextPrompt(a), TextPrompt(b)], **kw)
    assert torch.equal(pidx, idx[:n_frames]) and int(pidx.max()) == 1 and bool(torch.isfinite(frames).all())
    emb = m.encode_text([a, b]).cpu()
    ref = CLIPGrads(scale=500.0, clip_models=[small_model()], cutout_kwargs=dict(cutn=8), cutout_batches=1, clamp_gradient=0.05)
    torch.manual_seed(21)
    frames_e, _ = sample([EmbeddingPrompt(emb[0]), EmbeddingPrompt(emb[1])], **{**kw, "grad_modules": [ref]})
    assert torch.equal(frames, frames_e)
    # the step-by-step loop (no hipGraph) gives the same frames
    init = GuidedDiffusion.__init__

    def no_graph(self, *a_, **k_):
        init(self, *a_, **k_)
        self.use_graph = False
    monkeypatch.setattr(GuidedDiffusion, "__init__", no_graph)
    torch.manual_seed(21)
    frames_s, _ = sample([TextPrompt(a), TextPrompt(b)], **kw)
    assert torch.equal(frames, frames_s)
    # the prompts steer: one prompt for every frame ends elsewhere
    monkeypatch.setattr(GuidedDiffusion, "__init__", init)
    torch.manual_seed(21)
    frames_1, _ = sample([TextPrompt(a), TextPrompt(a)], **kw)
    assert not torch.equal(frames_1[switch:], frames[switch:])
