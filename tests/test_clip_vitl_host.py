"""CPU-only checks of the ViT-L/14 perceptors (224 and 336 px): the config tables, ``clip.load``'s rules for the new names, the
parameter shapes against the oracle's, a whole synthetic CLIP state dict through both towers' loaders, and the new C-ABI entry point."""
import ctypes

import pytest
import torch

from maua_amd import _lib as L
from maua_amd import clip as CL
from oracle import clip as OC

L14 = "ViT-L/14"
L14_336 = "ViT-L/14@336px"


def test_config_tables():
    assert CL.VISION_CONFIGS[L14] == (224, 14, 1024, 24, 16, 768)
    assert CL.VISION_CONFIGS[L14_336] == (336, 14, 1024, 24, 16, 768)
    for name in (L14, L14_336):
        assert CL.TEXT_CONFIGS[name] == (77, 49408, 768, 12, 12, 768)
        res, p, w, layers, heads, E = CL.VISION_CONFIGS[name]
        assert res % p == 0 and w // heads == 64 and CL.TEXT_CONFIGS[name][2] // CL.TEXT_CONFIGS[name][4] == 64
    # the towers this build already had are untouched
    assert CL.VISION_CONFIGS["ViT-B/16"] == (224, 16, 768, 12, 12, 512) and CL.TEXT_CONFIGS["ViT-B/16"] == (77, 49408, 512, 12, 8, 512)


def test_load_without_weights_is_file_not_found_and_resnets_stay_refused(tmp_path, monkeypatch):
    monkeypatch.setenv("HOME", str(tmp_path))   # (no ~/.cache/clip here)
    for name in (L14, L14_336):
        with pytest.raises(FileNotFoundError):
            CL.load(name)
    with pytest.raises(NotImplementedError) as e:
        CL.load("RN50")
    assert "ViT-L/14" in str(e.value) and "14-pixel" not in str(e.value)   # (listed among the towers, no longer named as missing)


@pytest.fixture(scope="module")
def synthetic_state_dict():
    """A whole CLIP ViT-L/14 state dict by shape: visual.* from the oracle's table, the 768-wide text half, logit_scale."""
    cfg = OC.vit_config(*CL.VISION_CONFIGS[L14])
    sd = {k: torch.full(shape, 0.01) for k, shape in OC.vit_param_shapes(cfg).items()}
    ctx, vocab, w, layers, heads, E = CL.TEXT_CONFIGS[L14]
    text = {"token_embedding.weight": (vocab, w), "positional_embedding": (ctx, w), "ln_final.weight": (w,), "ln_final.bias": (w,),
            "text_projection": (w, E)}
    for i in range(layers):
        b = f"transformer.resblocks.{i}."
        text.update({b + "attn.in_proj_weight": (3 * w, w), b + "attn.in_proj_bias": (3 * w,), b + "attn.out_proj.weight": (w, w),
                     b + "attn.out_proj.bias": (w,), b + "ln_1.weight": (w,), b + "ln_1.bias": (w,), b + "mlp.c_fc.weight": (4 * w, w),
                     b + "mlp.c_fc.bias": (4 * w,), b + "mlp.c_proj.weight": (w, 4 * w), b + "mlp.c_proj.bias": (w,),
                     b + "ln_2.weight": (w,), b + "ln_2.bias": (w,)})
    sd.update({k: torch.full(shape, 0.02) for k, shape in text.items()})
    sd["logit_scale"] = torch.tensor(4.6)
    return cfg, sd


def test_parameter_shapes_equal_the_oracles_and_a_whole_state_dict_loads(synthetic_state_dict):
    cfg, sd = synthetic_state_dict
    vt = CL.VisionTransformer(*CL.VISION_CONFIGS[L14])
    assert {"visual." + k: tuple(s) for k, s in vt._param_shapes().items()} == {k: tuple(s) for k, s in OC.vit_param_shapes(cfg).items()}
    assert tuple(vt.state_dict()["conv1.weight"].shape) == (1024, 3, 14, 14)
    assert tuple(vt.state_dict()["positional_embedding"].shape) == (257, 1024)
    model, _ = CL.load(L14, state_dict=sd)
    assert model.text is not None and (model.text.width, model.text.heads, model.text.embed_dim) == (768, 12, 768)
    assert float(model.visual.state_dict()["transformer.resblocks.23.mlp.c_fc.weight"][5, 7]) == pytest.approx(0.01)
    assert float(model.text.state_dict()["text_projection"][3, 3]) == pytest.approx(0.02)
    assert model.visual.input_resolution == 224 and model.visual.patch_size == 14
    # the 336 px tower differs in its positional embedding only: 577 tokens
    assert CL.VisionTransformer(*CL.VISION_CONFIGS[L14_336])._param_shapes()["positional_embedding"] == (577, 1024)
    # a 14-pixel conv1.weight of the wrong shape is refused by name
    bad = dict(sd)
    bad["visual.conv1.weight"] = torch.zeros(1024, 3, 16, 16)
    with pytest.raises(ValueError, match="conv1.weight"):
        vt.load_state_dict(bad, strict=False)


def test_library_exports_the_workspace_limit_entry_point():
    from maua_amd.build import build
    lib = ctypes.CDLL(str(build()))
    assert "maua_clip_set_workspace_limit" in L.declared_symbols()
    assert hasattr(lib, "maua_clip_set_workspace_limit")
