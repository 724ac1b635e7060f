"""CPU tests of CLIP's text side: the BPE tokenizer (maua_amd/clip_tokenizer.py) on a synthetic merges file whose ids can be worked
out by hand, and the host side of the text tower (maua_amd.clip.TextTransformer / load): keys, state-dict filtering, which models
get a tower, and the token checks that run before anything reaches the device."""
import gzip

import pytest
import torch

from maua_amd import clip as CL
from maua_amd import clip_tokenizer as CT

# A merges file: a header line, then merges in rank order.  Their ids follow the 256 byte symbols and the 256 "</w>" symbols.
MERGES = ["h e", "l l", "he ll", "hell o</w>", "t h", "th e</w>", "' s</w>", "l l</w>"]
HE, LL, HELL, HELLO, TH, THE, S_APOS, LL_W = range(512, 520)
SOT, EOT = 520, 521


def sym(ch):
    """id of a printable ASCII byte symbol ('!' .. '~' come first in bytes_to_unicode's order)."""
    return ord(ch) - ord("!")


def sym_w(ch):
    return 256 + sym(ch)


@pytest.fixture
def vocab(tmp_path):
    path = tmp_path / "merges.txt.gz"
    path.write_bytes(gzip.compress(("#version: synthetic\n" + "\n".join(MERGES) + "\n").encode()))
    return str(path)


def enc(vocab, text):
    return CT.get_tokenizer(vocab).encode(text)


def test_bytes_to_unicode_is_a_bijection_on_printable_characters():
    b2u = CT.bytes_to_unicode()
    assert len(b2u) == 256 and len(set(b2u.values())) == 256
    assert all(b2u[b] == chr(b) for b in range(ord("!"), ord("~") + 1))
    assert b2u[0] == chr(256) and b2u[ord(" ")] == chr(256 + 32)
    assert list(b2u.values())[:3] == ["!", '"', "#"]


def test_vocabulary_layout_and_special_tokens(vocab):
    tok = CT.get_tokenizer(vocab)
    assert len(tok.encoder) == 256 * 2 + len(MERGES) + 2
    assert tok.sot == len(tok.encoder) - 2 == SOT and tok.eot == len(tok.encoder) - 1 == EOT
    assert tok.encoder["hello</w>"] == HELLO and tok.encoder["a"] == sym("a") and tok.encoder["a</w>"] == sym_w("a")


def test_full_merge_and_byte_fallback(vocab):
    assert enc(vocab, "hello") == [HELLO]
    assert enc(vocab, "xyz") == [sym("x"), sym("y"), sym_w("z")]      # no merge applies: byte symbols, </w> on the last
    assert enc(vocab, "the") == [THE]
    # "hell": h e l l</w> -> he l l</w> ("h e" ranks first) -> "l l</w>" (rank 7) is the only ranked pair left -> he ll</w>
    assert enc(vocab, "hell") == [HE, LL_W]
    assert enc(vocab, "a") == [sym_w("a")]                               # one symbol: no pairs


def test_end_of_word_marker(vocab):
    # "o</w>" is a different symbol from "o": "hello" merges through "hell o</w>", "helloo" cannot use it
    assert enc(vocab, "helloo") == [HELL, sym("o"), sym_w("o")]
    assert enc(vocab, "ll") == [LL_W] and enc(vocab, "llx") == [LL, sym_w("x")]


def test_merge_rank_decides_between_competing_pairs(vocab):
    # "lll": l l l</w> - both "l l" (rank 1) and "l l</w>" (rank 7) apply; the lower rank merges first: ll l</w>, not l ll</w>
    assert enc(vocab, "lll") == [LL, sym_w("l")]


def test_contractions_split_off(vocab):
    assert enc(vocab, "it's") == [sym("i"), sym_w("t"), S_APOS]
    assert enc(vocab, "we'll") == [sym("w"), sym_w("e"), sym("'"), LL_W]


def test_non_ascii_becomes_byte_symbols(vocab):
    # "é" = UTF-8 c3 a9; bytes_to_unicode: 0xc3 sits at 94 + 12 + (0xc3 - 0xae), 0xa9 at 94 + (0xa9 - 0xa1)
    assert enc(vocab, "é") == [94 + 12 + (0xC3 - 0xAE), 256 + 94 + (0xA9 - 0xA1)]
    assert enc(vocab, "42!") == [sym_w("4"), sym_w("2"), sym_w("!")]   # digits one by one, punctuation as its own token


def test_cleaning_unescape_whitespace_lowercase(vocab):
    assert enc(vocab, "  HELLO &amp;\n\t The  ") == [HELLO, sym_w("&"), THE]
    assert enc(vocab, "&amp;amp;") == [sym_w("&")]                        # html.unescape twice
    assert enc(vocab, "Hello") == enc(vocab, "hello")


def test_tokenize_rows_padding_and_dtype(vocab):
    t = CT.tokenize(["hello", "xyz"], context_length=8, bpe_path=vocab)
    assert t.dtype == torch.int32 and tuple(t.shape) == (2, 8)
    assert t[0].tolist() == [SOT, HELLO, EOT, 0, 0, 0, 0, 0]
    assert t[1].tolist() == [SOT, sym("x"), sym("y"), sym_w("z"), EOT, 0, 0, 0]
    assert torch.equal(CT.tokenize("hello", context_length=8, bpe_path=vocab), t[:1])
    assert torch.equal(CL.tokenize("hello", context_length=8, bpe_path=vocab), t[:1])   # re-exported as maua_amd.clip.tokenize
    assert tuple(CT.tokenize("hello", bpe_path=vocab).shape) == (1, 77)


def test_tokenize_truncation(vocab):
    with pytest.raises(RuntimeError, match="Input hello hello hello is too long for context length 4"):
        CT.tokenize("hello hello hello", context_length=4, bpe_path=vocab)
    t = CT.tokenize(["hello hello hello", "hello"], context_length=4, truncate=True, bpe_path=vocab)
    assert t.tolist() == [[SOT, HELLO, HELLO, EOT], [SOT, HELLO, EOT, 0]]
    assert CT.tokenize("hello hello", context_length=4, bpe_path=vocab).tolist() == [[SOT, HELLO, HELLO, EOT]]   # fits exactly


def test_plain_text_merges_file_and_the_cache_directory(tmp_path, monkeypatch):
    home = tmp_path / "home"
    (home / ".cache" / "clip").mkdir(parents=True)
    (home / ".cache" / "clip" / CT.VOCAB_FILE).write_text("#version: synthetic\n" + "\n".join(MERGES) + "\n")
    monkeypatch.setenv("HOME", str(home))
    assert CT.find_vocab() == str(home / ".cache" / "clip" / CT.VOCAB_FILE)
    assert CT.tokenize("hello", context_length=4).tolist() == [[SOT, HELLO, EOT, 0]]


def test_missing_vocabulary_names_every_place(tmp_path, monkeypatch):
    monkeypatch.setenv("HOME", str(tmp_path))
    monkeypatch.setattr(CT.importlib.util, "find_spec", lambda name: None)
    with pytest.raises(FileNotFoundError) as e:
        CT.tokenize("hello")
    msg = str(e.value)
    assert "bpe_path" in msg and str(tmp_path / ".cache" / "clip" / CT.VOCAB_FILE) in msg and "clip" in msg
    with pytest.raises(FileNotFoundError, match="nowhere.txt.gz"):
        CT.tokenize("hello", bpe_path=str(tmp_path / "nowhere.txt.gz"))


def test_real_vocabulary_when_present():
    try:
        path = CT.find_vocab()
    except FileNotFoundError:
        pytest.skip("CLIP's bpe_simple_vocab_16e6.txt.gz is not on this machine")
    tok = CT.get_tokenizer(path)
    assert len(tok.encoder) == 49408 and tok.sot == 49406 and tok.eot == 49407
    t = CT.tokenize("a diagram", bpe_path=path)
    assert t[0, 0] == 49406 and int(t[0].argmax()) == int((t[0] != 0).sum()) - 1


# ------------------------------------------------------------------------------------------------ the text tower's host side
SMALL_TEXT = (16, 600, 64, 2, 2, 32)   # context, vocab, width, layers, heads, embed


def clip_text_keys(layers):
    keys = {"token_embedding.weight", "positional_embedding", "ln_final.weight", "ln_final.bias", "text_projection"}
    for i in range(layers):
        for k in ("attn.in_proj_weight", "attn.in_proj_bias", "attn.out_proj.weight", "attn.out_proj.bias", "ln_1.weight", "ln_1.bias",
                  "mlp.c_fc.weight", "mlp.c_fc.bias", "mlp.c_proj.weight", "mlp.c_proj.bias", "ln_2.weight", "ln_2.bias"):
            keys.add(f"transformer.resblocks.{i}.{k}")
    return keys


def test_text_configs_and_keys_of_vit_b16():
    assert CL.TEXT_CONFIGS["ViT-B/16"] == CL.TEXT_CONFIGS["ViT-B/32"] == (77, 49408, 512, 12, 8, 512)
    tt = CL.TextTransformer(*CL.TEXT_CONFIGS["ViT-B/16"])
    sd = tt.state_dict()
    assert set(sd) == clip_text_keys(12)
    assert tuple(sd["token_embedding.weight"].shape) == (49408, 512) and tuple(sd["text_projection"].shape) == (512, 512)
    assert tuple(sd["transformer.resblocks.11.attn.in_proj_weight"].shape) == (1536, 512)
    assert tuple(sd["transformer.resblocks.0.mlp.c_proj.weight"].shape) == (512, 2048)
    # CLIP.initialize_parameters' stds
    assert abs(float(sd["token_embedding.weight"].std()) - 0.02) < 1e-3 and abs(float(sd["positional_embedding"].std()) - 0.01) < 1e-3
    assert abs(float(sd["text_projection"].std()) - 512 ** -0.5) < 2e-3


def _whole_state_dict(text_cfg, vis_cfg, seed=0):
    g = torch.Generator().manual_seed(seed)
    vt = CL.VisionTransformer(*vis_cfg, generator=g)
    tt = CL.TextTransformer(*text_cfg, generator=g)
    sd = {"visual." + k: v for k, v in vt._params.items()}
    sd.update(tt._params)
    sd.update({"logit_scale": torch.tensor(4.6052), "input_resolution": torch.tensor(vis_cfg[0]),
               "context_length": torch.tensor(text_cfg[0]), "vocab_size": torch.tensor(text_cfg[1])})
    return sd, tt


def test_load_state_dict_takes_exactly_the_text_half():
    sd, src = _whole_state_dict(SMALL_TEXT, (32, 8, 64, 2, 2, 32))
    tt = CL.TextTransformer(*SMALL_TEXT, generator=torch.Generator().manual_seed(9))
    res = tt.load_state_dict(sd)                    # strict: visual.*, logit_scale and the archive entries are not "unexpected"
    assert not res.missing_keys and not res.unexpected_keys
    got = tt.state_dict()
    assert set(got) == clip_text_keys(2) and all(torch.equal(got[k], src._params[k]) for k in got)
    with pytest.raises(KeyError):
        tt.load_state_dict({k: v for k, v in sd.items() if k != "ln_final.bias"})
    with pytest.raises(ValueError):
        tt.load_state_dict({**sd, "text_projection": torch.zeros(64, 31)})


def test_load_state_dict_clears_the_embedding_cache():
    tt = CL.TextTransformer(*SMALL_TEXT)
    tt._cache[b"row"] = torch.zeros(32)
    tt.load_state_dict(tt.state_dict())
    assert tt._cache == {}


def test_load_builds_the_text_tower_when_asked_or_when_the_weights_have_it():
    sd, src = _whole_state_dict(CL.TEXT_CONFIGS["ViT-B/16"], CL.VISION_CONFIGS["ViT-B/16"])
    m, _ = CL.load("ViT-B/16", state_dict=sd)
    assert isinstance(m.text, CL.TextTransformer) and torch.equal(m.text.state_dict()["text_projection"], src._params["text_projection"])
    assert torch.equal(m.visual.state_dict()["proj"], sd["visual.proj"])
    assert CL.load("ViT-B/16", state_dict=sd, text_tower=False)[0].text is None
    del sd, src, m
    # random init: no text tower unless asked for (tests/test_oracle_clip.py pins the image-only model)
    assert CL.load("ViT-B/16", allow_random_init=True)[0].text is None
    m, _ = CL.load("ViT-B/16", allow_random_init=True, text_tower=True, bpe_path="/some/vocab.txt")
    assert isinstance(m.text, CL.TextTransformer) and m.text.context_length == 77 and m.bpe_path == "/some/vocab.txt"
    with pytest.raises(FileNotFoundError):
        CL.load("ViT-B/16", state_dict={"visual.proj": torch.zeros(768, 512)}, text_tower=True)


def test_encode_text_order_and_token_checks():
    vt = CL.VisionTransformer(32, 8, 64, 2, 2, 32)
    tt = CL.TextTransformer(*SMALL_TEXT)
    # a supplied text_encoder wins over the tower; no tower and no encoder: NotImplementedError
    assert CL.CLIPImageModel(vt, lambda s: ("enc", s), tt).encode_text("x") == ("enc", "x")
    with pytest.raises(NotImplementedError):
        CL.CLIPImageModel(vt).encode_text("x")
    # bad ids / shapes are ValueErrors raised on the host, before anything is launched
    ok = torch.zeros(2, 16, dtype=torch.int64)
    assert tt.check_tokens(ok) is not None
    for bad in (torch.full((1, 16), 600), torch.full((1, 16), -1), torch.zeros(1, 15, dtype=torch.int32), torch.zeros(16, dtype=torch.int32),
                torch.zeros(1, 16, dtype=torch.float32)):
        with pytest.raises(ValueError):
            tt(bad)
