"""CLIP's byte-level BPE tokenizer and ``clip.tokenize``, restated from the published algorithm (clip/simple_tokenizer.py, clip/clip.py).

``tokenize(texts, context_length=77, truncate=False, bpe_path=None)`` -> int32 [n, context_length]: per row ``<|startoftext|>``, the
text's BPE ids, ``<|endoftext|>``, zero padding.  The vocabulary is built like CLIP builds it: the 256 byte symbols of
``bytes_to_unicode``, the same symbols with ``</w>``, one entry per merge (the merges file's lines ``[1 : 49152 - 256 - 2 + 1]``),
then ``<|startoftext|>`` and ``<|endoftext|>`` - so sot = len(vocab) - 2 and eot = len(vocab) - 1 (49406 / 49407 for CLIP's file).

The merges file (``bpe_simple_vocab_16e6.txt.gz``, gzip or plain text) is not bundled and never downloaded.  It is looked for at
``bpe_path``, then in ``~/.cache/clip/`` (next to the checkpoints ``clip.load`` caches), then as the installed ``clip`` package's own
copy.  Text cleaning: ``html.unescape`` twice, whitespace collapsed, lower-cased, CLIP's token pattern (the ``regex`` module, for
``\\p{L}`` / ``\\p{N}``).  Deviation: ``ftfy.fix_text`` runs only when ``ftfy`` is importable - it repairs mojibake ("Ã©" for "é") and
leaves well-formed text alone, so without it only such broken input tokenizes differently from CLIP.
"""
import functools
import gzip
import html
import importlib.util
import os
import re

import torch

VOCAB_FILE = "bpe_simple_vocab_16e6.txt.gz"
SOT, EOT = "<|startoftext|>", "<|endoftext|>"
_PATTERN = r"""<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"""


@functools.lru_cache()
def bytes_to_unicode():
    """byte -> printable unicode character: the printable latin-1 bytes map to themselves, the other 68 to chr(256 + k) in order."""
    bs = list(range(ord("!"), ord("~") + 1)) + list(range(ord("¡"), ord("¬") + 1)) + list(range(ord("®"), ord("ÿ") + 1))
    cs = bs[:]
    n = 0
    for b in range(256):
        if b not in bs:
            bs.append(b)
            cs.append(256 + n)
            n += 1
    return dict(zip(bs, (chr(c) for c in cs)))


def get_pairs(word):
    return {(word[i], word[i + 1]) for i in range(len(word) - 1)}


def _regex():
    try:
        import regex
    except ImportError as e:
        raise ImportError("maua_amd.clip_tokenizer needs the `regex` module (CLIP's token pattern uses \\p{L} / \\p{N}): "
                          "pip install regex") from e
    return regex


def clean(text):
    try:
        import ftfy
        text = ftfy.fix_text(text)
    except ImportError:
        pass
    text = html.unescape(html.unescape(text)).strip()
    return re.sub(r"\s+", " ", text).strip().lower()


def find_vocab(bpe_path=None):
    """The merges file: ``bpe_path``, else ~/.cache/clip/<VOCAB_FILE>, else the installed clip package's copy."""
    tried = []
    if bpe_path is not None:
        if os.path.isfile(bpe_path):
            return str(bpe_path)
        tried.append(f"bpe_path={bpe_path!s}")
    else:
        tried.append("bpe_path (not given)")
    cache = os.path.join(os.path.expanduser("~/.cache/clip"), VOCAB_FILE)
    if os.path.isfile(cache):
        return cache
    tried.append(cache)
    spec = importlib.util.find_spec("clip")
    if spec is not None and spec.origin:
        pkg = os.path.join(os.path.dirname(spec.origin), VOCAB_FILE)
        if os.path.isfile(pkg):
            return pkg
        tried.append(pkg)
    else:
        tried.append("the installed `clip` package (not importable)")
    raise FileNotFoundError(f"CLIP's BPE vocabulary {VOCAB_FILE} not found; looked at: {'; '.join(tried)}. It is not downloaded: "
                            "pass bpe_path=..., or place the file in ~/.cache/clip/")


def _read_merges(path):
    with open(path, "rb") as f:
        data = f.read()
    if data[:2] == b"\x1f\x8b":
        data = gzip.decompress(data)
    lines = data.decode("utf-8").split("\n")
    # (blank lines dropped: CLIP's file has ~262 000 merges, so its slice never reaches the trailing newline a shorter file ends in)
    return [tuple(m.split()) for m in lines[1:49152 - 256 - 2 + 1] if m.strip()]


class SimpleTokenizer:
    """clip/simple_tokenizer.py SimpleTokenizer: ``encode(text)`` -> BPE ids (no sot / eot)."""

    def __init__(self, bpe_path=None):
        merges = _read_merges(find_vocab(bpe_path))
        self.byte_encoder = bytes_to_unicode()
        vocab = list(self.byte_encoder.values())
        vocab = vocab + [v + "</w>" for v in vocab]
        vocab += ["".join(m) for m in merges]
        vocab += [SOT, EOT]
        self.encoder = dict(zip(vocab, range(len(vocab))))
        self.decoder = {v: k for k, v in self.encoder.items()}
        self.bpe_ranks = dict(zip(merges, range(len(merges))))
        self.cache = {SOT: SOT, EOT: EOT}
        self.pat = _regex().compile(_PATTERN, _regex().IGNORECASE)
        self.sot, self.eot = self.encoder[SOT], self.encoder[EOT]

    def bpe(self, token):
        """One pre-token (byte symbols) -> its BPE symbols joined by spaces; the lowest-ranked adjacent pair merges first."""
        if token in self.cache:
            return self.cache[token]
        word = tuple(token[:-1]) + (token[-1] + "</w>",)
        pairs = get_pairs(word)
        if not pairs:
            return token + "</w>"
        while True:
            bigram = min(pairs, key=lambda p: self.bpe_ranks.get(p, float("inf")))
            if bigram not in self.bpe_ranks:
                break
            first, second = bigram
            new_word, i = [], 0
            while i < len(word):
                try:
                    j = word.index(first, i)
                except ValueError:
                    new_word.extend(word[i:])
                    break
                new_word.extend(word[i:j])
                i = j
                if word[i] == first and i < len(word) - 1 and word[i + 1] == second:
                    new_word.append(first + second)
                    i += 2
                else:
                    new_word.append(word[i])
                    i += 1
            word = tuple(new_word)
            if len(word) == 1:
                break
            pairs = get_pairs(word)
        out = " ".join(word)
        self.cache[token] = out
        return out

    def encode(self, text):
        ids = []
        for token in self.pat.findall(clean(text)):
            token = "".join(self.byte_encoder[b] for b in token.encode("utf-8"))
            ids.extend(self.encoder[t] for t in self.bpe(token).split(" "))
        return ids

    def decode(self, ids):
        text = "".join(self.decoder[i] for i in ids)
        byte_decoder = {v: k for k, v in self.byte_encoder.items()}
        return bytearray(byte_decoder[c] for c in text).decode("utf-8", errors="replace").replace("</w>", " ")


@functools.lru_cache(maxsize=8)
def _tokenizer_at(path, mtime):
    return SimpleTokenizer(path)


def get_tokenizer(bpe_path=None):
    """The tokenizer of the vocabulary ``find_vocab(bpe_path)`` resolves to (built once per file)."""
    path = find_vocab(bpe_path)
    return _tokenizer_at(path, os.path.getmtime(path))


def tokenize(texts, context_length=77, truncate=False, bpe_path=None):
    """clip.tokenize: a string or a list of strings -> int32 [n, context_length], rows ``sot ids eot`` padded with zeros.  A row longer
    than context_length raises RuntimeError, or with ``truncate`` is cut to context_length with eot as its last id."""
    if isinstance(texts, str):
        texts = [texts]
    tok = get_tokenizer(bpe_path)
    rows = [[tok.sot] + tok.encode(t) + [tok.eot] for t in texts]
    result = torch.zeros(len(rows), context_length, dtype=torch.int32)
    for i, ids in enumerate(rows):
        if len(ids) > context_length:
            if not truncate:
                raise RuntimeError(f"Input {texts[i]} is too long for context length {context_length}")
            ids = ids[:context_length]
            ids[-1] = tok.eot
        result[i, :len(ids)] = torch.tensor(ids, dtype=torch.int32)
    return result
