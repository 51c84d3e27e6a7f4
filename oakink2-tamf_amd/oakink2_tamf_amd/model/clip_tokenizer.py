"""CLIP's byte-level BPE tokenizer, written from its published description (Radford et al. 2021; the scheme of GPT-2's encoder with a
lower-cased, whitespace-cleaned input and an end-of-word marker).  The merges file is the USER's (`bpe_simple_vocab_16e6.txt.gz` of
OpenAI's release, or any file of that layout); none is shipped.

Vocabulary, in id order: the 256 byte symbols (every byte mapped to a printable unicode character), the same 256 with `</w>`
appended, one entry per merge, `<|startoftext|>`, `<|endoftext|>`.  The file's first line is a header; at most `max_merges` lines
after it are used (48 894 by default, which gives the 49 408 entries of the published models), a shorter file gives all of its lines.

A text is html-unescaped twice, whitespace-collapsed, stripped and lower-cased, split by PATTERN, and every piece is encoded on its
own: its UTF-8 bytes become symbols, the last one carries `</w>`, and the adjacent pair of lowest merge rank is merged (every
occurrence, left to right) until no pair has a rank.

The reference's pipeline also runs `ftfy.fix_text` first.  That package is not required here; for ASCII text it is the identity, so a
prompt with a non-ASCII character is refused (ValueError naming the prompt) instead of being tokenised differently."""
from __future__ import annotations

import gzip
import html
from typing import Dict, List, Sequence, Tuple, Union

import numpy as np

PATTERN = r"<\|startoftext\|>|<\|endoftext\|>|'s|'t|'re|'ve|'m|'ll|'d|[\p{L}]+|[\p{N}]|[^\s\p{L}\p{N}]+"
DEFAULT_MAX_MERGES = 49152 - 256 - 2  # 48 894
SOT, EOT = "<|startoftext|>", "<|endoftext|>"


def bytes_to_unicode() -> Dict[int, str]:
    """byte -> printable character, in vocabulary order: first the 188 printable Latin-1 bytes ('!'..'~', 0xA1..0xAC, 0xAE..0xFF), which
    keep their own character, then the other 68 in byte order, which take chr(256), chr(257), ..."""
    keep = list(range(ord("!"), ord("~") + 1)) + list(range(0xA1, 0xAC + 1)) + list(range(0xAE, 0xFF + 1))
    table = {b: chr(b) for b in keep}
    for b in range(256):
        if b not in table:
            table[b] = chr(256 + len(table) - len(keep))
    return table


def read_merges(path: str, max_merges: int = DEFAULT_MAX_MERGES) -> List[Tuple[str, str]]:
    """the merge pairs of a `.txt` or `.txt.gz` file: header line skipped, at most max_merges lines, each `left right`"""
    opener = gzip.open if str(path).endswith(".gz") else open
    with opener(path, "rt", encoding="utf-8") as f:
        lines = f.read().split("\n")
    merges = []
    for n, ln in enumerate(lines[1: 1 + int(max_merges)], start=2):
        if ln == "":
            continue
        parts = ln.split()
        if len(parts) != 2:
            raise ValueError(f"{path}:{n}: expected two symbols, got {ln!r}")
        merges.append((parts[0], parts[1]))
    return merges


class ClipTokenizer:
    def __init__(self, bpe_path: str, max_merges: int = DEFAULT_MAX_MERGES):
        import regex

        self.byte_encoder = bytes_to_unicode()
        merges = read_merges(bpe_path, max_merges)
        symbols = list(self.byte_encoder.values())
        vocab = symbols + [s + "</w>" for s in symbols] + ["".join(m) for m in merges] + [SOT, EOT]
        self.encoder = {}
        for i, tok in enumerate(vocab):
            self.encoder.setdefault(tok, i)  # (a repeated entry keeps its first id and still takes up a slot)
        self.vocab_size = len(vocab)
        self.bpe_ranks = {}
        for i, m in enumerate(merges):
            self.bpe_ranks.setdefault(m, i)
        self.sot_id, self.eot_id = self.vocab_size - 2, self.vocab_size - 1
        self._cache = {SOT: [self.sot_id], EOT: [self.eot_id]}
        self._pat = regex.compile(PATTERN, regex.IGNORECASE)

    @staticmethod
    def clean(text: str) -> str:
        if not text.isascii():
            bad = sorted({c for c in text if ord(c) > 127})
            raise ValueError(f"prompt {text!r} holds non-ASCII characters {bad}: this tokenizer has no ftfy step and takes ASCII text only")
        text = html.unescape(html.unescape(text))
        if not text.isascii():  # (an entity such as &eacute;)
            raise ValueError(f"prompt {text!r} holds a non-ASCII character after html unescaping: this tokenizer takes ASCII text only")
        return " ".join(text.split()).strip().lower()

    def bpe(self, piece: str) -> List[int]:
        """ids of one piece of the split"""
        if piece in self._cache:
            return self._cache[piece]
        word = [self.byte_encoder[b] for b in piece.encode("utf-8")]
        word[-1] += "</w>"
        while len(word) > 1:
            ranks = [self.bpe_ranks.get((a, b)) for a, b in zip(word, word[1:])]
            known = [r for r in ranks if r is not None]
            if not known:
                break
            first, second = word[ranks.index(min(known))], word[ranks.index(min(known)) + 1]
            out, i = [], 0
            while i < len(word):
                if i + 1 < len(word) and word[i] == first and word[i + 1] == second:
                    out.append(first + second)
                    i += 2
                else:
                    out.append(word[i])
                    i += 1
            word = out
        ids = [self.encoder[s] for s in word]
        self._cache[piece] = ids
        return ids

    def encode(self, text: str) -> List[int]:
        """ids of a text, without the start and end markers"""
        ids: List[int] = []
        for piece in self._pat.findall(self.clean(text)):
            ids.extend(self.bpe(piece))
        return ids

    def tokenize(self, texts: Union[str, Sequence[str]], context_length: int = 77, truncate: bool = False) -> np.ndarray:
        """(B, context_length) int32: [SOT] + ids + [EOT], zero-padded.  A text that does not fit raises ValueError, or with `truncate`
        is cut to context_length with its last id set to EOT."""
        if isinstance(texts, str):
            texts = [texts]
        out = np.zeros((len(texts), int(context_length)), dtype=np.int32)
        for i, text in enumerate(texts):
            ids = [self.sot_id] + self.encode(text) + [self.eot_id]
            if len(ids) > context_length:
                if not truncate:
                    raise ValueError(f"prompt {text!r} has {len(ids)} tokens, the context length is {context_length}")
                ids = ids[:context_length]
                ids[-1] = self.eot_id
            out[i, : len(ids)] = ids
        return out

    def token_count(self, text: str) -> int:
        """tokens of a text with its start and end markers, before any truncation"""
        return len(self.encode(text)) + 2


__all__ = ["ClipTokenizer", "PATTERN", "DEFAULT_MAX_MERGES", "bytes_to_unicode", "read_merges"]
