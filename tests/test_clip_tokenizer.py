"""CPU: model/clip_tokenizer.py on the committed synthetic merges file tests/golden/clip_bpe_synthetic.txt (41 hand-made merges behind a
header line; not a trained vocabulary).  Ids are derived by hand from the vocabulary layout - 256 byte symbols (the 188 printable
bytes first: '!' is 0, 'a' is 64), the same with `</w>` at 256 + i, merge k at 512 + k, then SOT and EOT - and the BPE is compared
with a naive independent implementation on generated strings."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN

from oakink2_tamf_amd.model.clip_tokenizer import ClipTokenizer, bytes_to_unicode, read_merges

BPE = os.path.join(GOLDEN, "clip_bpe_synthetic.txt")
N_MERGES = 41
SOT, EOT = 512 + N_MERGES, 512 + N_MERGES + 1


def sym(ch):  # id of a printable ASCII byte symbol: position in '!'..'~'
    return ord(ch) - ord("!")


def end(ch):  # ... of the same symbol with </w>
    return 256 + sym(ch)


def merge(k):  # id of the k-th merge (0-based line after the header)
    return 512 + k


@pytest.fixture(scope="module")
def tok():
    return ClipTokenizer(BPE)


def test_vocabulary_layout(tok):
    b2u = bytes_to_unicode()
    assert len(b2u) == 256 and len(set(b2u.values())) == 256 and all(c.isprintable() and not c.isspace() for c in b2u.values())
    assert list(b2u)[:3] == [33, 34, 35] and b2u[ord("a")] == "a" and b2u[32] == chr(256 + 32) and b2u[0] == chr(256)
    assert len(read_merges(BPE)) == N_MERGES
    assert tok.vocab_size == 512 + N_MERGES + 2 and (tok.sot_id, tok.eot_id) == (SOT, EOT)
    assert tok.encoder["!"] == 0 and tok.encoder["a"] == sym("a") == 64 and tok.encoder["a</w>"] == 256 + 64
    assert tok.encoder["the</w>"] == merge(1) and tok.encoder["th"] == merge(0) and tok.encoder["er</w>"] == merge(40)


def test_hand_derived_ids(tok):
    # "the": t h e</w> -> (t h) rank 0 -> th e</w> -> rank 1 -> the</w>
    assert tok.encode("the") == [merge(1)]
    # "hand": h a n d</w>: (a n) rank 3 wins over (h a) rank 7 -> h an d</w> -> (an d</w>) rank 4 -> h and</w>; "han d</w>" never forms
    assert tok.encode("hand") == [sym("h"), merge(4)]
    # "bottle": b o t t l e</w>: (b o) 19, (t t) 20, (l e</w>) 22 -> bo tt le</w> -> (bo tt) 21 -> bott le</w> -> 23
    assert tok.encode("bottle") == [merge(23)]
    # "there": (t h) 0 -> th e r e</w>; (e r) rank 6 -> th er e</w>; nothing joins th + er or er + e</w>
    assert tok.encode("there") == [merge(0), merge(6), end("e")]
    # "other": o t h e r</w>: (t h) 0 -> o th e r</w>; (e r</w>) rank 40 -> o th er</w>
    assert tok.encode("other") == [sym("o"), merge(0), merge(40)]
    # a word no merge touches: one id per byte, the last with </w>
    assert tok.encode("zzz") == [sym("z"), sym("z"), end("z")]
    assert tok.encode("hold the cup") == [merge(14), merge(1), merge(11)]
    assert tok.encode("") == [] and tok.encode("   ") == []


def test_splits_and_cleaning(tok):
    # 's is a piece of its own; a digit is a piece per digit; punctuation runs stay together
    assert tok.encode("cup's") == [merge(11), merge(24)]
    assert tok.encode("42") == [end("4"), end("2")]
    assert tok.encode("a1b") == [end("a"), end("1"), end("b")]
    assert tok.encode("go!!") == [sym("g"), end("o"), merge(38)]
    assert tok.encode("what?!") == tok.encode("what") + [merge(39)]
    assert tok.encode("x!!!") == [end("x"), sym("!"), merge(38)]  # only (! !</w>) has a rank: "!" + "!!</w>" stays two symbols
    # whitespace collapse, strip, lower-casing, html unescaping (twice)
    assert tok.encode("  Hold \t the\n CUP ") == tok.encode("hold the cup")
    assert tok.encode("cup &amp; bottle") == tok.encode("cup & bottle") == [merge(11), end("&"), merge(23)]
    assert tok.encode("cup &amp;amp; bottle") == tok.encode("cup & bottle")
    assert tok.clean("A  &lt;b&gt; ") == "a <b>"
    # the markers are pieces of their own, in any case
    assert tok.encode("cup <|endoftext|> hand") == [merge(11), EOT, sym("h"), merge(4)]
    assert tok.encode("<|STARTOFTEXT|>") == [SOT]


def test_non_ascii_is_rejected(tok):
    with pytest.raises(ValueError, match="caf"):
        tok.encode("pour the café")
    with pytest.raises(ValueError, match="non-ASCII"):
        tok.tokenize(["hold the cup", "naïve"])
    with pytest.raises(ValueError, match="ASCII"):
        tok.encode("caf&eacute;")


def test_tokenize_layout_truncation_and_overflow(tok):
    t = tok.tokenize(["hold the cup", "the"], context_length=8)
    assert t.dtype == np.int32 and t.shape == (2, 8)
    assert t[0].tolist() == [SOT, merge(14), merge(1), merge(11), EOT, 0, 0, 0] and t[1].tolist() == [SOT, merge(1), EOT, 0, 0, 0, 0, 0]
    assert np.array_equal(np.argmax(t, axis=1), [4, 2])
    assert tok.tokenize("the", context_length=5).shape == (1, 5)
    assert tok.tokenize(["the"]).shape == (1, 77)
    long = "zzzz the cup"  # 4 + 1 + 1 ids, 8 with the markers
    assert tok.token_count(long) == 8
    assert tok.tokenize([long], context_length=8)[0, -1] == EOT
    with pytest.raises(ValueError, match="8 tokens"):
        tok.tokenize([long], context_length=7)
    cut = tok.tokenize([long], context_length=6, truncate=True)[0]
    assert cut.tolist() == [SOT, sym("z"), sym("z"), sym("z"), end("z"), EOT]
    # a literal end marker inside the text becomes the EOT id: the first argmax - where the tower reads its output - is that one
    t = tok.tokenize(["cup <|endoftext|> hand"], context_length=10)[0]
    assert t.tolist() == [SOT, merge(11), EOT, sym("h"), merge(4), EOT, 0, 0, 0, 0] and int(np.argmax(t)) == 2


def test_txt_and_gz_give_the_same_table_and_max_merges_slices(tmp_path):
    gz = tmp_path / "merges.txt.gz"
    with open(BPE, "rb") as f, gzip.open(gz, "wb") as g:
        g.write(f.read())
    a, b = ClipTokenizer(BPE), ClipTokenizer(str(gz))
    assert a.encoder == b.encoder and a.bpe_ranks == b.bpe_ranks and a.vocab_size == b.vocab_size
    c = ClipTokenizer(BPE, max_merges=2)
    assert c.vocab_size == 512 + 2 + 2 and (c.sot_id, c.eot_id) == (514, 515) and list(c.bpe_ranks) == [("t", "h"), ("th", "e</w>")]
    assert c.encode("the hand") == [merge(1), sym("h"), sym("a"), sym("n"), end("d")]
    assert ClipTokenizer(BPE, max_merges=10 ** 6).vocab_size == a.vocab_size  # a shorter file gives all of its lines
    bad = tmp_path / "bad.txt"
    bad.write_text("#version\nt h\nonlyone\n")
    with pytest.raises(ValueError, match="bad.txt:3"):
        ClipTokenizer(str(bad))


def _naive_bpe(word, ranks):
    """textbook BPE on a list of symbols: while some adjacent pair has a rank, take the pair of lowest rank and join its occurrences
    scanning from the left"""
    word = list(word)
    while True:
        best = None
        for pair in zip(word, word[1:]):
            if pair in ranks and (best is None or ranks[pair] < ranks[best]):
                best = pair
        if best is None:
            return word
        out, i = [], 0
        while i < len(word):
            if word[i: i + 2] == list(best):
                out.append(best[0] + best[1])
                i += 2
            else:
                out.append(word[i])
                i += 1
        word = out


def test_agrees_with_a_naive_bpe_on_generated_ascii_strings(tok):
    import re

    merges = read_merges(BPE)
    ranks = {m: i for i, m in enumerate(merges)}
    vocab = [chr(b) for b in range(33, 127)]  # ASCII only: the symbols are the characters themselves
    rng = np.random.default_rng(7)
    alphabet = list("thehandcupholdtopourbottleonopenwithrightleftingander") + list(" '!?.,0123456789xyzs")
    n = 0
    for _ in range(300):
        text = "".join(rng.choice(alphabet, size=int(rng.integers(1, 30))))
        want = []
        # the split, restated for ASCII: 's 't 're 've 'm 'll 'd | letters | one digit | other non-space runs
        for piece in re.findall(r"'s|'t|'re|'ve|'m|'ll|'d|[a-z]+|[0-9]|[^\sa-z0-9]+", " ".join(text.split()).lower()):
            symbols = _naive_bpe(list(piece[:-1]) + [piece[-1] + "</w>"], ranks)
            for s in symbols:
                if s in ("".join(m) for m in merges):
                    want.append(512 + [("".join(m)) for m in merges].index(s))
                elif s.endswith("</w>"):
                    want.append(256 + vocab.index(s[:-4]))
                else:
                    want.append(vocab.index(s))
        assert tok.encode(text) == want, text
        n += len(want)
    assert n > 2000
