"""Text embeddings from prompts: the distinct `text` strings of a segment cache (or one prompt per line of a file) ->
a pickle `{text: np.ndarray (512,) float32}`, the file `launch/sample.py --data.text_embedding_filepath` reads.  The encoder is
model/text_encoder.py (CLIP's text tower, native HIP) with model/clip_tokenizer.py; neither its weights nor its vocabulary are
shipped: the first argument is OpenAI's `ViT-B-32.pt` archive (or a torch.save'd state dict of the text tower), the second the
merges file `bpe_simple_vocab_16e6.txt.gz`.

Every prompt is encoded as the reference does (model/interaction_segment_mdm.py:118-132): tokenised at max_text_len + 2 ids with
truncation, zero-padded to the model's context.  `--dry_run` lists the prompts, their token counts and which ones get truncated;
it needs the vocabulary file only - no GPU, no checkpoint."""
from __future__ import annotations

import argparse
import os
import pickle
from typing import List, Optional

import numpy as np

from .sample import DEFAULT_CACHE_DICT, _abspath

DEFAULT_OUT = os.path.join("common", "embed_text", "main", "text_embedding.pkl")


def make_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="oakink2_tamf_amd.launch.embed_text", allow_abbrev=False)
    ap.add_argument("--text_encoder.ckpt", dest="ckpt", default=None, help="ViT-B-32.pt (TorchScript archive) or a state dict of the text tower")
    ap.add_argument("--text_encoder.vocab", dest="vocab", default=None, help="the BPE merges file (.txt or .txt.gz)")
    ap.add_argument("--text_encoder.cfg", dest="cfg", default=None,
                    help="yaml with the tower's fields (vocab_size, context_length, width, num_heads, num_layers, embed_dim); default: ViT-B/32")
    ap.add_argument("--data.cache_dict_filepath", dest="cache", default=None, help=f"segment cache (default {DEFAULT_CACHE_DICT})")
    ap.add_argument("--text_file", default=None, help="one prompt per line, instead of the cache")
    ap.add_argument("--out", default=DEFAULT_OUT)
    ap.add_argument("--max_text_len", type=int, default=20)
    ap.add_argument("--no_round_fp16", action="store_true", help="keep the Linear / attention parameters as stored (default: rounded to fp16, as the reference's convert_weights)")
    ap.add_argument("--batch_size", type=int, default=256, help="prompts per encoder call (no output bit depends on it)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--dry_run", action="store_true", help="list the prompts and exit (no GPU, no checkpoint)")
    return ap


def load_cfg(path: Optional[str]):
    from ..model.text_encoder import make_cfg

    if path is None:
        return make_cfg()
    import yaml

    with open(path) as f:
        y = yaml.safe_load(f) or {}
    return make_cfg(y.get("model", y))


def cache_prompts(path: str) -> List[str]:
    """the distinct prompts of a segment cache (`save_cache_dict` output: interaction_segment_text_list), sorted"""
    with open(path, "rb") as f:
        cache = pickle.load(f)
    if not isinstance(cache, dict) or "interaction_segment_text_list" not in cache:
        raise SystemExit(f"embed_text: {path}: no interaction_segment_text_list")
    return sorted({str(t) for t in cache["interaction_segment_text_list"]})


def file_prompts(path: str) -> List[str]:
    """one prompt per line, in file order, repeats and empty lines dropped"""
    seen, out = set(), []
    with open(path, encoding="utf-8") as f:
        for ln in f.read().split("\n"):
            if ln.strip() != "" and ln not in seen:
                seen.add(ln)
                out.append(ln)
    return out


def save_table(path: str, prompts: List[str], emb: np.ndarray) -> None:
    """{text: (E,) float32} as launch/sample.py:load_text_embeddings reads it"""
    emb = np.asarray(emb, dtype=np.float32)
    if emb.shape[0] != len(prompts) or emb.ndim != 2:
        raise ValueError(f"{len(prompts)} prompts, embeddings of shape {emb.shape}")
    for t, e in zip(prompts, emb):
        if not np.isfinite(e).all():
            raise ValueError(f"the embedding of {t!r} holds a non-finite value")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        pickle.dump({t: np.array(e, dtype=np.float32) for t, e in zip(prompts, emb)}, f)


def main(argv=None) -> int:
    a = make_parser().parse_args(argv)
    if a.vocab is None:
        raise SystemExit("embed_text: --text_encoder.vocab is required (the BPE merges file is not shipped)")
    if a.text_file is not None and a.cache is not None:
        raise SystemExit("embed_text: give --data.cache_dict_filepath or --text_file, not both")
    cfg = load_cfg(a.cfg)
    prompts = file_prompts(_abspath(a.text_file)) if a.text_file is not None else cache_prompts(_abspath(a.cache or DEFAULT_CACHE_DICT))
    if not prompts:
        raise SystemExit("embed_text: no prompts")
    from ..model.clip_tokenizer import ClipTokenizer

    tok = ClipTokenizer(_abspath(a.vocab), max_merges=cfg["vocab_size"] - 514)
    if tok.vocab_size > cfg["vocab_size"]:
        raise SystemExit(f"embed_text: the vocabulary has {tok.vocab_size} entries, the model {cfg['vocab_size']}")
    limit = min(a.max_text_len + 2, cfg["context_length"])
    try:
        counts = [tok.token_count(t) for t in prompts]
    except ValueError as e:
        raise SystemExit(f"embed_text: {e}")
    out = _abspath(a.out)
    if a.dry_run:
        import json

        print(json.dumps({"cfg": cfg, "out": out, "max_text_len": a.max_text_len, "round_fp16": not a.no_round_fp16, "vocab_size": tok.vocab_size,
                          "prompts": [{"text": t, "tokens": n, "truncated": n > limit} for t, n in zip(prompts, counts)]}, indent=1))
        return 0
    if a.ckpt is None:
        raise SystemExit("embed_text: --text_encoder.ckpt is required (the tower's weights are not shipped)")
    from ..model.text_encoder import HipClipTextEncoder

    enc = HipClipTextEncoder(cfg, device=a.device, round_fp16=not a.no_round_fp16)
    enc.load_checkpoint(_abspath(a.ckpt))
    emb = []
    for s in range(0, len(prompts), max(1, a.batch_size)):
        emb.append(enc.encode_text(prompts[s: s + max(1, a.batch_size)], tok, max_text_len=a.max_text_len).cpu().numpy())
    enc.close()
    try:
        save_table(out, prompts, np.concatenate(emb))
    except ValueError as e:
        raise SystemExit(f"embed_text: {e}")
    print(f"{len(prompts)} prompts ({sum(n > limit for n in counts)} truncated): {out}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
