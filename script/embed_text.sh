#!/bin/bash
# Text embeddings from prompts on MI355X: the native CLIP text tower (the reference runs the `clip` package inside the model instead).
#
#   script/embed_text.sh [-n] <ViT-B-32.pt> <bpe vocab file> [--data.cache_dict_filepath PKL | --text_file FILE] [--out FILE]
#                        [--max_text_len 20] [--no_round_fp16] [--batch_size 256] [--device cuda:0] [--dry_run]
#
# Reads the distinct prompts of common/save_cache_dict/main/cache/test.pkl (or one prompt per line of --text_file) and writes
# common/embed_text/main/text_embedding.pkl, {text: (512,) float32}: the file script/sample.sh takes as --data.text_embedding_filepath.
# --dry_run lists prompts, token counts and truncations (no GPU, no checkpoint).  -n prints the command and exits.
set -u
here="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
dry=0
while [ $# -gt 0 ]; do
    case "$1" in
        -n|--dry-run) dry=1; shift ;;
        -h|--help) sed -n '2,9p' "${BASH_SOURCE[0]}" | sed 's/^# \{0,1\}//'; exit 0 ;;
        *) break ;;
    esac
done
if [ $# -lt 2 ]; then
    echo "usage: script/embed_text.sh [-n] <ViT-B-32.pt> <bpe vocab file> [extra flags]" >&2
    exit 2
fi
weight="$1"; vocab="$2"; shift 2
printf 'text tower: %s\nvocabulary: %s\n' "$weight" "$vocab"

cmd=(python -m oakink2_tamf_amd.launch.embed_text --text_encoder.ckpt "$weight" --text_encoder.vocab "$vocab" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
