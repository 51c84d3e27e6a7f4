#!/bin/bash
# FID of the refined samples on MI355X: stands where the reference's script/compute_score/compute_score_fid.py is run by hand.
#
#   script/compute_score_fid.sh [-n] <split> <encoder checkpoint> <model_name> [extra launcher flags ...]
#
# Scores the samples that script/sample_refine.sh left under common/sample_refine/main/sample/<split>/<model_name> against the split's
# ground truth (the split's process range and segment cache), with the SegmentEncoder of config/arch_encoder.yml.
# -n prints the command and exits (dry run).
set -u
here="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
dry=0
while [ $# -gt 0 ]; do
    case "$1" in
        -n|--dry-run) dry=1; shift ;;
        -h|--help) sed -n '2,8p' "${BASH_SOURCE[0]}" | sed 's/^# \{0,1\}//'; exit 0 ;;
        *) break ;;
    esac
done
if [ $# -lt 3 ]; then
    echo "usage: script/compute_score_fid.sh [-n] <split> <encoder checkpoint> <model_name> [extra flags]" >&2
    exit 2
fi
split="$1"; weight="$2"; name="$3"; shift 3
printf 'split:      %s\nencoder:    %s\nmodel_name: %s\n' "$split" "$weight" "$name"

cmd=(python -m oakink2_tamf_amd.launch.compute_score_fid
     --cfg "$here/config/arch_encoder.yml"
     --data.process_range "?(file:./asset/split/$split.txt)"
     --debug.cache_dict_filepath "common/save_cache_dict/main/cache/$split.pkl"
     --debug.sample_refine_filepath "common/sample_refine/main/sample/$split/$name"
     --debug.encoder_checkpoint_filepath "$weight" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
