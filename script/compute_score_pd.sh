#!/bin/bash
# Penetration depth of the refined samples on MI355X (the reference ships no such script): how deep the hand goes into the objects.
#
#   script/compute_score_pd.sh [-n] <split> <model_name> [extra launcher flags ...]
#
# Measures the samples that script/sample_refine.sh left under common/sample_refine/main/sample/<split>/<model_name> and the split's
# ground truth against the object meshes (every 20th frame; --stride changes that), in cm.  The MANO layers come through --mano.factory module:function and the
# object meshes through --data.obj_model_loader module:function (pass both among the extra flags).  -n prints the command and exits.
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
if [ $# -lt 2 ]; then
    echo "usage: script/compute_score_pd.sh [-n] <split> <model_name> [extra flags]" >&2
    exit 2
fi
split="$1"; name="$2"; shift 2
printf 'split:      %s\nmodel_name: %s\n' "$split" "$name"

cmd=(python -m oakink2_tamf_amd.launch.compute_score_pd
     --data.process_range "?(file:./asset/split/$split.txt)"
     --data.cache_dict_filepath "common/save_cache_dict/main/cache/$split.pkl"
     --debug.sample_refine_filepath "common/sample_refine/main/sample/$split/$name" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
