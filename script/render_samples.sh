#!/bin/bash
# Pictures of the refined samples on MI355X: stands where the reference's viewers (script/viz_seg.py, script/debug/debug_refine_sample.py)
# open a window.
#
#   script/render_samples.sh [-n] <split> <model_name> [extra launcher flags ...]
#
# Renders the samples that script/sample_refine.sh left under common/sample_refine/main/sample/<split>/<model_name>, hand and objects,
# frame by frame to common/render_samples/main/<split>/<model_name>/<clip>/frame_NNNN.png and sheet.png.  Objects are drawn as meshes
# with --data.obj_model_loader module:function, else as point clouds; --with_gt --mano.factory module:function adds the ground-truth
# hand in a second panel (pass them among the extra flags).  -n prints the command and exits (dry run).
set -u
here="$(cd "$(dirname "${BASH_SOURCE[0]}")/.." && pwd)"
dry=0
while [ $# -gt 0 ]; do
    case "$1" in
        -n|--dry-run) dry=1; shift ;;
        -h|--help) sed -n '2,10p' "${BASH_SOURCE[0]}" | sed 's/^# \{0,1\}//'; exit 0 ;;
        *) break ;;
    esac
done
if [ $# -lt 2 ]; then
    echo "usage: script/render_samples.sh [-n] <split> <model_name> [extra flags]" >&2
    exit 2
fi
split="$1"; name="$2"; shift 2
printf 'split:      %s\nmodel_name: %s\n' "$split" "$name"

cmd=(python -m oakink2_tamf_amd.launch.render_samples
     --data.process_range "?(file:./asset/split/$split.txt)"
     --data.cache_dict_filepath "common/save_cache_dict/main/cache/$split.pkl"
     --debug.sample_refine_filepath "common/sample_refine/main/sample/$split/$name"
     --out_dir "common/render_samples/main/$split/$name" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
