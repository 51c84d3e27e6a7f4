#!/bin/bash
# Object embeddings from point clouds on MI355X: the native PointBERT point encoder (the reference ships no script for this step).
#
#   script/embed_objects.sh [-n] <point encoder checkpoint> [extra launcher flags ...]
#
# Reads common/retrieve_obj_pointcloud/main/pointcloud/<obj_id>.npz and writes common/retrieve_obj_embedding/main/embedding/<obj_id>.pt,
# the files script/sample.sh reads (--data.obj_pointcloud_prefix, --out_dir, --obj_ids, --color r,g,b, --pc_norm, --seed change that).
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
if [ $# -lt 1 ]; then
    echo "usage: script/embed_objects.sh [-n] <point encoder checkpoint> [extra flags]" >&2
    exit 2
fi
weight="$1"; shift 1
printf 'point encoder: %s\n' "$weight"

cmd=(python -m oakink2_tamf_amd.launch.embed_objects --point_encoder.ckpt "$weight" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
