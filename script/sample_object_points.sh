#!/bin/bash
# Object point clouds from mesh files on MI355X: the bit-defined HIP surface sampler + farthest-point sampling (the reference ships no
# script for this step; its clouds come from a retrieve_obj_pointcloud step that is not published).
#
#   script/sample_object_points.sh [-n] <mesh prefix> [extra launcher flags ...]
#
# Reads <mesh prefix>/<obj_id>.{obj,ply,stl} (or the single mesh file in <mesh prefix>/<obj_id>/) and writes
# common/retrieve_obj_pointcloud/main/pointcloud/<obj_id>.npz, the files script/embed_objects.sh and the refiner read (--out_dir,
# --obj_ids, --n_points, --oversample, --seed, --scale, --with_normals, --from_points, --overwrite, --dry_run, --out_json change that).
# -n prints the command and exits (dry run).
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
if [ $# -lt 1 ]; then
    echo "usage: script/sample_object_points.sh [-n] <mesh prefix> [extra flags]" >&2
    exit 2
fi
prefix="$1"; shift 1
printf 'mesh prefix: %s\n' "$prefix"

cmd=(python -m oakink2_tamf_amd.launch.sample_object_points "$prefix" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
