#!/bin/bash
# Signed distance files of objects from mesh files on MI355X: the reference's SDFData pickles (sdf_util.load_sdf_data), made without pysdf
# by the exact point-to-mesh distance and the inside test of SIV.  Not a speed cache: voxelising is milliseconds.
#
#   script/process_object_sdf.sh [-n] <mesh prefix> [extra launcher flags ...]
#
# Reads <mesh prefix>/<obj_id>.{obj,ply,stl} (or the single mesh file in <mesh prefix>/<obj_id>/) and writes
# common/retrieve_obj_sdf/main/sdf/<obj_id>.pkl, which script/compute_score_siv.sh --data.obj_sdf_prefix takes as it is (--out_dir,
# --obj_ids, --resolution, --bbox_expand_ratio, --overwrite, --dry_run, --out_json change that).
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
    echo "usage: script/process_object_sdf.sh [-n] <mesh prefix> [extra flags]" >&2
    exit 2
fi
prefix="$1"; shift 1
printf 'mesh prefix: %s\n' "$prefix"

cmd=(python -m oakink2_tamf_amd.launch.process_object_sdf "$prefix" "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
