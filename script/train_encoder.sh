#!/bin/bash
# Train the FID encoder on MI355X: stands where the reference's script/train_encoder.sh is run.
#
#   script/train_encoder.sh [-n] [extra launcher flags ...]
#
# The reference's command line (its presets, 400 epochs, milestones 80,160,240,320, validation and test every 20 epochs, --commit) on
# one device: the reference's world batch of 256 over 4 GPUs is one batch of 256 here.  Checkpoints land under
# common/train_encoder/<exp_id>/save/ and are what script/compute_score_fid.sh takes as its encoder checkpoint.
# -n prints the command and exits (dry run).
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

cmd=(python -m oakink2_tamf_amd.launch.train_encoder
     --cfg "$here/config/obj_embedding.yml"
     --cfg "$here/config/obj_pointcloud.yml"
     --cfg "$here/config/arch_encoder.yml"
     --train.cache_dict_filepath common/save_cache_dict/main/cache/train.pkl
     --val.cache_dict_filepath common/save_cache_dict/main/cache/val.pkl
     --test.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl
     --train.data.pose_repr_sample_dir_list common/sample/main/sample/train/arch_mdm_l__0099
     --train.data.gaussian_perturb_range 0.02,0.1
     --train.batch_size 256
     --train.num_epoch 400
     --train.scheduler_milestone 80,160,240,320
     --runtime.num_worker 0
     --runtime.device_id 0
     --val.val_freq 20 --test.test_freq 20
     --exp_id "encoder__?(ts)"
     --commit "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
