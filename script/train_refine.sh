#!/bin/bash
# Train the refiner R on MI355X: stands where the reference's script/train_refine.sh is run.
#
#   script/train_refine.sh [-n] [extra launcher flags ...]
#
# The reference's command line (the G stage's samples of the train cache plus their Gaussian perturbation, arch_mdm as its script
# names it, the loss coefficients of its loss_param_refine.yml, batch 64, --commit) on one device: the reference's world batch of 64
# over 4 GPUs is one batch of 64 here.  MANO from MANO_RIGHT.npz / MANO_LEFT.npz under asset/mano_npz (tools/mano_pkl_to_npz.py).
# Checkpoints land under common/train_refine/<exp_id>/save/ and are what script/sample_refine.sh takes.
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

cmd=(python -m oakink2_tamf_amd.launch.train_refine
     --cfg "$here/config/obj_embedding.yml"
     --cfg "$here/config/obj_pointcloud.yml"
     --cfg "$here/config/arch_mdm.yml"
     --train.cache_dict_filepath common/save_cache_dict/main/cache/train.pkl
     --val.cache_dict_filepath common/save_cache_dict/main/cache/val.pkl
     --test.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl
     --train.data.pose_repr_sample_dir_list common/sample/main/sample/train/arch_mdm_l__0099
     --train.data.gaussian_perturb_range 0.02,0.1
     --val.data.pose_repr_sample_dir_list common/sample/main/sample/val/arch_mdm_l__0399
     --test.data.pose_repr_sample_dir_list common/sample/main/sample/test/arch_mdm_l__0399
     --train.loss.c_weight_path asset/grabnet/rhand_weight.npy
     --train.loss.coef_rec_joint_loss 1.0
     --train.loss.coef_rec_vert_loss 1.0
     --train.loss.coef_dist_h_loss 0.1
     --mano.factory oakink2_tamf_amd.mano:make_mano_differentiable
     --mano.mano_path asset/mano_npz
     --train.batch_size 64
     --runtime.device_id 0
     --val.val_freq 20 --test.test_freq 40
     --exp_id "refine__?(ts)"
     --commit "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
