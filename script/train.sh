#!/bin/bash
# Train the denoiser G on MI355X: stands where the reference's script/train.sh is run.
#
#   script/train.sh [-n] [extra launcher flags ...]
#
# The reference's command line (reversed segments appended, arch_mdm_l, the loss coefficients of its loss_param.yml, batch 64,
# validation and test off, --commit) on one device: the reference's world batch of 64 over 4 GPUs is one batch of 64 here.
# The prompt embeddings come from script/embed_text.sh run over the train cache; MANO from MANO_RIGHT.npz / MANO_LEFT.npz under
# asset/mano_npz (tools/mano_pkl_to_npz.py).  Checkpoints land under common/train/<exp_id>/save/ and are what script/sample.sh takes.
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

cmd=(python -m oakink2_tamf_amd.launch.train
     --cfg "$here/config/obj_embedding.yml"
     --cfg "$here/config/obj_pointcloud.yml"
     --cfg "$here/config/arch_mdm_l.yml"
     --data.append_reverse_segment
     --train.cache_dict_filepath common/save_cache_dict/main/cache/train.pkl
     --val.cache_dict_filepath common/save_cache_dict/main/cache/val.pkl
     --test.cache_dict_filepath common/save_cache_dict/main/cache/test.pkl
     --data.text_embedding_filepath common/embed_text/main/text_embedding.pkl
     --train.loss.vpe_path asset/grabnet/verts_per_edge.npy
     --train.loss.c_weight_path asset/grabnet/rhand_weight.npy
     --train.loss.coef_rec_joint_loss 1.0
     --train.loss.coef_rec_vert_loss 1.0
     --train.loss.coef_edge_len_loss 0.1
     --train.loss.coef_dist_h_loss 0.1
     --train.loss.coef_dist_o_loss 1.0
     --mano.factory oakink2_tamf_amd.mano:make_mano_differentiable
     --mano.mano_path asset/mano_npz
     --train.batch_size 64
     --runtime.device_id 0
     --val.val_freq -1 --test.test_freq -1
     --exp_id "main__?(ts)"
     --commit "$@")

if [ "$dry" = 1 ]; then
    printf '%q ' "${cmd[@]}"; echo
    exit 0
fi
export PYTHONPATH="$here/oakink2-tamf_amd${PYTHONPATH:+:$PYTHONPATH}"
exec "${cmd[@]}"
