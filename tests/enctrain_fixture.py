"""A synthetic training tree for launch/train_encoder.py: oracle.fixtures' segment cache with its primitive names replaced by names
of the action list (the adapter looks the label up there), and one generated sample per segment in the layout launch/sample.py
leaves (<dir>/<sample_id:06d>.npy)."""
import os
import pickle
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def write_training_tree(root: str, n_segments: int = 6, max_len: int = 24):
    """-> (paths of oracle.fixtures.write_synthetic_dataset + "samples": the generated-sample directory, n_segments)"""
    from oakink2_tamf_amd.dataset.action_adapter import ACTION_LIST
    from oracle.fixtures import synthetic_sample_pose_repr, write_synthetic_dataset

    paths, cache = write_synthetic_dataset(root, n_segments=n_segments, max_len=max_len)
    infos = cache["interaction_segment_info_list"]
    cache["interaction_segment_info_list"] = [(a, f"{ACTION_LIST[(7 * i) % len(ACTION_LIST)]}:{b}", c) for i, (a, b, c) in enumerate(infos)]
    with open(paths["cache"], "wb") as f:
        pickle.dump(cache, f)
    paths["samples"] = os.path.join(root, "common", "sample", "main", "sample", "train", "arch_mdm_l__0099")
    os.makedirs(paths["samples"], exist_ok=True)
    for i in range(n_segments):
        np.save(os.path.join(paths["samples"], f"{i:06d}.npy"), synthetic_sample_pose_repr("train", i, max_len))
    return paths, n_segments


def launcher_cmd(paths, *extra):
    return [sys.executable, "-m", "oakink2_tamf_amd.launch.train_encoder", "--cfg", os.path.join(ROOT, "config", "arch_encoder.yml"),
            "--train.cache_dict_filepath", paths["cache"], "--val.cache_dict_filepath", paths["cache"], "--data.obj_embedding_prefix", paths["emb"],
            "--data.obj_pointcloud_prefix", paths["pc"], "--train.data.pose_repr_sample_dir_list", paths["samples"], *extra]


def launcher_env():
    return dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd")]))
