"""A synthetic training tree for launch/train.py and launch/train_refine.py: oracle.fixtures' segment cache, object embeddings, point
clouds and prompt-embedding table at 16 frames, one generated sample per segment in the layout launch/sample.py leaves, the MANO-shaped
arrays of tests/mano_fixture.py written as MANO_RIGHT.npz / MANO_LEFT.npz, and seeded stand-ins for the two loss assets."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oakink2-tamf_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

FRAMES, SEGMENTS, BATCH = 16, 6, 2
TINY = ["--model.latent_dim", "128", "--model.ff_size", "256", "--model.num_layers", "2", "--model.num_heads", "2"]
COEFS = {"train": {"coef_rec_joint_loss": 1.0, "coef_rec_vert_loss": 1.0, "coef_edge_len_loss": 0.1, "coef_dist_h_loss": 0.1, "coef_dist_o_loss": 1.0},
         "train_refine": {"coef_rec_joint_loss": 1.0, "coef_rec_vert_loss": 1.0, "coef_dist_h_loss": 0.1}}


def write_tree(root: str, mano: bool = True):
    """-> paths: cache, emb, pc, text (oracle.fixtures.write_synthetic_dataset), samples, mano (a directory), vpe, c_weight"""
    from oracle.fixtures import synthetic_sample_pose_repr, write_synthetic_dataset

    paths, _ = write_synthetic_dataset(root, n_segments=SEGMENTS, max_len=FRAMES)
    paths["samples"] = os.path.join(root, "common", "sample", "main", "sample", "train", "arch_mdm_l__0099")
    os.makedirs(paths["samples"], exist_ok=True)
    for i in range(SEGMENTS):
        np.save(os.path.join(paths["samples"], f"{i:06d}.npy"), synthetic_sample_pose_repr("train", i, FRAMES))
    asset = os.path.join(root, "asset")
    os.makedirs(asset, exist_ok=True)
    rng = np.random.default_rng(5)
    paths["c_weight"], paths["vpe"] = os.path.join(asset, "rhand_weight.npy"), os.path.join(asset, "verts_per_edge.npy")
    np.save(paths["c_weight"], rng.uniform(0.5, 1.5, size=778).astype(np.float32))
    np.save(paths["vpe"], np.stack([rng.permutation(778)[:96], rng.permutation(778)[:96]], axis=1).astype(np.int64))
    paths["mano"] = os.path.join(asset, "mano_npz")
    if mano:
        import mano_fixture as MF
        from oakink2_tamf_amd.mano import ManoArrays

        os.makedirs(paths["mano"], exist_ok=True)
        for name, seed in (("MANO_RIGHT.npz", 3), ("MANO_LEFT.npz", 4)):
            ManoArrays(**MF.synthetic_arrays(778, seed)).to_npz(os.path.join(paths["mano"], name))
    return paths


def launcher_cmd(prog: str, paths, *extra):
    """the command line of one launcher on the tree: tiny architecture, batch 2, every loss coefficient positive"""
    cmd = [sys.executable, "-m", f"oakink2_tamf_amd.launch.{prog}", "--train.cache_dict_filepath", paths["cache"], "--val.cache_dict_filepath", paths["cache"],
           "--data.obj_embedding_prefix", paths["emb"], "--data.obj_pointcloud_prefix", paths["pc"], "--train.batch_size", str(BATCH),
           "--train.loss.vpe_path", paths["vpe"], "--train.loss.c_weight_path", paths["c_weight"],
           "--mano.factory", "oakink2_tamf_amd.mano:make_mano_differentiable", "--mano.mano_path", paths["mano"], *TINY]
    for k, v in COEFS[prog].items():
        cmd += [f"--train.loss.{k}", str(v)]
    if prog == "train":
        cmd += ["--data.text_embedding_filepath", paths["text"]]
    else:
        cmd += ["--train.data.pose_repr_sample_dir_list", paths["samples"], "--train.data.gaussian_perturb_range", "0.02,0.1"]
    return cmd + list(extra)


def launcher_env():
    return dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT, os.path.join(ROOT, "oakink2-tamf_amd")]))
