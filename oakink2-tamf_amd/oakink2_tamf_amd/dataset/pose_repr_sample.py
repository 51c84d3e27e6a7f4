"""G-stage samples joined to their dataset items: the input of the R stage (reference dataset/pose_repr_sample.py:18-52,
97-108).

`launch/sample.py:234-237` leaves one `<sample_id:06d>.npy` (T, 99) float32 per dataset index under
`<cwd>/common/sample/<exp_id>/sample/<offset>/`; `launch/sample_refine.py:168-171` wraps the dataset in
`GeneratedPoseReprSampleAdaptor(dataset, [<that directory>, ...])`, whose item i is dataset item i plus

    sample_info       (basename of the directory, sample_id)
    sample_pose_repr  the array of the i-th .npy file, files taken directory by directory in sorted name order

The join is positional: the number of .npy files must equal the number of dataset items (the reference asserts it).

`GuassianPerturbSampleAdaptor` (the reference's spelling, :55-94) is the third part of the encoder's training set: the item's own pose
with Gaussian noise on its valid frames, the rot6d halves renormalised."""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import numpy as np


def list_sample_files(dir_list: Sequence[str]) -> List[Tuple[Tuple[str, int], str]]:
    """[((dir basename, sample id), path)] in the adaptor's order"""
    out = []
    for d in dir_list:
        base = os.path.basename(d)
        for name in sorted(n for n in os.listdir(d) if os.path.splitext(n)[-1] == ".npy"):
            out.append(((base, int(os.path.splitext(name)[0])), os.path.join(d, name)))
    return out


class GeneratedPoseReprSampleAdaptor:
    def __init__(self, interaction_segment_dataset, dir_list: Sequence[str]):
        self.interaction_segment_dataset = interaction_segment_dataset
        self.dir_list = list(dir_list)
        files = list_sample_files(self.dir_list)
        if len(files) != len(interaction_segment_dataset):
            raise AssertionError(f"{len(files)} generated samples under {self.dir_list} for {len(interaction_segment_dataset)} "
                                 "dataset items: the G stage must have sampled every clip of the cache dict")
        self.pose_repr_info_list = [info for info, _ in files]
        self.pose_repr_map = {info: np.load(path) for info, path in files}
        self.len = len(files)

    def __getitem__(self, index: int) -> Dict:
        item = self.interaction_segment_dataset[index]
        info = self.pose_repr_info_list[index]
        item["sample_info"] = info
        item["sample_pose_repr"] = self.pose_repr_map[info]
        return item

    def __len__(self) -> int:
        return self.len


class GuassianPerturbSampleAdaptor:
    """item i with a noisy copy of its pose as the "sample": sigma ~ U(sigma_range); on the item's first `len` frames the translation
    (columns 0:3) gets N(0, 0.1 sigma) and the 16 rot6d poses (columns 3:99) get N(0, sigma), then each 3-vector half of every rot6d
    is scaled back to unit length (norms clamped at 1e-7).  Frames past `len` are untouched.  np.random is called as the reference
    calls it - uniform, normal (len, 3), normal (len, 96) - so a seeded run draws the same noise.
    sample_info = (index, sigma)."""

    def __init__(self, interaction_segment_dataset, sigma_range: Sequence[float]):
        self.interaction_segment_dataset = interaction_segment_dataset
        self.sigma_min, self.sigma_max = float(sigma_range[0]), float(sigma_range[1])

    def __getitem__(self, index: int) -> Dict:
        item = self.interaction_segment_dataset[index]
        n = int(item["len"])
        sigma = np.random.uniform(self.sigma_min, self.sigma_max)
        d_tsl = np.random.normal(0, 0.1 * sigma, size=(n, 3))
        d_rot = np.random.normal(0, sigma, size=(n, 96))
        out = item["pose_repr"].copy()
        out[:n, 0:3] += d_tsl
        out[:n, 3:99] += d_rot
        halves = out[:n, 3:99].reshape(n, 32, 3)  # 16 joints x (first, second) column of the rotation
        halves = halves / np.maximum(np.linalg.norm(halves, axis=-1, keepdims=True), 1e-7)
        out[:n, 3:99] = halves.reshape(n, 96)
        item["sample_info"] = (index, sigma)
        item["sample_pose_repr"] = out
        return item

    def __len__(self) -> int:
        return len(self.interaction_segment_dataset)


class IdentitySampleAdaptor:
    """item i with its own ground-truth pose as the "sample" (:97-108; the R stage's sanity input)"""

    def __init__(self, interaction_segment_dataset):
        self.interaction_segment_dataset = interaction_segment_dataset
        self.len = len(interaction_segment_dataset)

    def __getitem__(self, index: int) -> Dict:
        item = self.interaction_segment_dataset[index]
        item["sample_info"] = None
        item["sample_pose_repr"] = item["pose_repr"]
        return item

    def __len__(self) -> int:
        return self.len
