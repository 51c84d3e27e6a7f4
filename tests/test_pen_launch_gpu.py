"""launch/train.py and launch/train_refine.py with `--train.loss.coef_pen_loss 1 --data.obj_sdf_prefix DIR` end to end on the MI355X,
as subprocesses under a time limit: 2 epochs on the synthetic tree of tests/train_launch_fixture.py.  The pickles are made here with
meshdist.process_sdf on the sphere mesh of tests/golden/siv_lattice_sphere.npz, scaled to half a metre, at resolution 16, for every object of the cache but the
first, which therefore runs as an object without a lattice.

That the term is OFF without the flags - no lattice set built, no sdf_grid_id collated - is checked once, device-free, in
tests/test_pen_launch_cpu.py; a second training run for "off" would only compare the parent with itself."""
import math
import os
import pickle
import re
import subprocess
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import meshdist_cases as MC  # noqa: E402
import train_launch_fixture as F  # noqa: E402
from test_pen_launch_cpu import object_ids  # noqa: E402

pytestmark = pytest.mark.gpu
EPOCHS = 2
LIMIT = 240  # seconds per child


@pytest.fixture(scope="module")
def sdf_fields():
    from oakink2_tamf_amd import meshdist

    v, f = MC.fixture_mesh("sphere")
    v = v * (0.5 / float(abs(v).max()))  # half a metre: the synthetic hands, wherever they are, have a chance to lie inside
    fields, info = meshdist.process_sdf(v, f, resolution=16, device="cuda:0", info=True)
    assert info["n_inside"] > 0
    return fields


@pytest.mark.parametrize("prog", ["train", "train_refine"])
def test_two_epochs_with_the_pen_term(prog, sdf_fields, tmp_path):
    import torch

    cwd = str(tmp_path)
    paths = F.write_tree(cwd)
    ids = object_ids(paths)
    prefix = os.path.join(cwd, "sdf")
    os.makedirs(prefix)
    for oid in ids[1:]:
        with open(os.path.join(prefix, f"{oid}.pkl"), "wb") as fh:
            pickle.dump(dict(sdf_fields), fh, protocol=4)
    cmd = F.launcher_cmd(prog, paths, "--train.num_epoch", str(EPOCHS), "--exp_id", "pen", "--commit", "--train.loss.coef_pen_loss", "1",
                         "--data.obj_sdf_prefix", prefix)
    r = subprocess.run(cmd, capture_output=True, text=True, env=F.launcher_env(), cwd=cwd, timeout=LIMIT)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-4000:]
    assert "pen: 1 of the cache's objects have no file" in log
    pens = [float(m) for m in re.findall(r"^\s+pen\s*: (\S+)$", log, flags=re.M)]
    print(f"{prog}: pen per epoch {pens}")
    assert len(pens) == EPOCHS and all(math.isfinite(p) and p >= 0.0 for p in pens)
    save = os.path.join(cwd, "common", prog, "pen", "save")
    assert sorted(os.listdir(save)) == ["model_0000.pt", "model_0001.pt", "optimizer_0000.pt", "optimizer_0001.pt"]
    sd = torch.load(os.path.join(save, "model_0001.pt"), map_location="cpu")
    assert all(torch.isfinite(v).all() for v in sd.values())
    arch = dict(latent_dim=128, ff_size=256, num_layers=2, num_heads=2)
    if prog == "train":
        from oakink2_tamf_amd.model.interaction_segment_mdm import InterationSegmentMDM

        module = InterationSegmentMDM(**arch)
    else:
        from oakink2_tamf_amd.model.segment_refine_model import SegmentRefineModel

        module = SegmentRefineModel(None, **arch, use_pc=True)
    missing, unexpected = module.load_state_dict(sd, strict=False)
    assert not unexpected and not [k for k in missing if not k.startswith("clip_model")]
