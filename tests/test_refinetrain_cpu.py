"""The refiner's training step without a device: the float64 restatement of the training forward (tests/refine_train_restatement.py)
held to oracle.mdm_oracle.refine_forward at p = 0 and, through its autograd, to every tests/golden/refinetrain_*.npz fixture (the
reference's own module and loss); the Python-side refusals; the description of libtamf_refinetrain.so in _lib."""
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refine_train_restatement as R  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
TRUNK_FIXTURES = ("refinetrain_tiny.npz", "refinetrain_l1_ff16.npz", "refinetrain_deep.npz")


@pytest.mark.parametrize("arch,B,T,nobj,ragged", [(R.ARCH_L1, 1, 1, 1, False), (R.ARCH_TINY, 3, 14, 2, True), (R.ARCH_TINY, 2, 5, 3, False),
                                                  (R.ARCH_DEEP, 2, 13, 2, True)])
def test_restatement_equals_oracle(arch, B, T, nobj, ragged):
    """p = 0: the restatement is oracle.mdm_oracle.refine_forward in float64 to 1e-12 (padded and ragged object means)"""
    sd = R.leaf_state_dict(R.seeded_state_dict(arch, 3))
    inp, obj_num = R.seeded_inputs(arch, B, T, nobj, 4, ragged)
    x, h = torch.from_numpy(inp["sample_pose_repr"]).double(), torch.from_numpy(inp["h2o_dist"]).double()
    with torch.no_grad():
        a = R.refine_train_forward(sd, arch, x, h, R.cond_of(inp), obj_num=obj_num)
        b = R.oracle_forward(sd, arch, x, h, inp, torch.float64, obj_num)
    assert float((a - b).abs().max()) <= 1e-12


def test_restatement_masks_scale_and_drop():
    """an all-true mask at p scales by 1 / (1 - p) at that site only; an all-false mask at site 0 leaves a constant function of the input"""
    arch = R.ARCH_L1
    sd = R.leaf_state_dict(R.seeded_state_dict(arch, 5))
    inp, _ = R.seeded_inputs(arch, 2, 3, 1, 6)
    x, h = torch.from_numpy(inp["sample_pose_repr"]).double(), torch.from_numpy(inp["h2o_dist"]).double()
    shapes = R.site_shapes(arch, 3)
    with torch.no_grad():
        base = R.refine_train_forward(sd, arch, x, h, R.cond_of(inp))
        ones = {s: torch.ones(2, *rc, dtype=torch.bool) for s, rc in shapes.items()}
        kept = R.refine_train_forward(sd, arch, x, h, R.cond_of(inp), masks={3: ones[3]}, p=0.5)
        zero = R.refine_train_forward(sd, arch, x, h, R.cond_of(inp), masks={0: ~ones[0]}, p=0.5)
        zero2 = R.refine_train_forward(sd, arch, x, 2 * h, R.cond_of(inp), masks={0: ~ones[0]}, p=0.5)
    assert float((kept - base).abs().max()) > 1e-6
    assert float(((zero - x) - (zero2 - x)).abs().max()) == 0.0


@pytest.mark.parametrize("name", TRUNK_FIXTURES)
def test_restatement_reproduces_fixture(name):
    """float64 autograd through the restatement gives the reference's float64 output, loss and parameter gradients to 1e-9"""
    c = R.load_case(os.path.join(GOLDEN, name))
    out, loss, grads = R.loss_and_grads(c["sd"], c["arch"], c["inputs"], c["G"], c["obj_num"])
    assert R.rel_err(out, c["out"]) <= 1e-9
    assert abs(loss - c["loss"]) <= 1e-9 * abs(c["loss"])
    err = R.fixture_grad_err(grads, c)
    assert max(err.values()) <= 1e-9, max(err, key=err.get)
    assert c["tol_rel"] == pytest.approx(4 * float(c["z"]["e32_grad"])) and c["tol_rel_out"] == pytest.approx(4 * float(c["z"]["e32_out"]))


def e2e_case():
    """refinetrain_e2e.npz -> (case, batch of float64 tensors, obj_points, HandInteractionLoss on torch MANO layers and the torch
    nearest neighbour)"""
    sys.path.insert(0, os.path.join(HERE, "..", "oakink2-tamf_amd"))
    import contact_restatement as CS
    import mano_fixture as MF
    import mano_restatement as MR
    from oakink2_tamf_amd.mano import ManoArrays
    from oakink2_tamf_amd.model.interaction_loss import HandInteractionLoss

    c = R.load_case(os.path.join(GOLDEN, "refinetrain_e2e.npz"))
    z = c["z"]
    layers = []
    for seed in (int(z["seed_rh"]), int(z["seed_lh"])):
        arrays = ManoArrays(**MF.synthetic_arrays(778, seed))
        layer = MR.TorchManoLayer(arrays, 0, "cpu", torch.float64)
        layer.th_faces = torch.as_tensor(arrays.faces).long()
        layers.append(layer)
    loss = HandInteractionLoss(layers[0], layers[1], np.zeros((0, 2), np.int64), z["v_weights"], float(z["coef_rec_joint_loss"]),
                               float(z["coef_rec_vert_loss"]), coef_dist_h_loss=float(z["coef_dist_h_loss"]), contact_fn=CS.signed_contact_distance)
    batch = {k: torch.from_numpy(c["inputs"][k]).double() for k in ("sample_pose_repr", "pose_repr", "shape", "obj_embedding", "obj_traj", "mask")}
    batch["hand_side"] = c["inputs"]["hand_side"]
    return c, batch, torch.from_numpy(c["inputs"]["obj_points"]).double(), loss, CS


def test_restatement_reproduces_e2e_fixture():
    """the whole step in float64 torch - restatement trunk, MANO restatement, torch nearest neighbour, HandInteractionLoss.refine_terms,
    through segment_refine_train.refine_step_loss - gives the reference's loss terms and parameter gradients to 1e-9"""
    c, batch, pts, loss, CS = e2e_case()
    from oakink2_tamf_amd.model.segment_refine_train import refine_step_loss

    sd = R.leaf_state_dict(c["sd"])
    inp = {k: v.numpy() if torch.is_tensor(v) else v for k, v in batch.items()}

    def trunk(h2o):
        return R.refine_train_forward(sd, c["arch"], batch["sample_pose_repr"], h2o, R.cond_of(inp), obj_num=c["obj_num"])

    total, terms, res = refine_step_loss(trunk, batch, loss, pts, c["obj_num"], merged_fn=CS.merged_h2o_dist)
    total.backward()
    assert R.rel_err(res["refine_pose_repr"].detach().numpy(), c["out"]) <= 1e-9
    for k in ("loss", "rec_joint", "rec_vert", "dist_h"):
        ref = float(c["z"][f"term/{k}"])
        assert abs(float(terms[k].detach()) - ref) <= 1e-9 * abs(ref), k
    grads = {k: v.grad.numpy() for k, v in sd.items() if k not in R.BUFFERS}
    err = R.fixture_grad_err(grads, c)
    assert max(err.values()) <= 1e-9, max(err, key=err.get)


# ---- the Python-side refusals ----
def _batch(arch, B=2, T=4, nobj=2):
    inp, _ = R.seeded_inputs(arch, B, T, nobj, 9)
    b = {k: torch.from_numpy(inp[k]) for k in ("sample_pose_repr", "shape", "obj_embedding", "obj_traj")}
    b["hand_side"] = inp["hand_side"]
    return b, torch.from_numpy(inp["h2o_dist"])


def test_refusals_shapes_and_dtypes():
    from oakink2_tamf_amd.model.segment_refine_train import check_refine_batch

    arch = R.arch_dict(R.ARCH_TINY)
    b, h = _batch(R.ARCH_TINY)
    assert check_refine_batch(b, h, arch, [2, 1], [7, 9])[:3] == (2, 4, 2)
    for key, bad in (("sample_pose_repr", b["sample_pose_repr"][:, :, :98]), ("shape", b["shape"][:, :3]), ("obj_embedding", b["obj_embedding"][:1]),
                     ("obj_traj", b["obj_traj"][:, :, :, :8]), ("obj_traj", b["obj_traj"][:, :1])):
        with pytest.raises(ValueError, match=key):
            check_refine_batch({**b, key: bad}, h, arch)
    with pytest.raises(ValueError, match="h2o_dist"):
        check_refine_batch(b, h[:, :, :777], arch)
    with pytest.raises(ValueError, match="hand_side"):
        check_refine_batch({**b, "hand_side": ["rh"]}, h, arch)
    with pytest.raises(ValueError, match="unexpected hand_side"):
        check_refine_batch({**b, "hand_side": ["rh", "both"]}, h, arch)
    with pytest.raises(ValueError, match="obj_num"):
        check_refine_batch(b, h, arch, obj_num=[1, 3])
    with pytest.raises(ValueError, match="obj_num"):
        check_refine_batch(b, h, arch, obj_num=[1])
    with pytest.raises(ValueError, match="clip_ids"):
        check_refine_batch(b, h, arch, clip_ids=[1, 2, 3])
    with pytest.raises(TypeError, match="shape"):
        check_refine_batch({**b, "shape": b["shape"].long()}, h, arch)
    with pytest.raises(TypeError, match="h2o_dist"):
        check_refine_batch(b, h.numpy(), arch)


class _FakeBackend:
    def __init__(self):
        self.calls = 0

    def run_backward(self, grad):
        self.calls += 1


def test_refusal_second_backward_and_second_forward():
    """two backwards through one forward and a second forward before the backward of the first raise; the graph needs no device"""
    from oakink2_tamf_amd.model.segment_refine_train import PendingForward, SegmentRefineTrainStep, _TrunkFunction

    backend, pending = _FakeBackend(), PendingForward()
    anchor = torch.zeros(1, requires_grad=True)
    out = _TrunkFunction.apply(backend, pending, torch.ones(2, 3), anchor)
    assert out.requires_grad
    out.sum().backward(retain_graph=True)
    assert backend.calls == 1 and anchor.grad is None
    with pytest.raises(RuntimeError, match="serves one backward"):
        out.sum().backward()
    assert backend.calls == 1
    out = _TrunkFunction.apply(backend, PendingForward(), torch.ones(2, 3), anchor)
    with pytest.raises(RuntimeError, match="double backward"):
        torch.autograd.grad(out.sum(), anchor, create_graph=True, allow_unused=True)

    ts = object.__new__(SegmentRefineTrainStep)  # (no device: the refusal comes before anything touches one)
    ts._h, ts._pending = object(), PendingForward()
    with pytest.raises(RuntimeError, match="no backward yet"):
        ts.forward({})
    ts._h = None  # (nothing to destroy)


TAMF_ERR_INVALID = -1
HEADS_MSG = "the head dimension must be 64: latent_dim = 64 * num_heads, got latent_dim %d with %d heads"
FF_MSG = "ff_size must be a multiple of 16 in [16, 4096], got %d"


def test_create_and_mask_refusals_through_ctypes():
    """status and last_error text of every refusal of tamf_refinetrain_create and tamf_refinetrain_dropout_mask that returns before
    the first device call; *out, a sentinel before the call, is NULL after every refused create that was given both pointers"""
    import ctypes

    from oakink2_tamf_amd.hip_backend import _Arch
    from oakink2_tamf_amd.model import segment_refine_train as srt

    lib = srt.lib()
    good = R.arch_dict(R.ARCH_L1)  # (latent_dim 64, one head, ff_size 16, one layer)

    def create(arch=None, max_batch=2, max_frames=7, null=None):
        a = dict(good, **(arch or {}))
        st = _Arch(*[a[k] for k in R.ARCH_NAMES[:8]], 0, a["h2o_dim"], 1)
        out = ctypes.c_void_p(None if null == "arch" else 0x5A5A5A5A)  # (the null check comes before *out is written)
        rc = lib.tamf_refinetrain_create(None if null == "arch" else ctypes.byref(st), max_batch, max_frames, 0, None if null == "out" else ctypes.byref(out))
        return rc, lib.tamf_refinetrain_last_error().decode(), out.value

    cases = [(dict(null="arch"), "null argument"), (dict(null="out"), "null argument"),
             (dict(arch=dict(num_heads=9, latent_dim=576)), "num_heads = 9 outside [1, 8]"), (dict(arch=dict(num_heads=0)), "num_heads = 0 outside [1, 8]"),
             (dict(arch=dict(latent_dim=128)), HEADS_MSG % (128, 1)), (dict(arch=dict(ff_size=24)), FF_MSG % 24), (dict(arch=dict(ff_size=4112)), FF_MSG % 4112),
             (dict(arch=dict(num_layers=0)), "num_layers = 0 outside [1, 64]"), (dict(arch=dict(num_layers=65)), "num_layers = 65 outside [1, 64]")]
    cases += [(dict(arch={k: v}), f"{k} = {v} outside [1, 4096]")
              for k in ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "h2o_dim") for v in (0, 4097)]
    cases += [(dict(max_frames=1022), "max_frames = 1022 outside [1, 1021]"), (dict(max_frames=0), "max_frames = 0 outside [1, 1021]"),
              (dict(max_batch=0), "max_batch = 0 outside [1, 65535]"), (dict(max_batch=65536), "max_batch = 65536 outside [1, 65535]")]
    for kw, text in cases:
        rc, msg, out = create(**kw)
        assert (rc, msg) == (TAMF_ERR_INVALID, text), (kw, rc, msg)
        if kw.get("null") != "out":
            assert out is None, (kw, out)  # *out == NULL

    buf = (ctypes.c_uint8 * 64)()  # never written: the arguments are checked first
    ok = dict(site=0, rows=4, cols=4, p=0.5, out=ctypes.addressof(buf))
    for kw, text in ((dict(out=None), "null argument"), (dict(rows=0), "rows * cols must be in [1, 2^32)"), (dict(site=-1), "site must be >= 0"),
                     (dict(p=1.0), "p must be in [0, 1)"), (dict(p=float("nan")), "p must be in [0, 1)")):
        a = dict(ok, **kw)
        rc = lib.tamf_refinetrain_dropout_mask(3, 1, 2, a["site"], a["rows"], a["cols"], a["p"], a["out"], None)
        assert (rc, lib.tamf_refinetrain_last_error().decode()) == (TAMF_ERR_INVALID, text), (kw, rc)
    assert not any(buf)


def test_each_key_is_written_once():
    """every key stem of the refiner's state dict - outside the layers, and of one layer - occurs exactly once in the text of
    csrc/tamf_refinetrain.hip together with csrc/tamf_train_host.h (the layers' declarations): where the tensor is declared"""
    def stem(k):
        return re.sub(r"\.(weight|bias)$", "", k)

    layer = "seqTransEncoder.layers.0."
    keys = list(R.seeded_state_dict(R.ARCH_TINY, 0))
    outside = sorted({stem(k) for k in keys if not k.startswith("seqTransEncoder.")})
    per_layer = sorted({stem(k[len(layer):]) for k in keys if k.startswith(layer)})
    assert len(outside) == 11 and len(per_layer) == 7, (outside, per_layer)  # (norm1 and norm2 are two of the seven)
    text = ""
    for name in ("tamf_refinetrain.hip", "tamf_train_host.h"):
        with open(os.path.join(HERE, "..", "oakink2-tamf_amd", "csrc", name)) as f:
            text += f.read()
    for s in outside + per_layer:  # (as a whole word: input_process.poseEmbedding is also the tail of obj_input_process.poseEmbedding)
        n = len(re.findall(r"(?<![A-Za-z0-9_.])" + re.escape(s) + r"(?![A-Za-z0-9_])", text))
        assert n == 1, (s, n)


# ---- the library's description ----
def test_lib_description():
    from oakink2_tamf_amd import _lib

    lib = _lib.REFINETRAIN
    # (a training library in a group of its own: tests/test_contact_cpu.py pins TRAINING to its two entries, tests/test_host_mirror.py LIBRARIES)
    assert _lib.REFINE_TRAINING == (lib,) and lib not in _lib.LIBRARIES + _lib.TRAINING
    every = _lib.LIBRARIES + _lib.PREPROCESSING + _lib.TEXT_PREPROCESSING + _lib.TRAINING + _lib.REFINE_TRAINING
    assert len({l.stamp_path for l in every}) == len(every) == 8
    with open(os.path.join(_lib.INCLUDE, "tamf_refinetrain.h")) as f:
        declared = re.findall(r"\b(tamf_refinetrain_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    (out,) = lib.outputs
    assert out.file == "libtamf_refinetrain.so" and sorted(out.exports) == sorted(set(declared)) and len(declared) == len(set(declared))
    assert lib.sources == _lib._include_closure("tamf_refinetrain.hip")
    assert {"tamf_refinetrain.hip", "tamf_trunk_grad.h", "tamf_dropout.h", "tamf_f32_tower.h", "tamf_device.h", "tamf_weights.h",
            "tamf_train_host.h"} <= set(lib.sources)
    assert {"tamf_dropout.h", "tamf_train_host.h"} <= set(_lib.ENCTRAIN.sources)  # the shared dropout scheme and host code
    assert [l for l in every if "tamf_train_host.h" in l.sources] == [_lib.ENCTRAIN, lib]  # of the two training steps alone
    assert not set(_lib.EXPORTS) & set(out.exports)  # the sampler library gains no export
    assert callable(_lib.load_refinetrain)
