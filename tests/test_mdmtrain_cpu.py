"""The denoiser's training step without a device: the float64 restatement of the training forward (tests/mdm_train_restatement.py)
held to oracle.mdm_oracle.denoiser_forward at p = 0 and, through its autograd, to the tests/golden/mdmtrain_*.npz trunk fixtures (the
reference's own module); training_losses on a plain torch model against the reference's terms and gradients; the Python-side
refusals and those of tamf_mdmtrain_create; the description of libtamf_mdmtrain.so in _lib."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "oakink2-tamf_amd"))
import mdm_train_restatement as M  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")
TRUNK_FIXTURES = ("mdmtrain_l1_hd64.npz", "mdmtrain_l1_hd128.npz", "mdmtrain_tiny_hd64.npz", "mdmtrain_tiny_hd128.npz")
CSRC = os.path.join(HERE, "..", "oakink2-tamf_amd", "csrc")


@pytest.mark.parametrize("arch,B,T,nobj,ragged", [(M.ARCH_L1_64, 1, 1, 1, False), (M.ARCH_L1_128, 2, 3, 2, True), (M.ARCH_TINY_64, 3, 12, 2, True),
                                                  (M.ARCH_TINY_128, 2, 5, 3, False)])
def test_restatement_equals_oracle(arch, B, T, nobj, ragged):
    """p = 0: the restatement is oracle.mdm_oracle.denoiser_forward in float64 to 1e-12 (padded and ragged object means)"""
    sd = M.leaf_state_dict(M.seeded_state_dict(arch, 3))
    inp, obj_num = M.seeded_inputs(arch, B, T, nobj, 4, ragged)
    x, t = torch.from_numpy(inp["x_t"]).double(), torch.from_numpy(inp["t"])
    with torch.no_grad():
        a = M.mdm_train_forward(sd, arch, x, t, M.cond_of(inp), obj_num=obj_num)
        b = M.oracle_forward(sd, arch, x, t, inp, torch.float64, obj_num)
    assert a.shape == (B, arch.input_dim, 1, T) and float((a - b).abs().max()) <= 1e-12


@pytest.mark.parametrize("name", TRUNK_FIXTURES)
def test_restatement_reproduces_fixture(name):
    """float64 autograd through the restatement gives the reference's float64 output, loss and parameter gradients to 1e-9"""
    c = M.load_case(os.path.join(GOLDEN, name))
    out, loss, grads = M.loss_and_grads(c["sd"], c["arch"], c["inputs"], c["G"], c["obj_num"])
    assert M.rel_err(out, c["out"]) <= 1e-9
    assert abs(loss - c["loss"]) <= 1e-9 * abs(c["loss"])
    err = M.fixture_grad_err(grads, c)
    assert max(err.values()) <= 1e-9, max(err, key=err.get)
    assert c["tol_rel"] == pytest.approx(4 * float(c["z"]["e32_grad"])) and c["tol_rel_out"] == pytest.approx(4 * float(c["z"]["e32_out"]))
    assert c["arch"].latent_dim // c["arch"].num_heads == (128 if "hd128" in name else 64)


def objective_case(name):
    """mdmtrain_losses.npz / mdmtrain_sgd.npz -> (case, the diffusion the fixture was captured with)"""
    from oakink2_tamf_amd.model.diffusion_util import create_gaussian_diffusion

    c = M.load_case(os.path.join(GOLDEN, name))
    return c, create_gaussian_diffusion(int(c["z"]["diffusion_steps"]), "cosine")


def objective_batch(c, dtype=torch.float64, device="cpu"):
    inp = c["inputs"]
    b = {k: torch.from_numpy(np.ascontiguousarray(inp[k])).to(device=device, dtype=dtype) for k in ("text_embedding", "shape", "obj_embedding", "obj_traj")}
    b["hand_side"], b["mask"] = inp["hand_side"], torch.from_numpy(inp["mask"]).to(device)
    return b


def test_training_losses_on_the_reference_terms():
    """training_losses with the float64 restatement as the model: the reference's q_sample output, mse per clip and the gradients of
    (terms["loss"] * weights).mean(), to rounding; the callback's pair is handed through"""
    from oakink2_tamf_amd.model.interaction_segment_mdm_train import training_losses

    c, diffusion = objective_case("mdmtrain_losses.npz")
    inp, z = c["inputs"], c["z"]
    sd = M.leaf_state_dict(c["sd"])
    seen = {}

    def model(x_t, t, batch):
        seen["x_t"], seen["t"] = x_t, t
        return M.mdm_train_forward(sd, c["arch"], x_t, t, {k: batch[k] for k in ("text_embedding", "hand_side", "shape", "obj_embedding", "obj_traj")})

    x_start, t, noise = torch.from_numpy(inp["x_start"]).double(), torch.from_numpy(inp["t"]), torch.from_numpy(inp["noise"]).double()
    terms, extra = training_losses(diffusion, model, x_start, t, model_kwargs={"batch": objective_batch(c)}, noise=noise,
                                   loss_callback=lambda out, batch: (out.sum() * 0 + 3.0, {"three": 3.0}))
    assert float(extra[0].detach()) == 3.0 and extra[1] == {"three": 3.0} and terms["loss"] is terms["mse"]
    assert torch.equal(seen["t"], t) and M.rel_err(seen["x_t"].numpy(), z["x_t"]) <= 1e-12
    assert terms["mse"].shape == (3,) and M.rel_err(terms["mse"].detach().numpy(), z["mse"]) <= 1e-9
    (terms["loss"] * torch.from_numpy(inp["weights"]).double()).mean().backward()
    err = M.fixture_grad_err({k: v.grad.numpy() for k, v in sd.items() if k not in M.BUFFERS}, c)
    assert max(err.values()) <= 1e-9, max(err, key=err.get)
    assert training_losses(diffusion, model, x_start, t, model_kwargs={"batch": objective_batch(c)}, noise=noise)[1] == (None, None)
    with pytest.raises(KeyError, match="batch"):
        training_losses(diffusion, model, x_start, t)


def test_uniform_timesteps_and_the_pinned_refusal():
    """the uniform schedule sampler: t over the diffusion's timesteps, weights 1; GaussianDiffusion.training_losses stays a refusal"""
    from oakink2_tamf_amd.model.diffusion_util import create_gaussian_diffusion
    from oakink2_tamf_amd.model.interaction_segment_mdm_train import uniform_timesteps

    diffusion = create_gaussian_diffusion(50, "cosine")
    t, w = uniform_timesteps(diffusion, 4000, rng=np.random.default_rng(0))
    assert t.dtype == torch.int64 and int(t.min()) == 0 and int(t.max()) == 49 and w.dtype == torch.float32 and bool((w == 1).all())
    assert np.bincount(t.numpy(), minlength=50).min() > 40
    t2, _ = uniform_timesteps(diffusion, 8)
    assert t2.shape == (8,) and 0 <= int(t2.min()) and int(t2.max()) < 50
    with pytest.raises(NotImplementedError):
        diffusion.training_losses(None, None, None)


# ---- the Python-side refusals ----
def _batch(arch, B=2, T=4, nobj=2):
    inp, _ = M.seeded_inputs(arch, B, T, nobj, 9)
    b = {k: torch.from_numpy(inp[k]) for k in ("text_embedding", "shape", "obj_embedding", "obj_traj")}
    b["hand_side"] = inp["hand_side"]
    return b, torch.from_numpy(inp["x_t"]), torch.from_numpy(inp["t"])


def test_refusals_shapes_and_dtypes():
    from oakink2_tamf_amd.model.interaction_segment_mdm_train import check_mdm_batch

    arch = M.arch_dict(M.ARCH_TINY_128)
    b, x, t = _batch(M.ARCH_TINY_128)

    def check(x=x, t=t, batch=b, text=None, **kw):
        return check_mdm_batch(x, t, batch, batch["text_embedding"] if text is None else text, arch, **kw)

    got = check(obj_num=[2, 1], clip_ids=[7, 9])
    assert got[:3] == (2, 4, 2) and got[3] == [0, 1] and got[4].dtype == np.int32 and list(got[4]) == list(t.numpy())
    for key, bad in (("shape", b["shape"][:, :3]), ("obj_embedding", b["obj_embedding"][:1]), ("obj_traj", b["obj_traj"][:, :, :, :8]),
                     ("obj_traj", b["obj_traj"][:, :1])):
        with pytest.raises(ValueError, match=key):
            check(batch={**b, key: bad})
    for bad in (x[:, :98], x[:, :, 0], x.expand(2, 99, 2, 4)):
        with pytest.raises(ValueError, match="x_t"):
            check(x=bad)
    with pytest.raises(ValueError, match="text_embedding"):
        check(text=b["text_embedding"][:, :15])
    with pytest.raises(ValueError, match="timesteps"):
        check(t=t[:1])
    for bad in (torch.tensor([0, 5000]), torch.tensor([-1, 3])):
        with pytest.raises(ValueError, match=r"timesteps must be in \[0, 4999\]"):
            check(t=bad)
    assert check(t=torch.tensor([0, 4999]))[4].tolist() == [0, 4999]
    with pytest.raises(TypeError, match="timesteps"):
        check(t=t.float())
    with pytest.raises(ValueError, match="hand_side"):
        check(batch={**b, "hand_side": ["rh"]})
    with pytest.raises(ValueError, match="unexpected hand_side"):
        check(batch={**b, "hand_side": ["rh", "both"]})
    with pytest.raises(ValueError, match="obj_num"):
        check(obj_num=[1, 3])
    with pytest.raises(ValueError, match="clip_ids"):
        check(clip_ids=[1, 2, 3])
    with pytest.raises(TypeError, match="shape"):
        check(batch={**b, "shape": b["shape"].long()})
    with pytest.raises(TypeError, match="x_t"):
        check(x=x.numpy())


def test_refusal_second_forward_uses_the_refiners_mechanism():
    """the single-use claim is segment_refine_train's, not a copy; a second forward before the backward of the first raises without a device"""
    from oakink2_tamf_amd.model import interaction_segment_mdm_train as imt
    from oakink2_tamf_amd.model import segment_refine_train as srt

    assert imt.PendingForward is srt.PendingForward and imt._TrunkFunction is srt._TrunkFunction
    ts = object.__new__(imt.InterationSegmentMDMTrainStep)
    ts._h, ts._pending = object(), srt.PendingForward()
    with pytest.raises(RuntimeError, match="no backward yet"):
        ts.forward(None, None, {})
    ts.discard_forward()
    assert not ts._pending.open
    ts._h = None  # (nothing to destroy)


TAMF_ERR_INVALID = -1
HEADS_MSG = "the head dimension must be 64 or 128: latent_dim = 64 * num_heads or 128 * num_heads, in [64, 512], got latent_dim %d with %d heads"
FF_MSG = "ff_size must be a multiple of 16 in [16, 4096], got %d"


def test_create_and_mask_refusals_through_ctypes():
    """status and last_error text of every refusal of tamf_mdmtrain_create and tamf_mdmtrain_dropout_mask that returns before the first
    device call (each with its limit in the message); *out, a sentinel before the call, is NULL after every refused create"""
    from oakink2_tamf_amd.hip_backend import _Arch
    from oakink2_tamf_amd.model import interaction_segment_mdm_train as imt

    lib = imt.lib()
    good = M.arch_dict(M.ARCH_L1_128)

    def create(arch=None, max_batch=2, max_frames=7, null=None):
        a = dict(good, **(arch or {}))
        st = _Arch(*[a[k] for k in M.ARCH_NAMES], 0, 0)
        out = ctypes.c_void_p(None if null == "arch" else 0x5A5A5A5A)
        rc = lib.tamf_mdmtrain_create(None if null == "arch" else ctypes.byref(st), max_batch, max_frames, 0, None if null == "out" else ctypes.byref(out))
        return rc, lib.tamf_mdmtrain_last_error().decode(), out.value

    cases = [(dict(null="arch"), "null argument"), (dict(null="out"), "null argument"),
             (dict(arch=dict(latent_dim=96)), HEADS_MSG % (96, 1)), (dict(arch=dict(latent_dim=1024, num_heads=8)), HEADS_MSG % (1024, 8)),
             (dict(arch=dict(latent_dim=1024, num_heads=16)), HEADS_MSG % (1024, 16)), (dict(arch=dict(latent_dim=256, num_heads=1)), HEADS_MSG % (256, 1)),
             (dict(arch=dict(num_heads=0)), HEADS_MSG % (128, 0)), (dict(arch=dict(latent_dim=0, num_heads=0)), HEADS_MSG % (0, 0)),
             (dict(arch=dict(ff_size=24)), FF_MSG % 24), (dict(arch=dict(ff_size=4112)), FF_MSG % 4112),
             (dict(arch=dict(num_layers=0)), "num_layers = 0 outside [1, 64]"), (dict(arch=dict(num_layers=65)), "num_layers = 65 outside [1, 64]")]
    cases += [(dict(arch={k: v}), f"{k} = {v} outside [1, 4096]")
              for k in ("input_dim", "obj_input_dim", "hand_shape_dim", "obj_embed_dim", "clip_dim") for v in (0, 4097)]
    cases += [(dict(max_frames=1020), "max_frames = 1020 outside [1, 1019]"), (dict(max_frames=0), "max_frames = 0 outside [1, 1019]"),
              (dict(max_batch=0), "max_batch = 0 outside [1, 65535]"), (dict(max_batch=65536), "max_batch = 65536 outside [1, 65535]")]
    for kw, text in cases:
        rc, msg, out = create(**kw)
        assert (rc, msg) == (TAMF_ERR_INVALID, text), (kw, rc, msg)
        if kw.get("null") != "out":
            assert out is None, (kw, out)  # *out == NULL

    buf = (ctypes.c_uint8 * 64)()  # never written: the arguments are checked first
    ok = dict(site=0, rows=4, cols=4, p=0.5, out=ctypes.addressof(buf))
    for kw, text in ((dict(out=None), "null argument"), (dict(rows=0), "rows * cols must be in [1, 2^32)"), (dict(site=-1), "site must be >= 0"),
                     (dict(p=1.0), "p must be in [0, 1)")):
        a = dict(ok, **kw)
        rc = lib.tamf_mdmtrain_dropout_mask(3, 1, 2, a["site"], a["rows"], a["cols"], a["p"], a["out"], None)
        assert (rc, lib.tamf_mdmtrain_last_error().decode()) == (TAMF_ERR_INVALID, text), (kw, rc)
    assert not any(buf)


def test_each_key_is_written_once():
    """every key stem of G's state dict - outside the layers, and of one layer - occurs exactly once in the text of csrc/
    tamf_mdmtrain.hip together with csrc/tamf_train_host.h (the layers' declarations); the shared layer stack names no tensor"""
    def stem(k):
        return re.sub(r"\.(weight|bias)$", "", k)

    def count(s, text):  # (as a whole word: input_process.poseEmbedding is also the tail of obj_input_process.poseEmbedding)
        return len(re.findall(r"(?<![A-Za-z0-9_.])" + re.escape(s) + r"(?![A-Za-z0-9_])", text))

    layer = "seqTransEncoder.layers.0."
    keys = list(M.seeded_state_dict(M.ARCH_TINY_128, 0))
    outside = sorted({stem(k) for k in keys if not k.startswith("seqTransEncoder.")})
    per_layer = sorted({stem(k[len(layer):]) for k in keys if k.startswith(layer)})
    assert len(outside) == 14 and len(per_layer) == 7, (outside, per_layer)
    text = {}
    for name in ("tamf_mdmtrain.hip", "tamf_train_host.h", "tamf_trunk_host.h"):
        with open(os.path.join(CSRC, name)) as f:
            text[name] = f.read()
    for s in outside + per_layer:
        assert count(s, text["tamf_mdmtrain.hip"] + text["tamf_train_host.h"]) == 1, s
        assert count(s, text["tamf_trunk_host.h"]) == 0, s
    assert "declare" not in text["tamf_trunk_host.h"].replace("declares no tensor", "")


def test_one_layer_stack_for_both_models():
    """forward_layer / backward_layer are defined in tamf_trunk_host.h alone; both training libraries launch the attention kernels
    through it, and tamf_f32_tower.h holds no helper of theirs"""
    text = {}
    for name in ("tamf_mdmtrain.hip", "tamf_refinetrain.hip", "tamf_trunk_host.h", "tamf_trunk_grad.h"):
        with open(os.path.join(CSRC, name)) as f:
            text[name] = f.read()
    for fn in ("void forward_layer(", "void backward_layer(", "tg_attn_fwd_kernel<", "tg_wgrad_kernel,"):
        assert fn in text["tamf_trunk_host.h"] and fn not in text["tamf_mdmtrain.hip"] and fn not in text["tamf_refinetrain.hip"], fn
    for name in ("tamf_mdmtrain.hip", "tamf_refinetrain.hip"):
        assert "s.forward_layer(l)" in text[name] and "s.backward_layer(l)" in text[name]
    assert "template <int HD>\n__global__ __launch_bounds__(64) void tg_attn_bwd_kv_kernel" in text["tamf_trunk_grad.h"]
    assert "f32_score_tile(" not in text["tamf_trunk_grad.h"] and "f32_load_q(" not in text["tamf_trunk_grad.h"]
    modes = re.search(r"enum TgMode \{(.*?)\};", text["tamf_trunk_grad.h"], flags=re.S).group(1)
    names = re.findall(r"^\s*(TG_\w+)", modes, flags=re.M)
    assert names[-1] == "TG_HEAD" and names[:8] == ["TG_LIN", "TG_SILU", "TG_GELU_DROP", "TG_DROP_RES", "TG_HEAD_RES", "TG_BWD_SILU", "TG_BWD_GELU_DROP", "TG_BWD_RES"]


# ---- the library's description ----
def test_lib_description():
    from oakink2_tamf_amd import _lib

    lib = _lib.MDMTRAIN
    old = _lib.LIBRARIES + _lib.PREPROCESSING + _lib.TEXT_PREPROCESSING + _lib.TRAINING + _lib.REFINE_TRAINING
    assert _lib.DENOISER_TRAINING == (lib,) and lib not in old
    every = old + _lib.DENOISER_TRAINING
    assert len({l.stamp_path for l in every}) == len(every) == 9 and len({l.digest() for l in every}) == 9
    with open(os.path.join(_lib.INCLUDE, "tamf_mdmtrain.h")) as f:
        declared = re.findall(r"\b(tamf_mdmtrain_\w+)\s*\(", re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S))
    (out,) = lib.outputs
    assert out.file == "libtamf_mdmtrain.so" and sorted(out.exports) == sorted(set(declared)) and len(declared) == len(set(declared)) == 9
    assert out.exports is _lib.MDMTRAIN_EXPORTS and _lib.MDMTRAIN_LIB_PATH == lib.paths[0]
    assert lib.sources == _lib._include_closure("tamf_mdmtrain.hip")
    assert {"tamf_mdmtrain.hip", "tamf_trunk_host.h", "tamf_trunk_grad.h", "tamf_dropout.h", "tamf_f32_tower.h", "tamf_device.h", "tamf_weights.h",
            "tamf_train_host.h"} <= set(lib.sources)
    assert [l for l in every if "tamf_trunk_host.h" in l.sources] == [_lib.REFINETRAIN, lib]  # of the two trunk training steps alone
    assert [l for l in every if "tamf_train_host.h" in l.sources] == [_lib.ENCTRAIN, _lib.REFINETRAIN, lib]
    assert not (set(_lib.EXPORTS) | set(_lib.REFINETRAIN_EXPORTS)) & set(out.exports)
    assert callable(_lib.load_mdmtrain)
    import inspect

    assert "DENOISER_TRAINING" in inspect.getsource(_lib.build)


def test_built_library_exports_the_headers_functions():
    """nm -D of the built library: exactly the header's functions among the tamf_* symbols"""
    import shutil
    import subprocess

    from oakink2_tamf_amd import _lib

    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/llvm/bin/llvm-nm"
    path = _lib.MDMTRAIN.build()
    res = subprocess.run([nm, "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    syms = sorted(ln.split()[-1] for ln in res.stdout.splitlines() if ln.split() and ln.split()[-1].startswith("tamf_"))
    assert syms == sorted(_lib.MDMTRAIN_EXPORTS)
