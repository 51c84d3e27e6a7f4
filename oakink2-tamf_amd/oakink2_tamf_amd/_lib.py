"""Locate / build / load the native libraries.  Each is described once, by a Library: its translation unit in csrc/, its C headers in
include/, the files it produces with their extra flags and export lists, the kernels whose descriptors the build looks up in the
device assembly, and whether the counted-wait ISA checks apply.  Sources, digest, staleness, build and load are written once, over
that description:
  SAMPLER  csrc/tamf_hip.hip  -> libtamf_hip.so (include/tamf_hip.h, the drop-in surface) and, for tests/ and tools/ only,
                                 libtamf_hip_hooks.so (-DTAMF_TEST_HOOKS: + csrc/tamf_hip_hooks.h, the entry points of include/tamf_hip_test.h)
  EVAL     csrc/tamf_eval.hip -> libtamf_eval.so (include/tamf_eval.h: the context-free evaluation kernels of the SIV score)
  MANO     csrc/tamf_mano.hip -> libtamf_mano.so (include/tamf_mano.h: the native MANO hand layer)
  POINTENC csrc/tamf_pointenc.hip -> libtamf_pointenc.so (include/tamf_pointenc.h: the PointBERT point encoder behind obj_embedding)
  TEXTENC  csrc/tamf_textenc.hip -> libtamf_textenc.so (include/tamf_textenc.h: the CLIP text tower behind text_embedding)
  ENCTRAIN csrc/tamf_enctrain.hip -> libtamf_enctrain.so (include/tamf_enctrain.h: the SegmentEncoder training step - forward, loss, gradients)
  CONTACT  csrc/tamf_contact.hip -> libtamf_contact.so (include/tamf_contact.h: the contact-distance kernels of the training losses)
  REFINETRAIN csrc/tamf_refinetrain.hip -> libtamf_refinetrain.so (include/tamf_refinetrain.h: the SegmentRefineModel training step - forward, backward)
  MDMTRAIN csrc/tamf_mdmtrain.hip -> libtamf_mdmtrain.so (include/tamf_mdmtrain.h: the InterationSegmentMDM training step - forward, backward)
  OPTIM    csrc/tamf_optim.hip -> libtamf_optim.so (include/tamf_optim.h: per-parameter gradient clipping + AdamW over a tensor table)
  RENDER   csrc/tamf_render.hip -> libtamf_render.so (include/tamf_render.h: projection, triangle / point rasteriser, Lambert shading,
           depth peeling, composite, supersampling resolve)
  SURFACE  csrc/tamf_surface.hip -> libtamf_surface.so (include/tamf_surface.h: the bit-defined surface sampler behind the object point
           clouds - face areas, block scan with a fixed carry pass, Philox draw + binary search on the CDF)
  MESHDIST csrc/tamf_meshdist.hip -> libtamf_meshdist.so (include/tamf_meshdist.h: the bit-defined point-to-mesh distance behind the
           penetration depth score and process_sdf - triangle tiles with boxes, culled sweep, the inside test of tamf_mesh_contains)
  SDFGRID  csrc/tamf_sdfgrid.hip -> libtamf_sdfgrid.so (include/tamf_sdfgrid.h: the bit-defined SDF-lattice sampler behind the training
           losses' `pen` term - pose transform and trilinear read of the lattices process_sdf writes, forward and backward)
  WINDING  csrc/tamf_winding.hip -> libtamf_winding.so (include/tamf_winding.h: the generalized winding number behind the `winding` sign of
           process_sdf, the PD and SIV scores and the penetration map - solid angles summed in a fixed tree, points and lattices)
POINTENC and TEXTENC share two headers of csrc/, compiled into each: tamf_f32_tower.h (the fp32 GEMM, LayerNorm row and attention
score tile of the two towers) and tamf_weights.h (the host side: error string, weight table, packer, upload, workspace helpers).
ENCTRAIN, REFINETRAIN and MDMTRAIN share tamf_train_host.h (the table of bound tensors, the context base, the call checks, the
launcher); REFINETRAIN and MDMTRAIN share tamf_trunk_host.h (the layer stack over the kernels of tamf_trunk_grad.h).
Every library has its own sources, stamp and lock: building or loading one never touches another."""
from __future__ import annotations

import ctypes
import os
import shutil
import subprocess
import threading
from dataclasses import dataclass
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.normpath(os.path.join(_HERE, "..", "csrc"))
INCLUDE = os.path.normpath(os.path.join(_HERE, "..", "..", "include"))
LIB_DIR = os.path.join(_HERE, "lib")  # everything a build writes: libraries, stamps, locks, the work directory
LIB_PATH = os.path.join(LIB_DIR, "libtamf_hip.so")
HOOKS_PATH = os.path.join(LIB_DIR, "libtamf_hip_hooks.so")  # test / measurement build (never loaded by the product path)
EVAL_LIB_PATH = os.path.join(LIB_DIR, "libtamf_eval.so")
MANO_LIB_PATH = os.path.join(LIB_DIR, "libtamf_mano.so")
POINTENC_LIB_PATH = os.path.join(LIB_DIR, "libtamf_pointenc.so")
TEXTENC_LIB_PATH = os.path.join(LIB_DIR, "libtamf_textenc.so")
ENCTRAIN_LIB_PATH = os.path.join(LIB_DIR, "libtamf_enctrain.so")
CONTACT_LIB_PATH = os.path.join(LIB_DIR, "libtamf_contact.so")
REFINETRAIN_LIB_PATH = os.path.join(LIB_DIR, "libtamf_refinetrain.so")
MDMTRAIN_LIB_PATH = os.path.join(LIB_DIR, "libtamf_mdmtrain.so")
OPTIM_LIB_PATH = os.path.join(LIB_DIR, "libtamf_optim.so")
RENDER_LIB_PATH = os.path.join(LIB_DIR, "libtamf_render.so")
SURFACE_LIB_PATH = os.path.join(LIB_DIR, "libtamf_surface.so")
MESHDIST_LIB_PATH = os.path.join(LIB_DIR, "libtamf_meshdist.so")
SDFGRID_LIB_PATH = os.path.join(LIB_DIR, "libtamf_sdfgrid.so")
WINDING_LIB_PATH = os.path.join(LIB_DIR, "libtamf_winding.so")

EXPORTS = [  # include/tamf_hip.h: what libtamf_hip.so exports, nothing else
    "tamf_ctx_create", "tamf_ctx_resize", "tamf_ctx_destroy", "tamf_last_error", "tamf_load_weight", "tamf_finalize_weights",
    "tamf_set_schedule", "tamf_set_timestep_map", "tamf_set_cond", "tamf_set_cond_ragged", "tamf_denoise", "tamf_ddpm_step", "tamf_sample_loop", "tamf_refine",
    "tamf_encode",
    "tamf_pose_decode", "tamf_h2o_dist", "tamf_contact_min_dist", "tamf_mesh_contains", "tamf_transform_points", "tamf_vertex_normals",
    "tamf_power_spectrum_sum",
    "tamf_get_status_flags", "tamf_step_kernel_count", "tamf_loop_stats", "tamf_step_profile", "tamf_refine_profile",
]
HOOK_EXPORTS = [  # include/tamf_hip_test.h: additionally in libtamf_hip_hooks.so
    "tamf_test_gemm", "tamf_test_gemm_resid", "tamf_test_attention", "tamf_test_philox", "tamf_test_set_guard_bytes", "tamf_test_check_guards",
    "tamf_test_poke", "tamf_test_fail_alloc_after", "tamf_test_fill_scratch", "tamf_bench_gemm", "tamf_bench_attention", "tamf_bench_mfma_rate", "tamf_set_gemm_tuning",
]
EVAL_EXPORTS = [  # include/tamf_eval.h: what libtamf_eval.so exports
    "tamf_eval_last_error", "tamf_voxelize_lattice", "tamf_mesh_contains_count_workspace", "tamf_mesh_contains_count",
]
MANO_EXPORTS = [  # include/tamf_mano.h: what libtamf_mano.so exports
    "tamf_mano_last_error", "tamf_mano_model_create", "tamf_mano_model_destroy", "tamf_mano_model_set_tiles", "tamf_mano_forward",
    "tamf_mano_backward",
]
POINTENC_EXPORTS = [  # include/tamf_pointenc.h: what libtamf_pointenc.so exports
    "tamf_pointenc_last_error", "tamf_pointenc_model_create", "tamf_pointenc_load_weight", "tamf_pointenc_finalize", "tamf_pointenc_destroy",
    "tamf_pointenc_fold_bn", "tamf_pointenc_fps", "tamf_pointenc_group", "tamf_pointenc_workspace_bytes", "tamf_pointenc_encode",
]
TEXTENC_EXPORTS = [  # include/tamf_textenc.h: what libtamf_textenc.so exports
    "tamf_textenc_last_error", "tamf_textenc_model_create", "tamf_textenc_load_weight", "tamf_textenc_finalize", "tamf_textenc_destroy",
    "tamf_textenc_workspace_bytes", "tamf_textenc_encode",
]
ENCTRAIN_EXPORTS = [  # include/tamf_enctrain.h: what libtamf_enctrain.so exports
    "tamf_enctrain_last_error", "tamf_enctrain_create", "tamf_enctrain_destroy", "tamf_enctrain_bind", "tamf_enctrain_step",
    "tamf_enctrain_dropout_mask",
]
CONTACT_EXPORTS = [  # include/tamf_contact.h: what libtamf_contact.so exports
    "tamf_contact_last_error", "tamf_contact_forward", "tamf_contact_backward",
]
REFINETRAIN_EXPORTS = [  # include/tamf_refinetrain.h: what libtamf_refinetrain.so exports
    "tamf_refinetrain_last_error", "tamf_refinetrain_create", "tamf_refinetrain_destroy", "tamf_refinetrain_bind", "tamf_refinetrain_forward",
    "tamf_refinetrain_backward", "tamf_refinetrain_dropout_mask", "tamf_refinetrain_set_profile", "tamf_refinetrain_get_profile",
]
MDMTRAIN_EXPORTS = [  # include/tamf_mdmtrain.h: what libtamf_mdmtrain.so exports
    "tamf_mdmtrain_last_error", "tamf_mdmtrain_create", "tamf_mdmtrain_destroy", "tamf_mdmtrain_bind", "tamf_mdmtrain_forward",
    "tamf_mdmtrain_backward", "tamf_mdmtrain_dropout_mask", "tamf_mdmtrain_set_profile", "tamf_mdmtrain_get_profile",
]
OPTIM_EXPORTS = [  # include/tamf_optim.h: what libtamf_optim.so exports
    "tamf_optim_last_error", "tamf_optim_create", "tamf_optim_destroy", "tamf_optim_bind", "tamf_optim_grad_norms", "tamf_optim_step",
]
RENDER_EXPORTS = [  # include/tamf_render.h: what libtamf_render.so exports
    "tamf_render_last_error", "tamf_render_project", "tamf_render_clear", "tamf_render_raster", "tamf_render_points", "tamf_render_shade_mesh",
    "tamf_render_shade_points", "tamf_render_fill", "tamf_render_raster_behind", "tamf_render_points_behind", "tamf_render_shade_mesh_colors",
    "tamf_render_shade_points_colors", "tamf_render_composite", "tamf_render_resolve",
]
SURFACE_EXPORTS = [  # include/tamf_surface.h: what libtamf_surface.so exports
    "tamf_surface_last_error", "tamf_surface_workspace_bytes", "tamf_surface_sample",
]
MESHDIST_EXPORTS = [  # include/tamf_meshdist.h: what libtamf_meshdist.so exports
    "tamf_meshdist_last_error", "tamf_meshdist_workspace", "tamf_meshdist_prepare", "tamf_meshdist_points_workspace", "tamf_meshdist_points",
    "tamf_meshdist_lattice",
]
SDFGRID_EXPORTS = [  # include/tamf_sdfgrid.h: what libtamf_sdfgrid.so exports
    "tamf_sdfgrid_last_error", "tamf_sdfgrid_forward", "tamf_sdfgrid_backward",
]
WINDING_EXPORTS = [  # include/tamf_winding.h: what libtamf_winding.so exports
    "tamf_winding_last_error", "tamf_winding_workspace", "tamf_winding_prepare", "tamf_winding_points_workspace", "tamf_winding_points",
    "tamf_winding_lattice",
]


class TamfBuildError(RuntimeError):
    pass


def _include_closure(root: str):
    """root and every csrc header it includes with #include "...", transitively: what a build of `root` reads from csrc/"""
    import re

    seen, todo = [], [root]
    while todo:
        name = todo.pop()
        path = os.path.join(CSRC, name)
        if name in seen or not os.path.exists(path):
            continue
        seen.append(name)
        with open(path) as f:
            todo += [m for m in re.findall(r'^\s*#\s*include\s+"([^"/]+)"', f.read(), flags=re.M)]
    return sorted(seen)


def _compile(hipcc: str, workdir: str, extra, name: str, source: str):
    """One hipcc run in `workdir` with -save-temps=obj: the library AND the device assembly of the same compile.
    The product build takes no flags from the environment (tools/ab_build.sh builds the -DTAMF_BENCH / -DTAMF_TIMELINE copies
    for measurements under other file names)."""
    os.makedirs(workdir, exist_ok=True)
    out = os.path.join(workdir, name)
    cmd = [hipcc, "-O3", "--offload-arch=gfx950", "-std=c++17", "-shared", "-fPIC", "-Wno-unused-value", "-Wno-unused-function", "-save-temps=obj",
           "-o", out, os.path.join(CSRC, source)] + list(extra)
    res = subprocess.run(cmd, capture_output=True, text=True, cwd=workdir)
    if res.returncode != 0:
        raise TamfBuildError("hipcc failed:\n" + res.stdout + res.stderr)
    asm = [f for f in os.listdir(workdir) if f.endswith("gfx950.s")]
    return out, (os.path.join(workdir, asm[0]) if asm else None)


def _check_counted_waits(asms, verbose: bool) -> None:
    """The clip-tile GEMM's counted waits assume one global_store per source-level store: verified on the assembly of THIS compile
    (whatever hipcc the site has), of every produced file.  Raises what makes build() compile again with -DTAMF_CLIP_SAFE_WAIT."""
    import warnings

    from . import _isa_check

    n = nd = 0
    for a in asms:
        if a is None:
            raise _isa_check.IsaMismatch("hipcc left no device assembly to check")
        n = _isa_check.check(a)
        nd = _isa_check.check_deep(a)
    if verbose:
        print(f"ISA check: all {n} clip_gemm_kernel and {nd} gemm_deep_kernel instantiations match the counted waits (both builds)")
    try:  # register spilling in a hot kernel is a performance bug, not a correctness one: reported, never fatal
        _isa_check.check_scratch(asms[0])
    except _isa_check.IsaMismatch as e:
        warnings.warn(f"libtamf_hip: {e}")


class Output(NamedTuple):
    file: str  # in LIB_DIR
    flags: tuple  # beyond those of _compile
    exports: list  # exactly the tamf_* symbols the file defines


@dataclass(frozen=True)
class Library:
    name: str  # of its first output, without the suffix: names the stamp, the lock and the library in messages
    root: str  # the translation unit in csrc/
    headers: tuple  # of include/: part of the digest
    outputs: tuple  # of Output; compiled side by side when there are two
    kernels: tuple = ()  # name prefixes whose descriptors must be in the device assembly; their scratch / VGPR use is reported
    counted_waits: bool = False  # _check_counted_waits, and the -DTAMF_CLIP_SAFE_WAIT rebuild when it fails

    @property
    def sources(self):
        """what a build reads from csrc/ (the #include closure of the translation unit), sorted"""
        return _include_closure(self.root)

    @property
    def paths(self):
        return [os.path.join(LIB_DIR, o.file) for o in self.outputs]

    @property
    def stamp_path(self) -> str:
        return self.paths[0] + ".src.sha256"

    def digest(self) -> str:
        """sha256 over the sources and the C headers (directory-tagged names + contents: csrc/tamf_mano.h and include/tamf_mano.h share
        a base name): what the built library is stamped with"""
        import hashlib

        h = hashlib.sha256()
        for tag, path in [("csrc/" + s, os.path.join(CSRC, s)) for s in self.sources] + [("include/" + h_, os.path.join(INCLUDE, h_)) for h_ in self.headers]:
            if os.path.exists(path):
                h.update(tag.encode())
                with open(path, "rb") as f:
                    h.update(f.read())
        return h.hexdigest()

    def stale(self) -> bool:
        """Fresh when every produced file exists and the stamp written beside them by build() equals the digest of the sources in the
        tree.  Content, not mtimes: copying the tree to a GPU box resets every mtime, and eight ranks of a multi-GPU launch must not
        queue behind a needless 80-second rebuild inside somebody's timed window.  A library without a stamp is rebuilt."""
        if not all(os.path.exists(p) for p in self.paths):
            return True
        try:
            with open(self.stamp_path) as f:
                return f.read().strip() != self.digest()
        except OSError:
            return True

    def _compile_all(self, hipcc: str, wd: str, extra=()):
        """[(library, device assembly)] per output, each from a work directory of its own; never more than two hipcc at a time"""
        from concurrent.futures import ThreadPoolExecutor

        with ThreadPoolExecutor(max_workers=2) as ex:
            return list(ex.map(lambda o: _compile(hipcc, os.path.join(wd, o.file), o.flags + tuple(extra), o.file, self.root), self.outputs))

    def _report_kernels(self, asm, verbose: bool) -> None:
        """The scratch / VGPR use of self.kernels, from the device assembly: a missing descriptor is an error, a spilling kernel is
        reported, never fatal."""
        from . import _isa_check

        if asm is None:
            raise TamfBuildError(f"hipcc left no device assembly of {self.outputs[0].file} to check")
        rep = _isa_check.scratch_report(asm, prefixes=self.kernels)
        if len(rep) < len(self.kernels):
            raise TamfBuildError(f"{self.outputs[0].file}: kernel descriptors missing from the device assembly (found {[r[0] for r in rep]})")
        for name, scratch, vgprs in rep:
            if verbose:
                print(f"{self.name}: {name}: {vgprs} vgprs, {scratch} B scratch")
            if scratch > _isa_check.SCRATCH_LIMIT:
                import warnings

                warnings.warn(f"{self.name}: {name} keeps {scratch} bytes of scratch per lane ({vgprs} vgprs)")

    def build(self, force: bool = False, verbose: bool = False) -> str:
        """hipcc --offload-arch=gfx950 -shared of every output (cross-compiles without a GPU), the checks on the device assembly of
        that very compile, then the libraries and the stamp moved into place.  Returns the path of the first output."""
        if not force and not self.stale():
            return self.paths[0]
        hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
        if not os.path.exists(hipcc):
            raise TamfBuildError(f"hipcc not found: cannot build {self.outputs[0].file}")
        os.makedirs(LIB_DIR, exist_ok=True)
        import fcntl
        import tempfile

        from . import _isa_check

        # one builder at a time (the ranks of a multi-GPU launch all import this module): the others wait and then find it fresh
        with open(self.paths[0] + ".lock", "w") as lock:  # (closing it releases the lock)
            fcntl.flock(lock, fcntl.LOCK_EX)
            if not force and not self.stale():
                return self.paths[0]
            with tempfile.TemporaryDirectory(prefix="tamf_build_", dir=LIB_DIR) as wd:
                built = self._compile_all(hipcc, wd)
                safe = False
                if self.counted_waits:
                    try:
                        _check_counted_waits([asm for _, asm in built], verbose)
                    except (_isa_check.IsaMismatch, IndexError, KeyError, ValueError) as e:  # (a newer hipcc may also break the checker's parsing)
                        import warnings

                        warnings.warn(f"{self.name}: {e}\nrebuilding with -DTAMF_CLIP_SAFE_WAIT (counted waits -> vmcnt(0))")
                        for o in self.outputs:
                            shutil.rmtree(os.path.join(wd, o.file), ignore_errors=True)
                        built = self._compile_all(hipcc, wd, ["-DTAMF_CLIP_SAFE_WAIT"])
                        safe = True
                if self.kernels:
                    self._report_kernels(built[0][1], verbose)
                digest = self.digest()  # (of the sources as they are now: an edit during the compile makes the stamp differ next time)
                for (out, _), path in reversed(list(zip(built, self.paths))):  # (the first output last, then the stamp)
                    os.replace(out, path)
                with open(self.stamp_path + ".tmp", "w") as f:
                    f.write(digest + "\n")
                os.replace(self.stamp_path + ".tmp", self.stamp_path)
        if verbose:
            print("built", " and ".join(self.paths[:1] + [o.file for o in self.outputs[1:]]) + (" (safe waits)" if safe else ""))
        return self.paths[0]


SAMPLER = Library("libtamf_hip", "tamf_hip.hip", ("tamf_hip.h", "tamf_hip_test.h"),
                  (Output("libtamf_hip.so", (), EXPORTS), Output("libtamf_hip_hooks.so", ("-DTAMF_TEST_HOOKS",), EXPORTS + HOOK_EXPORTS)),
                  counted_waits=True)
EVAL = Library("libtamf_eval", "tamf_eval.hip", ("tamf_eval.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
               (Output("libtamf_eval.so", (), EVAL_EXPORTS),),
               kernels=("_Z23voxelize_lattice_kernel", "_Z26mesh_contains_count_kernel"))
MANO = Library("libtamf_mano", "tamf_mano.hip", ("tamf_mano.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
               (Output("libtamf_mano.so", (), MANO_EXPORTS),),
               kernels=("_Z19mano_forward_kernelILi1EE", "_Z19mano_forward_kernelILi2EE", "_Z19mano_forward_kernelILi4EE"))
POINTENC = Library("libtamf_pointenc", "tamf_pointenc.hip", ("tamf_pointenc.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                   (Output("libtamf_pointenc.so", (), POINTENC_EXPORTS),),
                   kernels=("_Z10fps_kernelILi8ELb1EE", "_Z10fps_kernelILi16ELb1EE", "_Z10fps_kernelILi32ELb0EE", "_Z12group_kernel", "_Z15f32_gemm_kernelI5PeEpiE", "_Z11attn_kernel"))
TEXTENC = Library("libtamf_textenc", "tamf_textenc.hip", ("tamf_textenc.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                  (Output("libtamf_textenc.so", (), TEXTENC_EXPORTS),),
                  kernels=("_Z12embed_kernel", "_Z9ln_kernel", "_Z15f32_gemm_kernelI5TeEpiE", "_Z11attn_kernel"))
ENCTRAIN = Library("libtamf_enctrain", "tamf_enctrain.hip", ("tamf_enctrain.h", "tamf_hip.h"),  # (tamf_hip.h for tamf_status and tamf_arch)
                   (Output("libtamf_enctrain.so", (), ENCTRAIN_EXPORTS),),
                   kernels=("_Z10lin_kernel", "_Z12wgrad_kernel", "_Z15attn_fwd_kernel", "_Z17attn_bwd_q_kernel", "_Z18attn_bwd_kv_kernel"))
CONTACT = Library("libtamf_contact", "tamf_contact.hip", ("tamf_contact.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                  (Output("libtamf_contact.so", (), CONTACT_EXPORTS),),
                  kernels=("_Z18contact_h2o_kernel", "_Z18contact_o2h_kernel", "_Z23contact_backward_kernel"))
REFINETRAIN = Library("libtamf_refinetrain", "tamf_refinetrain.hip", ("tamf_refinetrain.h", "tamf_hip.h"),  # (tamf_hip.h for tamf_status and tamf_arch)
                      (Output("libtamf_refinetrain.so", (), REFINETRAIN_EXPORTS),),
                      kernels=("_Z13tg_lin_kernelILb0EE", "_Z13tg_lin_kernelILb1EE", "_Z15tg_wgrad_kernel", "_Z18tg_attn_fwd_kernel", "_Z20tg_attn_bwd_q_kernel",
                               "_Z21tg_attn_bwd_kv_kernel"))
MDMTRAIN = Library("libtamf_mdmtrain", "tamf_mdmtrain.hip", ("tamf_mdmtrain.h", "tamf_hip.h"),  # (tamf_hip.h for tamf_status and tamf_arch)
                   (Output("libtamf_mdmtrain.so", (), MDMTRAIN_EXPORTS),),
                   kernels=("_Z13tg_lin_kernelILb0EE", "_Z13tg_lin_kernelILb1EE", "_Z15tg_wgrad_kernel", "_Z18tg_attn_fwd_kernelILi64EE",
                            "_Z18tg_attn_fwd_kernelILi128EE", "_Z20tg_attn_bwd_q_kernelILi64EE", "_Z20tg_attn_bwd_q_kernelILi128EE",
                            "_Z21tg_attn_bwd_kv_kernelILi64EE", "_Z21tg_attn_bwd_kv_kernelILi128EE"))
OPTIM = Library("libtamf_optim", "tamf_optim.hip", ("tamf_optim.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                (Output("libtamf_optim.so", (), OPTIM_EXPORTS),),
                kernels=("_Z18optim_sumsq_kernel", "_Z19optim_update_kernel", "_Z17optim_norm_kernel"))
RENDER = Library("libtamf_render", "tamf_render.hip", ("tamf_render.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                 (Output("libtamf_render.so", (), RENDER_EXPORTS),),
                 kernels=("_Z21render_project_kernel", "_Z20render_raster_kernelILb0EE", "_Z20render_raster_kernelILb1EE", "_Z20render_points_kernelILb0EE",
                          "_Z20render_points_kernelILb1EE", "_Z24render_shade_mesh_kernelILb0EE", "_Z24render_shade_mesh_kernelILb1EE",
                          "_Z23render_composite_kernel", "_Z21render_resolve_kernel"))
SURFACE = Library("libtamf_surface", "tamf_surface.hip", ("tamf_surface.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                  (Output("libtamf_surface.so", ("-ffp-contract=off",), SURFACE_EXPORTS),),
                  kernels=("_Z24surface_area_scan_kernel", "_Z20surface_carry_kernel", "_Z24surface_add_carry_kernel", "_Z21surface_sample_kernel"))
MESHDIST = Library("libtamf_meshdist", "tamf_meshdist.hip", ("tamf_meshdist.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                   (Output("libtamf_meshdist.so", ("-ffp-contract=off",), MESHDIST_EXPORTS),),
                   kernels=("_Z24md_inside_prepare_kernel", "_Z22meshdist_points_kernel", "_Z23meshdist_lattice_kernel"))
SDFGRID = Library("libtamf_sdfgrid", "tamf_sdfgrid.hip", ("tamf_sdfgrid.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                  (Output("libtamf_sdfgrid.so", ("-ffp-contract=off",), SDFGRID_EXPORTS),),
                  kernels=("_Z22sdfgrid_forward_kernel", "_Z23sdfgrid_backward_kernel"))
WINDING = Library("libtamf_winding", "tamf_winding.hip", ("tamf_winding.h", "tamf_hip.h"),  # (tamf_hip.h for the tamf_status enum)
                  (Output("libtamf_winding.so", ("-ffp-contract=off",), WINDING_EXPORTS),),
                  kernels=("_Z21winding_points_kernelILb0EE", "_Z21winding_points_kernelILb1EE", "_Z21winding_reduce_kernel", "_Z22winding_lattice_kernel"))
LIBRARIES = (SAMPLER, EVAL, MANO)  # the sampling and evaluation path
PREPROCESSING = (POINTENC,)  # what prepares a run's inputs (launch/embed_objects.py); described, built and loaded the same way
TEXT_PREPROCESSING = (TEXTENC,)  # the same for the prompts (launch/embed_text.py)
TRAINING = (ENCTRAIN, CONTACT)  # the SegmentEncoder training step (launch/train_encoder.py); the contact-distance losses (contact.py)
REFINE_TRAINING = (REFINETRAIN,)  # the refiner's training step (model/segment_refine_train.py); a group of its own: tests pin TRAINING to two
DENOISER_TRAINING = (MDMTRAIN,)  # the denoiser's training step (model/interaction_segment_mdm_train.py); a group of its own for the same reason
OPTIMISER = (OPTIM,)  # the optimiser step of the train / train_refine launchers (optim.py); a group of its own for the same reason
RENDERING = (RENDER,)  # the offscreen renderer behind launch/render_samples.py (render.py); a group of its own for the same reason
OBJECT_PREPROCESSING = (SURFACE,)  # the surface sampler behind launch/sample_object_points.py (surface.py); a group of its own for the same reason
OBJECT_DISTANCE = (MESHDIST,)  # the point-to-mesh distance behind the PD score, process_sdf and the penetration map (meshdist.py); a group of its own for the same reason
PENETRATION_LOSS = (SDFGRID,)  # the SDF-lattice sampler behind the training losses' `pen` term (sdfgrid.py); a group of its own for the same reason
OBJECT_SIGN = (WINDING,)  # the winding-number inside test for open and scanned object meshes (winding.py); a group of its own for the same reason


def build(force: bool = False, verbose: bool = False) -> str:
    """Every library, the sampler pair first, each only when ITS sources changed.  One library at a time.  Returns LIB_PATH."""
    for lib in LIBRARIES + PREPROCESSING + TEXT_PREPROCESSING + TRAINING + REFINE_TRAINING + DENOISER_TRAINING + OPTIMISER + RENDERING + OBJECT_PREPROCESSING + OBJECT_DISTANCE + PENETRATION_LOSS + OBJECT_SIGN:
        lib.build(force, verbose)
    return LIB_PATH


def build_mano(force: bool = False, verbose: bool = False) -> str:
    """libtamf_mano.so alone.  Returns its path."""
    return MANO.build(force, verbose)


_lock = threading.Lock()
_loaded = {}  # output file name -> CDLL


def _load(lib: Library, file: str) -> ctypes.CDLL:
    """One output of `lib`, that library built first when missing or stale (and no other).  Raises - never falls back to a CPU path."""
    with _lock:
        if file not in _loaded:
            lib.build()
            # torch ships its own libamdhip64; import it first so that the library binds to the HIP runtime
            # instance torch uses (one runtime per process: shared device memory, streams, contexts).
            import torch  # noqa: F401

            _loaded[file] = ctypes.CDLL(os.path.join(LIB_DIR, file))
        return _loaded[file]


def load() -> ctypes.CDLL:
    """libtamf_hip.so (include/tamf_hip.h)"""
    return _load(SAMPLER, "libtamf_hip.so")


def load_hooks() -> ctypes.CDLL:
    """The -DTAMF_TEST_HOOKS build (include/tamf_hip_test.h): tests/, tools/ and bench.py's register-only MFMA probe.  A separate
    library object with its own process-global state (guard-band mode, kernel-selection word): contexts created through it are
    independent of contexts of libtamf_hip.so."""
    return _load(SAMPLER, "libtamf_hip_hooks.so")


def load_eval() -> ctypes.CDLL:
    """libtamf_eval.so (include/tamf_eval.h).  Independent of load(): neither needs the other."""
    return _load(EVAL, "libtamf_eval.so")


def load_mano_lib() -> ctypes.CDLL:
    """libtamf_mano.so (include/tamf_mano.h).  Independent of load() and load_eval()."""
    return _load(MANO, "libtamf_mano.so")


def load_pointenc() -> ctypes.CDLL:
    """libtamf_pointenc.so (include/tamf_pointenc.h).  Independent of the other libraries."""
    return _load(POINTENC, "libtamf_pointenc.so")


def load_textenc() -> ctypes.CDLL:
    """libtamf_textenc.so (include/tamf_textenc.h).  Independent of the other libraries."""
    return _load(TEXTENC, "libtamf_textenc.so")


def load_enctrain() -> ctypes.CDLL:
    """libtamf_enctrain.so (include/tamf_enctrain.h).  Independent of the other libraries."""
    return _load(ENCTRAIN, "libtamf_enctrain.so")


def load_contact() -> ctypes.CDLL:
    """libtamf_contact.so (include/tamf_contact.h).  Independent of the other libraries."""
    return _load(CONTACT, "libtamf_contact.so")


def load_refinetrain() -> ctypes.CDLL:
    """libtamf_refinetrain.so (include/tamf_refinetrain.h).  Independent of the other libraries."""
    return _load(REFINETRAIN, "libtamf_refinetrain.so")


def load_mdmtrain() -> ctypes.CDLL:
    """libtamf_mdmtrain.so (include/tamf_mdmtrain.h).  Independent of the other libraries."""
    return _load(MDMTRAIN, "libtamf_mdmtrain.so")


def load_optim() -> ctypes.CDLL:
    """libtamf_optim.so (include/tamf_optim.h).  Independent of the other libraries."""
    return _load(OPTIM, "libtamf_optim.so")


def load_render() -> ctypes.CDLL:
    """libtamf_render.so (include/tamf_render.h).  Independent of the other libraries."""
    return _load(RENDER, "libtamf_render.so")


def load_surface() -> ctypes.CDLL:
    """libtamf_surface.so (include/tamf_surface.h).  Independent of the other libraries."""
    return _load(SURFACE, "libtamf_surface.so")


def load_meshdist() -> ctypes.CDLL:
    """libtamf_meshdist.so (include/tamf_meshdist.h).  Independent of the other libraries."""
    return _load(MESHDIST, "libtamf_meshdist.so")


def load_sdfgrid() -> ctypes.CDLL:
    """libtamf_sdfgrid.so (include/tamf_sdfgrid.h).  Independent of the other libraries."""
    return _load(SDFGRID, "libtamf_sdfgrid.so")


def load_winding() -> ctypes.CDLL:
    """libtamf_winding.so (include/tamf_winding.h).  Independent of the other libraries."""
    return _load(WINDING, "libtamf_winding.so")


def load_from(path: str) -> ctypes.CDLL:
    """Bind the process to another build of the library, given explicitly by the caller, before the first load().  For the
    measurement scripts under tools/ (two builds alternating on one box, debug builds with timeline stamps; tools/ab_build.sh
    compiles them with -DTAMF_TEST_HOOKS): it stands for BOTH libraries.  The product path never calls this and reads no
    environment variable."""
    with _lock:
        if any(o.file in _loaded for o in SAMPLER.outputs):
            raise RuntimeError("libtamf_hip is already loaded in this process")
        import torch  # noqa: F401

        lib = ctypes.CDLL(path)
        for o in SAMPLER.outputs:
            _loaded[o.file] = lib
        return lib
