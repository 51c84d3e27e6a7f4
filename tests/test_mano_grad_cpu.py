"""CPU: the surface of libtamf_mano.so with the backward - the C header's function set, the export list and the symbols of the library
cross-compiled here (hipcc --offload-arch=gfx950, no GPU needed) agree, and tamf_mano_backward is among them."""
import os
import re
import subprocess

from conftest import ROOT


def test_header_export_list_and_built_library_agree():
    from oakink2_tamf_amd import _lib

    with open(os.path.join(ROOT, "include", "tamf_mano.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    declared = set(re.findall(r"\b(tamf_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(_lib.MANO_EXPORTS) and len(set(_lib.MANO_EXPORTS)) == len(_lib.MANO_EXPORTS)
    assert "tamf_mano_backward" in declared and "tamf_mano_forward" in declared
    path = _lib.build_mano()  # (builds when the sources changed: a compile error of the device code fails here)
    assert os.path.exists(path) and not _lib.MANO.stale()
    nm = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True)
    assert nm.returncode == 0
    syms = {ln.split()[-1] for ln in nm.stdout.splitlines() if " T " in ln}
    assert {s for s in syms if s.startswith("tamf_")} == set(_lib.MANO_EXPORTS)
    lib = _lib.load_mano_lib()
    assert lib.tamf_mano_backward is not None


def test_the_backward_kernel_is_in_the_device_code_and_the_forward_untouched_in_the_lists():
    from oakink2_tamf_amd import _lib

    # the device code of the backward lives in the forward's header: no new source file, no new entry in the reported kernels
    assert _lib.MANO.sources == ["tamf_device.h", "tamf_mano.h", "tamf_mano.hip"] and len(_lib.MANO.kernels) == 3
    with open(os.path.join(_lib.CSRC, "tamf_mano.h")) as f:
        src = f.read()
    assert "mano_backward_kernel" in src and "atomicAdd" not in src
    r = subprocess.run(["strings", _lib.build_mano()], capture_output=True, text=True)
    assert r.returncode == 0 and "mano_backward_kernel" in r.stdout


def test_differentiable_factory_is_exported():
    from oakink2_tamf_amd import mano as M

    assert "make_mano_differentiable" in M.__all__ and callable(M.make_mano_differentiable)
    import inspect

    sig = inspect.signature(M.HipManoLayer.__init__)
    assert sig.parameters["differentiable"].default is False
