"""CPU: the context-free error slot of libtamf_hip.so (tamf_last_error(NULL)) belongs to the calling thread.

include/tamf_hip.h lets contexts be driven from different threads and the library takes no process-wide lock, so two threads can
fail at the same time - a refused tamf_ctx_create, a bad shape to tamf_power_spectrum_sum from a scoring worker.  Each must read
its own message.  The calls below return before any HIP call, so no GPU is needed."""
import ctypes
import os
import re
import threading

from oakink2_tamf_amd import _lib

TAMF_ERR_INVALID = -1
CALLS = 2000


def _library():
    lib = _lib.load()
    lib.tamf_last_error.restype = ctypes.c_char_p
    lib.tamf_last_error.argtypes = [ctypes.c_void_p]
    return lib  # (the calls below pass None and small ints only: right with or without the argtypes hip_backend sets)


def test_the_shape_checks_come_before_any_hip_call():
    """what lets the test below run without a GPU: the two shape checks are the first two statements of tamf_power_spectrum_sum"""
    src = open(os.path.join(_lib.CSRC, "tamf_hip.hip")).read()
    body = src[src.index('extern "C" int tamf_power_spectrum_sum('):]
    body = body[body.index("{\n") + 2:]
    first, second = body.split("\n")[:2]
    assert first.startswith("  if (N < 1 || F < 1) return fail(nullptr, TAMF_ERR_INVALID, \"bad shape (N = \"")
    assert second.startswith("  if (T < 3) return fail(nullptr, TAMF_ERR_INVALID, \"T = \"")
    assert re.search(r"^static thread_local std::string g_noctx_err;", src, flags=re.M)


def test_two_threads_failing_at_once_each_read_their_own_message():
    lib = _library()
    barrier = threading.Barrier(2)
    bad = {"a": [], "b": []}

    def worker(name, N, T, F, ok):
        barrier.wait()
        for i in range(CALLS):  # (ctypes releases the GIL during both calls: the threads overlap)
            rc = lib.tamf_power_spectrum_sum(None, None, N, T, F, 0, None, None, None)
            msg = lib.tamf_last_error(None).decode()
            if rc != TAMF_ERR_INVALID or not ok(msg):
                bad[name].append((i, rc, msg))

    threads = [threading.Thread(target=worker, args=("a", 0, 8, 1, lambda m: m == "bad shape (N = 0, F = 1)")),
               threading.Thread(target=worker, args=("b", 1, 2, 1, lambda m: m.startswith("T = 2:")))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not bad["a"] and not bad["b"], (len(bad["a"]), bad["a"][:3], len(bad["b"]), bad["b"][:3])


def test_a_refused_create_is_read_back_on_the_same_thread():
    lib = _library()
    assert lib.tamf_ctx_create(None, 1, 8, 0, 0, None) == TAMF_ERR_INVALID
    assert lib.tamf_last_error(None) == b"null argument"
