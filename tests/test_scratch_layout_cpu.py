"""CPU: scratch_layout (csrc/tamf_shapes.h) - where Q | K, the attention output and the input-merge rows of a sampler context live:
views of the hidden operand's allocation when they fit, allocations of their own otherwise.  A stand-alone program includes the
header (plain host code); checked over the architectures (d, ff), the operand widths, guard-band mode and every context size from one
clip of one frame to 64 clips of 208 rows."""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT


PAIRS = [(128, 256), (128, 384), (128, 512), (256, 1024), (512, 2048)]  # (d, ff): ARCH_TINY, ff = 3 d exactly, the test arch, arch_mdm / arch_refine, arch_mdm_l
SIZES = [(1, 1), (1, 2), (2, 16), (3, 20), (3, 160), (7, 33), (31, 97), (32, 160), (64, 160), (64, 196), (64, 203)]  # (clips, frames), G: 5 prefix rows
FIELDS = ("alias", "host", "qk_off", "a_off", "h1_off", "qk_bytes", "a_bytes", "h1_bytes", "hidden_bytes")


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    """{(d, ff, eb, guard, B, T): dict of the layout's fields}, from one run of the stand-alone program"""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    main = r"""
#include <cstdio>
#include "tamf_shapes.h"
int main() {
  int d, ff, eb, guard, B, T;
  while (scanf("%d %d %d %d %d %d", &d, &ff, &eb, &guard, &B, &T) == 6) {
    const long long Sp = (T + 5 + 7) / 8 * 8;
    const ScratchLayout s = scratch_layout(B * Sp, (long long)B * T, d, ff, eb, guard);
    printf("%d %d %d %d %d %d : %d %llu %llu %llu %llu %llu %llu %llu %llu\n", d, ff, eb, guard, B, T, (int)s.alias, s.host_bytes,
           s.qk_off, s.a_off, s.h1_off, s.qk_bytes, s.a_bytes, s.h1_bytes, s.hidden_bytes);
  }
  return 0;
}
"""
    tmp = tmp_path_factory.mktemp("layout")
    (tmp / "m.cpp").write_text(main)
    subprocess.run([cxx, "-std=c++17", "-O0", "-Wall", "-I", os.path.join(ROOT, "oakink2-tamf_amd", "csrc"), "-o", str(tmp / "m"), str(tmp / "m.cpp")], check=True)
    cases = [(d, ff, eb, g, B, T) for d, ff in PAIRS for eb in (2, 4) for g in (0, 256) for B, T in SIZES]
    out = subprocess.run([str(tmp / "m")], input="".join("%d %d %d %d %d %d\n" % c for c in cases), check=True, capture_output=True, text=True).stdout
    res = {}
    for line in out.strip().split("\n"):
        key, val = line.split(":")
        res[tuple(int(v) for v in key.split())] = dict(zip(FIELDS, (int(v) for v in val.split())))
    assert sorted(res) == sorted(cases)
    return res


def _sizes(d, ff, eb, B, T):
    M = B * ((T + 5 + 7) // 8 * 8)
    return M * ff * eb, M * 2 * d * eb, M * d * eb, B * T * d * eb


def test_aliasing_is_on_exactly_when_everything_fits(layouts):
    for (d, ff, eb, g, B, T), s in layouts.items():
        hidden, qk, a, h1 = _sizes(d, ff, eb, B, T)
        assert bool(s["alias"]) == (qk + a <= hidden and h1 <= qk), (d, ff, eb, g, B, T)
        assert bool(s["alias"]) == (ff >= 3 * d)  # in whole rows: the three real architectures and the test arch alias, ARCH_TINY does not
        assert (s["hidden_bytes"], s["qk_bytes"], s["a_bytes"], s["h1_bytes"]) == (hidden, qk, a, h1)  # (all whole 256-byte units already)
        if not s["alias"]:
            assert s["host"] == hidden  # every buffer an allocation of its own, the hidden operand as before


def test_views_are_aligned_disjoint_and_inside_the_allocation(layouts):
    for key, s in layouts.items():
        if not s["alias"]:
            continue
        g = key[3]
        views = {n: (s[n + "_off"], s[n + "_off"] + s[n + "_bytes"]) for n in ("qk", "a", "h1")}
        for n, (lo, hi) in views.items():
            assert lo % 256 == 0 and hi % 256 == 0 and 0 <= lo < hi <= s["host"], (key, n)
        assert views["qk"][1] <= views["a"][0] or views["a"][1] <= views["qk"][0], key  # both live during attention
        assert s["host"] >= s["hidden_bytes"] and s["host"] % 256 == 0
        if g == 0:  # the point of it: no scratch byte beyond the hidden operand's own
            assert s["host"] == s["hidden_bytes"]
            assert views["h1"][0] >= views["qk"][0] and views["h1"][1] <= views["qk"][1]  # h1 shares Q | K's bytes
        else:
            # margins [lo - g, lo) and [hi, hi + g) of every view: outside every view and outside the hidden operand (whose every byte
            # FFN1 stores); the one behind the last view is the allocation's own upper margin
            spans = list(views.values()) + [(0, s["hidden_bytes"])]
            for n, (lo, hi) in views.items():
                for mlo, mhi in ((lo - g, lo), (hi, hi + g)):
                    assert mlo >= 0, (key, n)
                    assert mhi <= s["host"] or mlo == s["host"], (key, n)
                    for vlo, vhi in spans:
                        assert mhi <= vlo or mlo >= vhi, (key, n, (mlo, mhi), (vlo, vhi))
            for x, y in (("qk", "a"), ("qk", "h1"), ("a", "h1")):  # with margins no two views share a byte
                assert views[x][1] + g <= views[y][0] or views[y][1] + g <= views[x][0], key
