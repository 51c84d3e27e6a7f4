"""CPU: the host-only halves of the sampler library - csrc/tamf_weight_prep.h (checkpoint key set, operand packing, deferred-LayerNorm
fold, composed input map) and csrc/tamf_shapes.h (sequence shape of a call and of the workspaces).  One stand-alone driver program
includes the two headers, reads cases from stdin and prints results; it is built with the host sanitizers (address, undefined) by the
clang++ that ships beside hipcc (the packer needs _Float16) and run directly.  Floats cross the pipe as their 32 bits in hex."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from oracle import mdm_oracle as O

CSRC = os.path.join(ROOT, "oakink2-tamf_amd", "csrc")
F32, BF16, BF16X3, F16X3 = 0, 1, 2, 3  # tamf_precision
ERR_INVALID, ERR_RANGE = -1, -6  # tamf_status
KINDS = {"G": 0, "R": 1, "E": 2}

DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "tamf_weight_prep.h"
#include "tamf_shapes.h"

static int rd_int() {
  int v = 0;
  if (scanf("%d", &v) != 1) exit(3);
  return v;
}
static std::vector<float> rd(size_t n) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) {
    unsigned u = 0;
    if (scanf("%x", &u) != 1) exit(3);
    memcpy(&v[i], &u, 4);
  }
  return v;
}
static void wr(const float* p, size_t n) {
  for (size_t i = 0; i < n; ++i) {
    unsigned u;
    memcpy(&u, p + i, 4);
    printf("%08x ", u);
  }
  printf("\n");
}
int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    const std::string c = cmd;
    if (c == "pack") {
      const int prec = rd_int(), N = rd_int(), K = rd_int(), ldk = rd_int();
      const std::vector<float> w = rd((size_t)N * K);
      const PackedOperand po = pack_operand(prec, w.data(), N, K, ldk);
      unsigned sb;
      memcpy(&sb, &po.inv_scale, 4);
      printf("%d %d %08x %zu %zu %d\n", (int)po.refused, po.error_code(), sb, po.nonzero, po.small, (int)po.small_share_noted());
      printf("%s\n", po.refused ? po.error_message("W.test").c_str() : po.small_share_noted() ? po.range_note("W.test").c_str() : "-");
      printf("x");
      for (unsigned char b : po.image) printf("%02x", b);
      printf("\n");
    } else if (c == "fold") {
      const int N = rd_int(), Npad = rd_int(), d = rd_int(), hg = rd_int(), hb = rd_int();
      const std::vector<float> W = rd((size_t)N * d), b = rd(N), g = rd(hg ? d : 0), be = rd(hb ? d : 0);
      const FoldedLinear f = fold_layernorm(W.data(), b.data(), N, Npad, d, hg ? g.data() : nullptr, hb ? be.data() : nullptr);
      wr(f.w.data(), f.w.size());
      wr(f.c2.data(), f.c2.size());
    } else if (c == "compose") {
      const int mk = rd_int(), col0 = rd_int(), d = rd_int(), K = rd_int(), ld_n = rd_int(), ld_k = rd_int(), nout = rd_int();
      const std::vector<float> Wm1 = rd((size_t)d * mk), Wx = rd((size_t)d * K);
      std::vector<float> out(nout, 0.f);
      compose_block(Wm1.data(), mk, col0, d, Wx.data(), K, out.data(), ld_n, ld_k);
      wr(out.data(), out.size());
    } else if (c == "bias") {
      const int nb = rd_int(), d = rd_int();
      const std::vector<float> Wm1 = rd((size_t)d * nb * d), bm1 = rd(d);
      std::vector<std::vector<float>> bx;
      for (int i = 0; i < nb; ++i) bx.push_back(rd(d));
      const float* p[3] = {bx[0].data(), bx[1].data(), nb > 2 ? bx[2].data() : nullptr};
      const std::vector<float> a = input_bias_term_by_term(Wm1.data(), nb * d, d, bm1.data(), p, nb);
      wr(a.data(), a.size());
      if (nb == 2) {
        std::vector<float> e(d);
        input_bias_two_terms_per_column(Wm1.data(), d, bm1.data(), p[0], p[1], e.data());
        wr(e.data(), e.size());
      }
    } else if (c == "shapes") {
      tamf_arch a{};
      a.input_dim = rd_int(); a.obj_input_dim = rd_int(); a.hand_shape_dim = rd_int(); a.obj_embed_dim = rd_int();
      a.latent_dim = rd_int(); a.ff_size = rd_int(); a.num_layers = rd_int(); a.num_heads = rd_int();
      a.clip_dim = rd_int(); a.h2o_dim = rd_int(); a.kind = rd_int();
      for (const auto& kv : expected_shapes(a)) {
        printf("%s", kv.first.c_str());
        for (long long v : kv.second) printf(" %lld", v);
        printf("\n");
      }
      printf("end\n");
    } else if (c == "seq") {
      const int T = rd_int(), P = rd_int();
      const SeqShape s = seq_shape(T, P), m = seq_shape_max(T, P);
      printf("%d %d %d %d %d %d %d\n", s.S, s.Sp, s.Skp, vt_row_keys(s.S, s.Sp), m.S, m.Sp, m.Skp);
    } else if (c == "fit") {
      const int B = rd_int(), T = rd_int(), ff = rd_int(), d = rd_int();
      printf("%d\n", (int)dims_fit_32bit_offsets(B, T, ff, d));
    } else {
      return 2;
    }
  }
  return 0;
}
"""


def _clangxx():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
    for cand in (os.path.join(rocm, "llvm", "bin", "clang++"), os.path.join(rocm, "lib", "llvm", "bin", "clang++"), "/opt/rocm/llvm/bin/clang++"):
        if os.path.exists(cand):
            return cand
    raise AssertionError("no clang++ beside hipcc")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """run(text) -> the driver's output lines; the program is built once"""
    tmp = tmp_path_factory.mktemp("weight_prep")
    (tmp / "driver.cpp").write_text(DRIVER)
    exe = str(tmp / "driver")
    subprocess.run([_clangxx(), "-std=c++17", "-O1", "-fsanitize=address,undefined", "-I", CSRC, "-o", exe, str(tmp / "driver.cpp")], check=True)

    def run(text):
        res = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert res.returncode == 0 and "runtime error" not in res.stderr and "Sanitizer" not in res.stderr, res.stderr[-2000:]
        return res.stdout.split("\n")

    return run


def _hex(a):
    return " ".join(map("{:08x}".format, np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32).tolist()))


def _floats(line, shape=None):
    a = np.array([int(t, 16) for t in line.split()], dtype=np.uint32).view(np.float32)
    return a if shape is None else a.reshape(shape)


def _pack(driver, prec, w, ldk):
    """-> dict(refused, code, inv_scale, nonzero, small, noted, text, image: uint8 array) of pack_operand(prec, w [N][K], ldk)"""
    N, K = w.shape
    head, text, image = driver("pack %d %d %d %d %s\n" % (prec, N, K, ldk, _hex(w)))[:3]
    refused, code, sb, nonzero, small, noted = head.split()
    return dict(refused=int(refused), code=int(code), inv_scale=float(np.array([int(sb, 16)], np.uint32).view(np.float32)[0]), nonzero=int(nonzero),
                small=int(small), noted=bool(int(noted)), text=text, image=np.frombuffer(bytes.fromhex(image[1:]), np.uint8))


def _planes(image, N, K, ldk):
    """hi and lo [N][K] uint16 of a split-mode image: element (r, k) at (idx >> 5) * 64 + (idx & 31), its lo 32 halves later"""
    h = image.view(np.uint16)
    idx = np.arange(N)[:, None] * ldk + np.arange(K)[None, :]
    o = (idx >> 5) * 64 + (idx & 31)
    return h[o], h[o + 32], o


def _weights():
    """[16][128]: seeded normal weights at 0.04 and the edge values: tiny, signed zeros, beyond fp16, below every format, 64 exact ties"""
    rng = np.random.default_rng(0)
    edge = np.array([1e-6, -1e-6, 0.0, -0.0, 7e4, -7e4, 1e-30, -1e-30], np.float32)
    ties = (0x3F808000 + np.arange(64, dtype=np.uint32) * 0x10000).astype(np.uint32).view(np.float32)  # halfway between two bf16 values
    w = np.concatenate([edge, ties, (0.04 * rng.standard_normal(16 * 128 - 72)).astype(np.float32)])
    return rng.permutation(w).reshape(16, 128)


def _bits(t):
    return t.view(torch.int16).numpy().view(np.uint16)


def test_bf16_and_bf16x3_packing_is_torch_rounding(driver):
    w = _weights()
    tw = torch.from_numpy(w)
    hi_ref = tw.to(torch.bfloat16)
    lo_ref = (tw - hi_ref.float()).to(torch.bfloat16)
    p = _pack(driver, BF16, w, 128)
    assert p["refused"] == 0 and p["inv_scale"] == 1.0 and not p["noted"]
    np.testing.assert_array_equal(p["image"].view(np.uint16).reshape(16, 128), _bits(hi_ref))
    p = _pack(driver, BF16X3, w, 128)
    assert p["refused"] == 0 and p["inv_scale"] == 1.0 and not p["noted"] and p["image"].size == 16 * 128 * 4
    hi, lo, _ = _planes(p["image"], 16, 128, 128)
    np.testing.assert_array_equal(hi, _bits(hi_ref))
    np.testing.assert_array_equal(lo, _bits(lo_ref))
    # NaN inputs (quiet, signalling with low payload bits only, negative): a NaN comes out, in both planes
    nan = np.array([0x7FC00000, 0x7F800001, 0xFFC00000, 0x7FA00000] * 8, np.uint32).view(np.float32).reshape(1, 32)
    for prec in (BF16, BF16X3):
        h = _pack(driver, prec, nan, 32)["image"].view(np.uint16)
        assert h.size == (32 if prec == BF16 else 64)
        assert ((h & 0x7F80) == 0x7F80).all() and ((h & 0x007F) != 0).all()


def test_f16x3_packing_scale_planes_refusal_and_note(driver):
    w = _weights()
    p = _pack(driver, F16X3, w, 128)
    wexp = 15 - int(np.frexp(np.abs(w).max())[1])
    assert wexp == -2 and p["refused"] == 0 and p["inv_scale"] == float(np.ldexp(np.float32(1), -wexp))
    scaled = np.ldexp(w, wexp).astype(np.float32)
    hi_ref = scaled.astype(np.float16)
    lo_ref = (scaled - hi_ref.astype(np.float32)).astype(np.float16)
    hi, lo, _ = _planes(p["image"], 16, 128, 128)
    np.testing.assert_array_equal(hi, hi_ref.view(np.uint16))
    np.testing.assert_array_equal(lo, lo_ref.view(np.uint16))
    # a non-finite weight: refused before anything is stored, with the C-ABI's code and message; the other modes take it
    for bad in (np.inf, -np.inf, np.nan):
        wb = w.copy()
        wb[3, 7] = bad
        p = _pack(driver, F16X3, wb, 128)
        assert p["code"] == ERR_RANGE and p["image"].size == 0
        assert p["text"] == "f16x3: weight W.test holds a non-finite value and cannot be stored as split-fp16 operands; use bf16x3 or f32"
        assert _pack(driver, BF16X3, wb, 128)["refused"] == 0
    # the weight-range note: 0.04s under one 7e4 outlier, not the plain tensor
    plain = np.full((32, 32), 0.04, np.float32)
    p = _pack(driver, F16X3, plain, 32)
    assert not p["noted"] and p["text"] == "-" and p["nonzero"] == 1024 and p["small"] == 0
    plain[5, 5] = 7e4
    p = _pack(driver, F16X3, plain, 32)
    assert p["noted"] and p["refused"] == 0 and (p["nonzero"], p["small"]) == (1024, 1023) and p["image"].size == 32 * 32 * 4
    assert p["text"] == ("f16x3: 99 % of the non-zero weights of W.test are below 2^-17.5 of the tensor's largest magnitude: stored with fewer "
                         "than 22 significand bits (an outlier dominates the per-tensor scale)")
    assert not _pack(driver, BF16X3, plain, 32)["noted"]
    z = _pack(driver, F16X3, np.zeros((2, 32), np.float32), 32)  # all zero: no scale, no note
    assert z["inv_scale"] == 1.0 and not z["noted"] and not z["image"].any()


@pytest.mark.parametrize("N,K,ldk", [(3, 5, 32), (2, 33, 64), (128, 99, 128)])
def test_operand_layout(driver, N, K, ldk):
    rng = np.random.default_rng(N * 1000 + K)
    w = (0.04 * rng.standard_normal((N, K))).astype(np.float32)
    w[w == 0] = 0.04  # (no zero weight: a zero in the image is padding)
    for prec in (BF16X3, F16X3):
        image = _pack(driver, prec, w, ldk)["image"]
        assert image.size == N * ldk * 4
        hi, lo, o = _planes(image, N, K, ldk)
        assert (hi != 0).all()  # every element where the layout says (values: the packing tests)
        if prec == BF16X3:
            np.testing.assert_array_equal(hi, _bits(torch.from_numpy(w).to(torch.bfloat16)))
        rest = image.view(np.uint16).copy()
        rest[o] = 0
        rest[o + 32] = 0
        assert not rest.any()  # everything else is zero
    f = _pack(driver, F32, w, ldk)["image"].view(np.float32).reshape(N, ldk)
    np.testing.assert_array_equal(f[:, :K].view(np.uint32), w.view(np.uint32))
    assert not f[:, K:].view(np.uint32).any()
    b = _pack(driver, BF16, w, ldk)["image"].view(np.uint16).reshape(N, ldk)
    np.testing.assert_array_equal(b[:, :K], _bits(torch.from_numpy(w).to(torch.bfloat16)))
    assert not b[:, K:].any()
    for prec in (F32, BF16, BF16X3, F16X3):  # a leading dimension that is no multiple of 32
        p = _pack(driver, prec, w, ldk + 8)
        assert p["code"] == ERR_INVALID and p["image"].size == 0 and p["text"] == "operand leading dimension must be a multiple of 32"


def _assert_within_one_ulp(got, ref64, what):
    """every element of the fp32 result within one fp32 ulp of the float64 value (one rounding of a float64 sum: half an ulp plus a
    summation-order term of order d * 2^-53)"""
    err = np.abs(got.astype(np.float64) - ref64)
    ulp = np.spacing(np.abs(ref64).astype(np.float32)).astype(np.float64)
    worst = float((err / ulp).max())
    print("%s: worst error %.8f ulp, bit-equal to float32(float64 value): %s" % (what, worst, bool((got == ref64.astype(np.float32)).all())))
    assert (err <= ulp).all(), (what, worst)


@pytest.mark.parametrize("N,d", [(384, 128), (1024, 256), (99, 512)])
def test_layernorm_fold_against_float64(driver, N, d):
    rng = np.random.default_rng(N + d)
    W = (0.04 * rng.standard_normal((N, d))).astype(np.float32)
    b = (0.02 * rng.standard_normal(N)).astype(np.float32)
    g = (1.0 + 0.1 * rng.standard_normal(d)).astype(np.float32)
    be = (0.1 * rng.standard_normal(d)).astype(np.float32)
    Npad = (N + 127) // 128 * 128  # (99 -> 128: the output head's padding)
    out = driver("fold %d %d %d 1 1 %s %s %s %s\n" % (N, Npad, d, _hex(W), _hex(b), _hex(g), _hex(be)))
    w2, c2 = _floats(out[0], (Npad, d)), _floats(out[1])
    Wg = W.astype(np.float64) * g.astype(np.float64)
    _assert_within_one_ulp(w2[:N], Wg - Wg.mean(axis=1, keepdims=True), "fold weight (%d, %d)" % (N, d))
    _assert_within_one_ulp(c2[:N], b.astype(np.float64) + W.astype(np.float64) @ be.astype(np.float64), "fold c2 (%d, %d)" % (N, d))
    assert c2.size == Npad and not w2[N:].view(np.uint32).any() and not c2[N:].view(np.uint32).any()  # rows beyond N are zero
    # no LayerNorm in front (layer 0's attention block): the plain weight and bias, bit for bit
    out = driver("fold %d %d %d 0 0 %s %s\n" % (N, N, d, _hex(W), _hex(b)))
    np.testing.assert_array_equal(_floats(out[0], (N, d)).view(np.uint32), W.view(np.uint32))
    np.testing.assert_array_equal(_floats(out[1]).view(np.uint32), b.view(np.uint32))


def test_compose_block_and_input_bias_against_float64(driver):
    d, K, mk, c0 = 128, 99, 384, 256
    rng = np.random.default_rng(7)
    Wm1 = (0.05 * rng.standard_normal((d, mk))).astype(np.float32)
    Wx = (0.1 * rng.standard_normal((d, K))).astype(np.float32)
    ref = Wm1[:, c0:c0 + d].astype(np.float64) @ Wx.astype(np.float64)
    ld = 128  # rows of the fused weight are XK >= K long: the columns beyond K stay as they were (zero)
    row = _floats(driver("compose %d %d %d %d %d 1 %d %s %s\n" % (mk, c0, d, K, ld, d * ld, _hex(Wm1), _hex(Wx)))[0], (d, ld))
    _assert_within_one_ulp(row[:, :K], ref, "compose_block, row-major")
    assert not row[:, K:].view(np.uint32).any()
    tr = _floats(driver("compose %d %d %d %d 1 %d %d %s %s\n" % (mk, c0, d, K, d, K * d, _hex(Wm1), _hex(Wx)))[0], (K, d))
    _assert_within_one_ulp(tr, ref.T, "compose_block, transposed")
    np.testing.assert_array_equal(tr.T, row[:, :K])  # the same sums in the same order
    # the fused bias b_m1 + sum_x W_m1[:, block x] b_x: term by term (G: 2 terms, R: 3) and the encoder's two terms per column
    bm1 = (0.02 * rng.standard_normal(d)).astype(np.float32)
    bx = [(0.1 * rng.standard_normal(d)).astype(np.float32) for _ in range(3)]
    for nb in (2, 3):
        W = np.ascontiguousarray(Wm1[:, :nb * d])
        ref_b = bm1.astype(np.float64) + sum(W[:, i * d:(i + 1) * d].astype(np.float64) @ bx[i].astype(np.float64) for i in range(nb))
        out = driver("bias %d %d %s %s %s\n" % (nb, d, _hex(W), _hex(bm1), " ".join(_hex(v) for v in bx[:nb])))
        _assert_within_one_ulp(_floats(out[0]), ref_b, "input bias, %d terms one after the other" % nb)
        if nb == 2:
            _assert_within_one_ulp(_floats(out[1]), ref_b, "input bias, two terms per column")


def _expected_shapes(driver, arch):
    out = driver("shapes %d %d %d %d %d %d %d %d %d %d %d\n" % tuple(arch))
    lines = out[:out.index("end")]
    return {l.split()[0]: tuple(int(v) for v in l.split()[1:]) for l in lines}


@pytest.mark.parametrize("name", ["ARCH_TINY", "ARCH_MDM", "ARCH_MDM_L", "ARCH_TINY_R", "ARCH_REFINE"])
def test_expected_shapes_equal_the_oracle_key_set(driver, name):
    a = getattr(O, name)
    got = _expected_shapes(driver, (a.input_dim, a.obj_input_dim, a.hand_shape_dim, a.obj_embed_dim, a.latent_dim, a.ff_size, a.num_layers,
                                    a.num_heads, a.clip_dim, a.h2o_dim, KINDS[a.kind]))
    spec = {k: tuple(v) for k, v in O.state_dict_spec(a).items()}
    if a.kind == "G":
        # the one key of a G checkpoint the library does not ask for: the timestep embedder holds the SAME positional-encoding module, so
        # its buffer appears a second time under this name; tamf_load_weight ignores it like every key it does not expect
        assert spec.pop("embed_timestep.sequence_pos_encoder.pe") == spec["sequence_pos_encoder.pe"]
    assert got == spec, set(got) ^ set(spec)


def test_expected_shapes_of_the_segment_encoder(driver):
    import yaml

    from oakink2_tamf_amd.model.segment_encoder import SegmentEncoder

    with open(os.path.join(ROOT, "config", "arch_encoder.yml")) as f:
        m = yaml.safe_load(f)["model"]
    sd = SegmentEncoder(17, **m).state_dict()
    got = _expected_shapes(driver, (m["input_dim"], m["obj_input_dim"], m["hand_shape_dim"], m["obj_embed_dim"], m["latent_dim"], m["ff_size"],
                                    m["num_layers"], m["num_heads"], 512, 778, KINDS["E"]))
    assert got == {k: tuple(v.shape) for k, v in sd.items()}, set(got) ^ set(sd)


def test_sequence_shape_and_the_workspace_bound(driver):
    cases = [(T, P) for P in (3, 5) for T in range(1, 209)]
    out = driver("".join("seq %d %d\n" % c for c in cases))
    res = {c: tuple(int(v) for v in l.split()) for c, l in zip(cases, out)}
    for (T, P), (S, Sp, Skp, keys, Smax, Spmax, Skpmax) in res.items():
        assert S == T + P and Sp == (S + 7) // 8 * 8 and Skp == keys and Skp % 32 == 0 and Skp >= S
        assert (Smax, Spmax) == (S, Sp) and Skpmax == (max(S, 208) + 31) // 32 * 32  # the floor: the largest clip tile
        # what alloc_workspaces reserves per V^T row for max_frames = Tmax holds the row of every call with T <= Tmax
        assert all(res[(Tmax, P)][6] >= Skp for Tmax in range(T, 209)), (T, P)
    # check_dims: 32-bit operand offsets, five prefix rows counted whatever the kind
    fits = [(64, 196, 1024, 256), (64, 203, 2048, 512), (2521, 203, 2048, 512), (2520, 203, 2048, 512), (1198, 1000, 256, 128), (1199, 1000, 256, 128),
            (1, 4990, 2048, 512), (5000, 100, 256, 128)]
    out = driver("".join("fit %d %d %d %d\n" % c for c in fits))
    for (B, T, ff, d), l in zip(fits, out):
        ok = B * ((T + 5 + 7) // 8 * 8) * max(ff, 3 * d) * 4 < 2 ** 32 and B * T * 896 * 4 < 2 ** 32
        assert int(l) == int(ok), (B, T, ff, d)
    assert {int(l) for l in out[:len(fits)]} == {0, 1}
