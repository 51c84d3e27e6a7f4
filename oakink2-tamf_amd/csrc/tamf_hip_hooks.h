// The test and measurement entry points of libtamf_hip_hooks.so (include/tamf_hip_test.h) and everything that only they use: the
// tail of tamf_hip.hip in the -DTAMF_TEST_HOOKS build, included there once and nowhere else.  The product library does not parse
// this file.  What the hooks SET but product code reads (the guard-band and allocation-failure state of dev_alloc, the selection words
// g_krot / g_sel in tamf_launch.h, the list of live contexts, the launch lock) is defined in tamf_hip.hip and its headers.
#pragma once
#include "../../include/tamf_hip_test.h"

extern "C" int tamf_test_set_guard_bytes(int64_t bytes) {
  if (bytes < 0 || bytes > (1 << 20) || bytes % 256) return fail(nullptr, TAMF_ERR_INVALID, "guard bytes must be a multiple of 256 in [0, 1 MiB]");
  g_guard_bytes.store((size_t)bytes);
  return 0;
}

extern "C" int tamf_test_fail_alloc_after(int32_t n) {
  g_fail_alloc_in.store(n);
  return 0;
}
extern "C" int tamf_test_poke(tamf_ctx* ctx, int32_t alloc_index, int64_t offset, int32_t nbytes) {
  if (!ctx || alloc_index < 0 || (size_t)alloc_index >= ctx->guards.size() || nbytes <= 0) return fail(ctx, TAMF_ERR_INVALID, "bad argument");
  const GuardRec& g = ctx->guards[alloc_index];
  if (offset < -(int64_t)g.guard || offset + nbytes > (int64_t)(g.bytes + g.guard)) return fail(ctx, TAMF_ERR_INVALID, "outside the allocation and its margins");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipMemset(g.base + g.guard + offset, 0, nbytes));
  return 0;
}

extern "C" int tamf_test_check_guards(tamf_ctx* ctx, int32_t* n_checked) {
  if (!ctx) return fail(ctx, TAMF_ERR_INVALID, "null ctx");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  if (n_checked) *n_checked = (int32_t)ctx->guards.size();
  std::vector<unsigned char> host;
  int bad = 0;
  std::string report;
  for (size_t i = 0; i < ctx->guards.size(); ++i) {
    const GuardRec& g = ctx->guards[i];
    host.resize(g.guard);
    for (int side = 0; side < 2; ++side) {
      const char* src = side ? g.base + g.guard + g.bytes : g.base;
      HIPCHK(ctx, hipMemcpy(host.data(), src, g.guard, hipMemcpyDeviceToHost));
      size_t first = g.guard, last = 0, n = 0;
      for (size_t k = 0; k < g.guard; ++k)
        if (host[k] != GUARD_BYTE) {
          if (first == g.guard) first = k;
          last = k;
          ++n;
        }
      if (n) {
        ++bad;
        if (report.size() < 1500)
          report += std::string(report.empty() ? "" : "; ") + "allocation #" + std::to_string(i) + " [" + g.tag + "] of " +
                    std::to_string(g.bytes) + " bytes: " + std::to_string(n) + " bytes written " +
                    (side ? "BEYOND its end (offsets +" + std::to_string(first) + " .. +" + std::to_string(last) + ")"
                          : "BELOW its start (offsets -" + std::to_string(g.guard - first) + " .. -" + std::to_string(g.guard - last) + ")");
      }
    }
  }
  if (bad) return fail(ctx, TAMF_ERR_STATE, "out-of-bounds device stores: " + report);
  return 0;
}

// Every per-step scratch operand of a G / R context (Q | K, attention output, hidden activations, input-merge rows), through its current
// pointer and over its whole dimensioned size, set to `byte` (0xFF: a NaN in every operand format).  A step whose kernels read only what
// the same step wrote gives the same bits afterwards (tests/test_scratch_alias_gpu.py).
extern "C" int tamf_test_fill_scratch(tamf_ctx* ctx, int32_t byte) {
  TAMF_LAUNCH_LOCK;
  TRY(need_kind(ctx, __func__, KIND_G | KIND_R));
  if (byte < 0 || byte > 255) return fail(ctx, TAMF_ERR_INVALID, "byte must be in [0, 255]");
  HIPCHK(ctx, hipSetDevice(ctx->device));
  HIPCHK(ctx, hipDeviceSynchronize());
  const size_t eb = (size_t)ctx->EB, M = (size_t)ctx->Mmax, d = (size_t)ctx->d, BT = (size_t)ctx->Bmax * ctx->Tmax;
  HIPCHK(ctx, hipMemset(ctx->H_op.p, byte, M * ctx->ff * eb));
  HIPCHK(ctx, hipMemset(ctx->QK_op.p, byte, M * 2 * d * eb));
  HIPCHK(ctx, hipMemset(ctx->A_op.p, byte, M * d * eb));
  HIPCHK(ctx, hipMemset(ctx->h1_op.p, byte, BT * d * eb));
  HIPCHK(ctx, hipDeviceSynchronize());
  return 0;
}

// ------------------------------------------------------------------------------------------------
// kernel-level test hooks
// ------------------------------------------------------------------------------------------------
struct TmpBufs {
  std::vector<void*> v;
  ~TmpBufs() {
    for (void* p : v) (void)hipFree(p);
  }
  void* get(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
    v.push_back(p);
    return p;
  }
};

template <class Op>
static int test_gemm_impl(int M, int N, int K, const float* a, const float* w, const float* bias, int act, float* c,
                          const float* gamma, const float2* stats_in, float2* stats_out, bool resid, hipStream_t st) {
  typedef typename Op::elem_t E;
  if (prepare_all<Op>() != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "prepare failed");
  const int Kp = round_up(K, 64);
  TmpBufs tb;
  E* ao = (E*)tb.get((size_t)M * Kp * Op::EB);
  E* wo = (E*)tb.get((size_t)N * Kp * Op::EB);
  E* yo = (E*)tb.get((size_t)M * N * Op::EB);
  if (!ao || !wo || !yo) return fail(nullptr, TAMF_ERR_NOMEM, "hipMalloc failed");
  hipLaunchKernelGGL((pack_operand_kernel<Op>), grid1d((long)M * (Kp / 8)), dim3(256), 0, st, a, ao, (long)M, K, Kp);
  hipLaunchKernelGGL((pack_operand_kernel<Op>), grid1d((long)N * (Kp / 8)), dim3(256), 0, st, w, wo, (long)N, K, Kp);
  GemmArgs<Op> ga{ao, Kp, wo, Kp, M, N, Kp, 0};
  hipError_t e;
  if (resid) {
    // the residual GEMM of an encoder sublayer with the LayerNorm of its input deferred (EpiResid): c holds u on entry, u_next on return
    EpiResid<Op> ep{bias, gamma, c, Op::PREC == 0 ? nullptr : yo, N, stats_out, ACT_NONE, {}, LnStats{stats_in, N / 32, 1.0f / (float)N, 1e-5f}};
    // (the selection of the step: launch_resid for clip-aligned M - small tiles with the deep K pipeline when there are few of them - and
    // for every other M the small tiles where they fit, so that ragged tile edges of that kernel are tested too, else 128 x 128)
    const int sp = clip_rows_of_m(M);
    e = sp ? launch_resid<Op>(ga, ep, M / sp, sp, st) : launch_rows<Op>(ga, ep, st);
  } else {
    EpiStoreF32 ep{bias, c, N, act};
    // M = n * 208 rows (T = 196) or n * 168 rows (T = 160): the clip-aligned tiles the encoder layers use (a ladder of this hook's
    // own - the step has no plain fp32 store; 32 clips or fewer: the row-part tiles)
    const int nc = M / 208;
    bool done = false;
    if (M % 208 == 0 && N % 256 == 0 && ClipLaunch<Op, 4, EpiStoreF32>::applies(nc, 208, N, Kp)) {
      e = ClipLaunch<Op, 4, EpiStoreF32>::launch(nullptr, ao, Kp, wo, Kp, nc, 208, N, Kp, ep, st);
      done = true;
    } else {
      const int sp = clip_rows_of_m(M);
      if (sp) {
        TAMF_CLIP_NSUB(sp, {
          if (ClipLaunch<Op, 2, EpiStoreF32, NSP, 2>::applies_parts(M / sp, sp, N, Kp)) {
            e = ClipLaunch<Op, 2, EpiStoreF32, NSP, 2>::launch(nullptr, ao, Kp, wo, Kp, M / sp, sp, N, Kp, ep, st);
            done = true;
          } else if (ClipLaunch<Op, 2, EpiStoreF32, NS>::applies(M / sp, sp, N, Kp)) {
            e = ClipLaunch<Op, 2, EpiStoreF32, NS>::launch(nullptr, ao, Kp, wo, Kp, M / sp, sp, N, Kp, ep, st);
            done = true;
          }
        })
      }
    }
    if (!done) e = gemm128<Op>(ga, ep, st);
  }
  if (e != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, std::string("gemm launch: ") + hipGetErrorString(e));
  if (hipStreamSynchronize(st) != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "sync failed");
  e = hipGetLastError();
  if (e != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, std::string("gemm run: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int tamf_test_gemm(int32_t precision, int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev,
                              const float* bias_dev, int32_t act, float* c_dev, void* stream) {
  TAMF_LAUNCH_LOCK;
  if (M <= 0 || N <= 0 || K <= 0 || N % 128) return fail(nullptr, TAMF_ERR_INVALID, "N must be a multiple of 128");
  hipStream_t st = (hipStream_t)stream;
  if (precision < 0 || precision > TAMF_PREC_F16X3) return fail(nullptr, TAMF_ERR_INVALID, "unknown precision");
  TAMF_WITH_OP(precision, return test_gemm_impl<Op>(M, N, K, a_dev, w_dev, bias_dev, act, c_dev, nullptr, nullptr, nullptr, false, st));
  return 0;
}

extern "C" int tamf_test_gemm_resid(int32_t precision, int32_t M, int32_t N, int32_t K, const float* a_dev, const float* w_dev,
                                    const float* bb_dev, const float* gamma_dev, const float* stats_in_dev, float* x_dev,
                                    float* stats_out_dev, void* stream) {
  TAMF_LAUNCH_LOCK;
  if (M <= 0 || K <= 0 || !(N == 128 || N == 256 || N == 512)) return fail(nullptr, TAMF_ERR_INVALID, "N must be 128/256/512");
  if (!a_dev || !w_dev || !bb_dev || !gamma_dev || !x_dev || !stats_out_dev) return fail(nullptr, TAMF_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  if (precision < 0 || precision > TAMF_PREC_F16X3) return fail(nullptr, TAMF_ERR_INVALID, "unknown precision");
  TAMF_WITH_OP(precision, return test_gemm_impl<Op>(M, N, K, a_dev, w_dev, bb_dev, 0, x_dev, gamma_dev, (const float2*)stats_in_dev,
                                                    (float2*)stats_out_dev, true, st));
  return 0;
}

template <class Op>
static int test_attn_impl(int B, int S, int H, int hd, const float* qkv, float* out, hipStream_t st) {
  typedef typename Op::elem_t E;
  const int d = H * hd, Sp = round_up(S, 8), Skp = round_up(S, 32);
  const long M = (long)B * Sp;
  TmpBufs tb;
  const size_t qk_n = (size_t)M * 2 * d, vt_n = (size_t)B * d * Skp, o_n = (size_t)M * d;
  E* qk = (E*)tb.get(qk_n * Op::EB);
  E* vt = (E*)tb.get(vt_n * Op::EB);
  E* oo = (E*)tb.get(o_n * Op::EB);
  float* of = (float*)tb.get(o_n * 4);
  if (!qk || !vt || !oo || !of) return fail(nullptr, TAMF_ERR_NOMEM, "hipMalloc failed");
  (void)hipMemsetAsync(vt, 0, vt_n * Op::EB, st);
  const float qscale = 1.4426950408889634f / sqrtf((float)hd);
  hipLaunchKernelGGL((qkv_pack_kernel<Op>), grid1d(M * 3 * d), dim3(256), 0, st, qkv, qk, vt, B, S, Sp, Skp, H, hd, qscale);
  AttnArgs<Op> aa{qk, vt, oo, S, Sp, Skp, d, H, 0};
  hipError_t e = launch_attn<Op>(aa, B, hd, st);
  if (e != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, std::string("attn launch: ") + hipGetErrorString(e));
  hipLaunchKernelGGL((unpack_operand_kernel<Op>), grid1d(M * d), dim3(256), 0, st, oo, of, M, d, d);
  // compact [B][Sp][d] -> [B][S][d]
  for (int b = 0; b < B; ++b)
    (void)hipMemcpyAsync(out + (size_t)b * S * d, of + (size_t)b * Sp * d, (size_t)S * d * 4, hipMemcpyDeviceToDevice, st);
  if (hipStreamSynchronize(st) != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "sync failed");
  e = hipGetLastError();
  if (e != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, std::string("attn run: ") + hipGetErrorString(e));
  return 0;
}

extern "C" int tamf_test_attention(int32_t precision, int32_t B, int32_t S, int32_t H, int32_t hd, const float* qkv_dev,
                                   float* out_dev, void* stream) {
  TAMF_LAUNCH_LOCK;
  if (B <= 0 || S <= 0 || H <= 0 || !(hd == 64 || hd == 128)) return fail(nullptr, TAMF_ERR_INVALID, "bad attention shape");
  hipStream_t st = (hipStream_t)stream;
  if (precision < 0 || precision > TAMF_PREC_F16X3) return fail(nullptr, TAMF_ERR_INVALID, "unknown precision");
  TAMF_WITH_OP(precision, return test_attn_impl<Op>(B, S, H, hd, qkv_dev, out_dev, st));
  return 0;
}

// random operand fill for the kernel benchmarks (values in [-1, 1))
template <class Op>
__global__ void fill_operand_kernel(typename Op::elem_t* out, long n, unsigned salt) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 8;
  if (i >= n) return;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    unsigned h = (unsigned)(i + j) * 2654435761u + salt;
    h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
    v[j] = (float)(h >> 8) * (2.0f / 16777216.0f) - 1.0f;
  }
  Op::template store<8>(out, i, v);
}

template <class Op>
static int bench_gemm_impl(int epi_kind, int M, int N, int K, int iters, float* ms_out, hipStream_t st) {
  typedef typename Op::elem_t E;
  if (prepare_all<Op>() != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "prepare failed");
  TmpBufs tb;
  const long an = (long)M * K, wn = (long)N * K, on = (long)M * N;
  E* a = (E*)tb.get((size_t)an * Op::EB);
  E* w = (E*)tb.get((size_t)wn * Op::EB);
  E* o = (E*)tb.get((size_t)on * Op::EB);
  E* o2 = (E*)tb.get((size_t)on * Op::EB);
  float* x = (float*)tb.get((size_t)on * 4);
  float* vec = (float*)tb.get((size_t)N * 4 * 4);
  if (!a || !w || !o || !o2 || !x || !vec) return fail(nullptr, TAMF_ERR_NOMEM, "hipMalloc failed");
  hipLaunchKernelGGL((fill_operand_kernel<Op>), grid1d(an / 8), dim3(256), 0, st, a, an, 1u);
  hipLaunchKernelGGL((fill_operand_kernel<Op>), grid1d(wn / 8), dim3(256), 0, st, w, wn, 2u);
  hipLaunchKernelGGL((fill_operand_kernel<OpF32>), grid1d(on / 8), dim3(256), 0, st, x, on, 3u);
  hipLaunchKernelGGL((fill_operand_kernel<OpF32>), grid1d(N * 4 / 8), dim3(256), 0, st, vec, (long)N * 4, 4u);
  GemmArgs<Op> ga{a, K, w, K, M, N, K, 0};
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "event");
  hipError_t e = hipSuccess;
  for (int it = -2; it < iters && e == hipSuccess; ++it) {
    if (it == 0) (void)hipEventRecord(e0, st);
    if (epi_kind == 2) {
      e = hipErrorInvalidValue;  // (rounds 2 - 5: the LayerNorm-fused 64 x d tile; gone - kind 12 is the residual GEMM now)
    } else if (epi_kind == 3) {
      EpiStoreF32 ep{vec, x, N, ACT_NONE};
      if (M % 208 == 0 && ClipLaunch<Op, 2, EpiStoreF32>::applies(M / 208, 208, N, K))
        e = ClipLaunch<Op, 2, EpiStoreF32>::launch(nullptr, a, K, w, K, M / 208, 208, N, K, ep, st);
      else
        e = gemm128<Op>(ga, ep, st);
    } else if (epi_kind == 1) {
      const int d = N / 3;
      EpiQKV<Op> ep{vec, o, o2, d, d / 128, 128, 208, 224, 0.1f};
      e = gemm128<Op>(ga, ep, st);
    } else if (epi_kind >= 10 && epi_kind <= 12) {
      // the deferred-LayerNorm forms: 10 = FFN1 with the row terms, 11 = QKV with the row terms, 12 = residual GEMM
      {
        const LnStats ln{(const float2*)x, K / 32, 1.0f / (float)K, 1e-5f};  // (any finite numbers: x is M x N >= M x K / 16 floats)
        if (epi_kind == 10) {
          EpiBiasAct<Op, true> ep{vec, nullptr, 0, o, N, ACT_GELU, {}, ln};
          e = clip_rows_of_m(M) == 208 ? launch_ffn1<Op>(ga, ep, M / 208, 208, st) : gemm128<Op>(ga, ep, st);
        } else if (epi_kind == 11) {
          const int d = N / 3;
          EpiQKV<Op, true> ep{vec, o, o2, d, d / 128, 128, 208, 224, 0.1f, {}, ln};
          e = gemm128<Op>(ga, ep, st);
        } else {
          EpiResid<Op> ep{vec, vec + N, x, o, N, (float2*)o2, ACT_NONE, {}, LnStats{nullptr, N / 32, 1.0f / (float)N, 1e-5f}};
          e = clip_rows_of_m(M) == 208 ? launch_resid<Op>(ga, ep, M / 208, 208, st) : gemm128<Op>(ga, ep, st);
        }
      }
    } else {
      EpiBiasAct<Op> ep{vec, nullptr, 0, o, N, ACT_GELU};
      if (M % 208 == 0 && ClipLaunch<Op, 4, EpiBiasAct<Op>>::applies(M / 208, 208, N, K)) {
        e = ClipLaunch<Op, 4, EpiBiasAct<Op>>::launch(nullptr, a, K, w, K, M / 208, 208, N, K, ep, st);  // (ablations: ClipGemmArgs::abl)
      } else {
        if (g_krot >= 0 && (g_krot & 0x20000)) ep.ldo = 0;  // ablation: every row stores to the same (L2-resident) row - no HBM writes
        if (g_krot >= 0 && (g_krot & 0x8000)) ep.act = ACT_NONE;  // ablation: no GELU
        e = gemm128<Op>(ga, ep, st);
      }
    }
  }
  (void)hipEventRecord(e1, st);
  hipError_t se = hipStreamSynchronize(st);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess || se != hipSuccess)
    return fail(nullptr, TAMF_ERR_HIP, std::string("bench gemm: ") + hipGetErrorString(e != hipSuccess ? e : se));
  *ms_out = ms / iters;
  return 0;
}

// attention alone on random operands resident in HBM (tools/attn_bench.py): average ms of `iters` launches
template <class Op>
static int bench_attn_impl(int B, int S, int H, int hd, int iters, int abl, float* ms_out, hipStream_t st) {
  typedef typename Op::elem_t E;
  if (prepare_all<Op>() != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "prepare failed");
  const int d = H * hd, Sp = round_up(S, 8), Skp = round_up(S, 32);
  const long M = (long)B * Sp, qk_n = M * 2 * d, vt_n = (long)B * d * Skp, o_n = M * d;
  TmpBufs tb;
  E* qk = (E*)tb.get((size_t)qk_n * Op::EB);
  E* vt = (E*)tb.get((size_t)vt_n * Op::EB);
  E* oo = (E*)tb.get((size_t)o_n * Op::EB);
  if (!qk || !vt || !oo) return fail(nullptr, TAMF_ERR_NOMEM, "hipMalloc failed");
  hipLaunchKernelGGL((fill_operand_kernel<Op>), grid1d(qk_n / 8), dim3(256), 0, st, qk, qk_n, 5u);
  hipLaunchKernelGGL((fill_operand_kernel<Op>), grid1d(vt_n / 8), dim3(256), 0, st, vt, vt_n, 6u);
  AttnArgs<Op> aa{qk, vt, oo, S, Sp, Skp, d, H, abl};
  hipEvent_t e0, e1;
  if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "event");
  hipError_t e = hipSuccess;
  for (int it = -2; it < iters && e == hipSuccess; ++it) {
    if (it == 0) (void)hipEventRecord(e0, st);
    e = launch_attn<Op>(aa, B, hd, st);
  }
  (void)hipEventRecord(e1, st);
  hipError_t se = hipStreamSynchronize(st);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, e0, e1);
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  if (e != hipSuccess || se != hipSuccess)
    return fail(nullptr, TAMF_ERR_HIP, std::string("bench attention: ") + hipGetErrorString(e != hipSuccess ? e : se));
  *ms_out = ms / iters;
  return 0;
}

extern "C" int tamf_bench_attention(int32_t precision, int32_t B, int32_t S, int32_t H, int32_t hd, int32_t iters, int32_t abl,
                                    int32_t tuning, float* ms_out, void* stream) {
  TAMF_LAUNCH_LOCK;
  if (B <= 0 || S <= 0 || H <= 0 || !(hd == 64 || hd == 128) || iters <= 0 || !ms_out) return fail(nullptr, TAMF_ERR_INVALID, "bad argument");
  if (precision < 0 || precision > TAMF_PREC_F16X3) return fail(nullptr, TAMF_ERR_INVALID, "unknown precision");
  const int saved_rot = g_krot, saved_sel = g_sel;
  tamf_set_gemm_tuning(tuning);
  int rc = 0;
  TAMF_WITH_OP(precision, rc = bench_attn_impl<Op>(B, S, H, hd, iters, abl, ms_out, (hipStream_t)stream));
  g_krot = saved_rot;
  g_sel = saved_sel;
  return rc;
}

extern "C" int tamf_bench_mfma_rate(int32_t precision, int32_t millis, float* tflops_out, float* mhz_out, void* stream) {
  if (precision < 0 || precision > TAMF_PREC_F16X3 || millis <= 0 || millis > 20000 || !tflops_out) return fail(nullptr, TAMF_ERR_INVALID, "bad argument");
  hipStream_t st = (hipStream_t)stream;
  float* sink = nullptr;
  int cus = 0, dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
    return fail(nullptr, TAMF_ERR_HIP, "no device");
  const int grid = 2 * cus, block = 512, iters = 4000;  // 2 workgroups x 8 waves per CU = 4 waves per SIMD; about 1 ms per launch
  if (hipMalloc(&sink, (size_t)grid * block * sizeof(float)) != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, "hipMalloc failed");
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  auto launch = [&]() {
    if (precision == TAMF_PREC_F32) hipLaunchKernelGGL(mfma_rate_kernel<0>, dim3(grid), dim3(block), 0, st, sink, iters);
    else if (precision == TAMF_PREC_F16X3) hipLaunchKernelGGL(mfma_rate_kernel<2>, dim3(grid), dim3(block), 0, st, sink, iters);
    else hipLaunchKernelGGL(mfma_rate_kernel<1>, dim3(grid), dim3(block), 0, st, sink, iters);
  };
  // the first third of the time lets the power management settle, the rest is timed
  float ms1 = 0.f, ms = 0.f;
  launch();
  hipEventRecord(e0, st);
  launch();
  hipEventRecord(e1, st);
  hipEventSynchronize(e1);
  hipEventElapsedTime(&ms1, e0, e1);
  const int n_all = (int)(millis / (ms1 > 1e-3f ? ms1 : 1e-3f)) + 3, n_settle = n_all / 3, n = n_all - n_settle;
  for (int i = 0; i < n_settle; ++i) launch();
  hipEventRecord(e0, st);
  for (int i = 0; i < n; ++i) launch();
  hipEventRecord(e1, st);
  hipError_t e = hipEventSynchronize(e1);
  hipEventElapsedTime(&ms, e0, e1);
  hipEventDestroy(e0);
  hipEventDestroy(e1);
  hipFree(sink);
  if (e != hipSuccess || !(ms > 0.f)) return fail(nullptr, TAMF_ERR_HIP, e != hipSuccess ? hipGetErrorString(e) : "no time measured");
  const double mfmas = (double)n * grid * (block / 64) * (double)iters * 8;
  const double flop_per_mfma = precision == TAMF_PREC_F32 ? 2.0 * 16 * 16 * 4 : 2.0 * 16 * 16 * 32;
  *tflops_out = (float)(mfmas * flop_per_mfma / (ms * 1e-3) / 1e12);
  // the clock this rate implies if the pipe issued one MFMA per 16 cycles (32 for the fp32 shape: 8 passes of 4 cycles): a LOWER bound of sclk
  if (mhz_out) *mhz_out = (float)(mfmas / (cus * 4.0) * (precision == TAMF_PREC_F32 ? 32.0 : 16.0) / (ms * 1e-3) / 1e6);
  return 0;
}

extern "C" int tamf_bench_gemm(int32_t precision, int32_t epi_kind, int32_t krot, int32_t M, int32_t N, int32_t K,
                               int32_t iters, float* ms_out, void* stream) {
  TAMF_LAUNCH_LOCK;
  if (M <= 0 || N <= 0 || K <= 0 || iters <= 0 || !ms_out) return fail(nullptr, TAMF_ERR_INVALID, "bad argument");
  if (epi_kind == 1 && (N % 384 || M % 208)) return fail(nullptr, TAMF_ERR_INVALID, "qkv bench needs N = 3d, M multiple of 208");
  const int saved_rot = g_krot, saved_sel = g_sel;
  tamf_set_gemm_tuning(krot);  // -1 = per-kernel defaults; >= 0 = GemmArgs::krot bits (tamf_gemm.h) + selection overrides
  hipStream_t st = (hipStream_t)stream;
  int rc = 0;
  if (precision < 0 || precision > TAMF_PREC_F16X3) rc = fail(nullptr, TAMF_ERR_INVALID, "unknown precision");
  else TAMF_WITH_OP(precision, rc = bench_gemm_impl<Op>(epi_kind, M, N, K, iters, ms_out, st));
  g_krot = saved_rot;
  g_sel = saved_sel;
  return rc;
}

extern "C" int tamf_set_gemm_tuning(int32_t krot) {
  TAMF_LAUNCH_LOCK;
  // low 20 bits: GemmArgs::krot bits (all ones = keep the per-kernel defaults); bits 20..30: kernel-selection overrides (g_sel).
  // The words are process-global and a captured loop graph has the selection of its capture time baked in, so every live
  // context's graph is retired here: the next tamf_sample_loop re-captures with the new selection (same as tamf_denoise).
  // (selection bit 2048 - the row-block kernels - has no room above bit 30: it is "low 20 bits = 0x7FFFF", i.e. all ones but bit 19)
  int sel = krot >= 0 ? (krot >> 20) & 0x7FF : 0;
  const int low = krot & 0xFFFFF;
  int rot = -1;
  if (krot >= 0 && low == 0x7FFFF) sel |= 2048;
  else if (krot >= 0 && low != 0xFFFFF) rot = low;
  if (sel != g_sel || rot != g_krot) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    for (tamf_ctx* c : g_live_ctx) (void)retire_graph(c);
  }
  g_sel = sel;
  g_krot = rot;
  return 0;
}

extern "C" int tamf_test_philox(uint64_t seed, int64_t clip_id_base, int32_t draw, int32_t B, int32_t n_feat, int32_t T,
                                float* out_dev, void* stream) {
  if (B <= 0 || n_feat <= 0 || T <= 0 || !out_dev) return fail(nullptr, TAMF_ERR_INVALID, "bad argument");
  hipLaunchKernelGGL(philox_fill_kernel, grid1d((long)B * n_feat * T), dim3(256), 0, (hipStream_t)stream, out_dev,
                     (unsigned long long)seed, (long long)clip_id_base, (unsigned)draw, B, n_feat, T);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(nullptr, TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

#ifdef TAMF_TIMELINE
// debug builds only (not part of include/tamf_hip.h): which = 0 GEMM (5 u64 per workgroup), 1 attention (4 u64)
extern "C" int tamf_debug_timeline(int which, void* dst, size_t bytes) {
  if (which == 0) return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_gemm_ts), bytes, 0, hipMemcpyDeviceToHost);
  if (which == 2) return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_clip_ts), bytes, 0, hipMemcpyDeviceToHost);
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_attn_ts), bytes, 0, hipMemcpyDeviceToHost);
}
#endif
