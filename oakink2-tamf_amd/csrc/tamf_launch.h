// Which kernel runs a GEMM or attention launch of a given shape, with what grid / block / LDS size: the selection words, the launcher
// of every kernel family, one selection function per GEMM role of the denoiser step, the attention launch, and prepare_all.  Host
// code; tamf_hip.hip includes it after the kernel headers.  Nothing here knows tamf_ctx: operands, epilogues and shapes come in.
// The shape arithmetic the decisions rest on (clip_tile_rows, vt_row_keys, scratch_layout, ...) is HIP-free and lives in tamf_shapes.h.
#pragma once
#include "tamf_shapes.h"
// ------------------------------------------------------------------------------------------------
// kernel launchers
// ------------------------------------------------------------------------------------------------
// GemmArgs::krot bits (tamf_gemm.h): L2 touch-prefetch distance, XCD arrangement.  -1 = per-kernel default: the 64-row
// LayerNorm tiles prefetch 4 K tiles ahead into L2 (their weight panel is shared by every workgroup and has been evicted
// from the 4 MB L2 by the other GEMMs of the layer: 186 -> 153 us in situ), the 128 x 128 tiles do not (it costs them
// 5-8 %).  Only the kernel benchmark hook (tamf_bench_gemm) overrides it.
static int g_krot = -1;
// kernel-selection overrides for A/B measurements (tamf_set_gemm_tuning bits 20..): 1 = no clip tiles at all,
// 2 = FFN2 / out-proj on the 128 x 128 tiles, 4 = attention split once more, 8 = FFN1 on the 128 x 128 tiles,
// 16 = residual GEMMs of a few clips on the clip / 128 x 128 tiles too (no 32- / 64-row tiles), 64 = f32: QKV on the 128 x 128 tiles,
// 32 = FFN1 (whole-clip tiles in two or more exact rounds): column-split rounds (off without the bit: they cut FFN1's fetch
//      by 6.6 % and make the step 0.6 % (f16x3) / 2.3 % (bf16) slower),
// 512 = streaming attention kernel in the 16-bit modes too,
// 1024 = clip tiles from 50 % (not 74 %) of the workgroup slots of their rounds.
// (Rounds 2 - 5 also had 16 (another meaning) / 256 / 2048 / 4096: the LayerNorm-fused 64 x d tile, the GEMM + LayerNorm-kernel form and the row-block kernel
// of the residual GEMMs - gone with the deferred LayerNorm, which every mode uses now; 32 / 128: clip-tile variants of FFN1 / QKV that
// lost their A/B; 256 (another meaning): the overlap probe of round 6, measured and removed - DESIGN.md section 6.  The bits are accepted and ignored.)
static int g_sel = 0;
static inline int krot_for(bool ln_tile) { return g_krot >= 0 ? g_krot : (ln_tile ? (4 << 8) : 0); }

// resident workgroup slots of the chip for the 2-per-CU tiles (MI355X: 256 CUs); one "round" of a launch.  Per DEVICE (one
// process-wide word followed the device of the context created last): written by tamf_ctx_create under the launch lock, read for the
// calling thread's current device - every entry point that enqueues kernels has made its context's device current.
static std::atomic<int> g_wg_slots_dev[64];
static inline int wg_slots() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  const int v = g_wg_slots_dev[dev & 63].load(std::memory_order_relaxed);
  return v > 0 ? v : 512;
}

// Raise the dynamic-LDS ceiling of `Kernel` to `bytes`, once per device: kernel attributes are per device, and so are the flags -
// one set per kernel instantiation.  Every launcher's prepare() is this, so a launch prepares its own kernel when nobody has.
template <auto Kernel>
static hipError_t lds_once(int bytes) {
  static std::atomic<bool> done[64];  // (zero-initialised; relaxed: the attribute calls are idempotent)
  int dev = 0;
  (void)hipGetDevice(&dev);
  if (dev >= 0 && dev < 64 && done[dev].load(std::memory_order_acquire)) return hipSuccess;
  hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (e == hipSuccess && dev >= 0 && dev < 64) done[dev].store(true, std::memory_order_release);
  return e;
}

template <class Op, int BM, int BN, class Epi, bool CAN_SPLIT = false>
struct GemmLaunch {
  static constexpr int SMEM = GemmSmem<BM, BN>::TOTAL;
  // wave grid: the 64-row LayerNorm tiles own a CU and run 8 waves (2 x 4), the 64 x 512 one 16 waves (2 x 8: four waves
  // per SIMD cover each other's LDS / barrier latency, 36.6 -> 35.1 us for out-proj); the 128 x 128 tiles run 8 waves
  // (4 x 2) with two workgroups per CU
  // waves along M of the 128 x 128 tiles: 4 = 8 waves per workgroup (4 x 2), two workgroups per CU = 4 waves per SIMD.
  // Round 3, two builds alternating on one box: QKV 62.8 -> 60.7 us (f16x3), 31.5 -> 29.6 us (bf16) against the 2 x 2
  // grid of rounds 1 - 2; the whole step -1 %: a workgroup left alone on its CU during its partner's epilogue keeps 2 waves per SIMD
  static constexpr int WGN = (BM <= 64) ? (BN == 512 ? 8 : 4) : 2;
  static constexpr int WGM = (BM <= 64 || Op::PREC == 0) ? 2 : 4;  // (f32: the 2 x 2 grid stays - input_merge.2 78 us against 91 us with 4 x 2)
  static hipError_t prepare() {
    hipError_t e = lds_once<gemm_kernel<Op, BM, BN, WGM, WGN, Epi, 1>>(SMEM);
    if constexpr (CAN_SPLIT) {
      if (e == hipSuccess) e = lds_once<gemm_kernel<Op, BM, BN, WGM, WGN, Epi, 2>>(SMEM);
      if (e == hipSuccess) e = lds_once<gemm_kernel<Op, BM, BN, WGM, WGN, Epi, 4>>(SMEM);
    }
    return e;
  }
  static hipError_t launch(const GemmArgs<Op>& ga, const Epi& epi, hipStream_t st) {
    hipError_t e = prepare();
    if (e != hipSuccess) return e;
    if ((ga.K * Op::EB) % GEMM_BKB != 0 || ga.N % BN != 0 || ga.M <= 0) return hipErrorInvalidValue;
    const int ntn = ga.N / BN, ntm = (ga.M + BM - 1) / BM, tiles = ntn * ntm;
    GemmArgs<Op> gb = ga;
    gb.krot = krot_for(BM <= 64 && BN >= 256);
    // wide-N launches (FFN1: 16 column tiles): XCDs in a 4 x 2 arrangement over the tile grid - each L2 then serves half of W
    // instead of all of it (FETCH_SIZE 162 -> 137 MB per launch, time unchanged); with few column tiles it would re-read A
    if (g_krot < 0 && BM == 128 && ntn >= 8) gb.krot |= 0x10000;  // (also picked up by the persistent grid below: QKV, round 4)
    gb.n_full = tiles;
    int split = 1;
    if constexpr (CAN_SPLIT) {
      // tiles left over after the last full round: cut them 2- or 4-ways while every slice still gets a CU to itself
      // (measured: slices sharing a CU take as long as the whole tiles did, FFN1 93.5 -> 89 us with 2 x 128 slices)
      // (a launch of less than one round is sliced as long as the slices fit the workgroup slots: two slices sharing a CU
      // overlap each other's latencies, one whole tile alone on a CU does not)
      const int n_full = (tiles / wg_slots()) * wg_slots(), rem = tiles - n_full, cus = n_full ? wg_slots() / 2 : wg_slots();
      if (rem > 0) {
        split = (rem * 4 <= cus) ? 4 : (rem * 2 <= cus) ? 2 : 1;
        if (split > 1) gb.n_full = n_full;
      }
    }
    gb.n_tiles = 0;
    int nblk = gb.n_full + (tiles - gb.n_full) * split;
    // more than one round, a partial last round and no slices: a persistent one-round grid balances the CUs (the hardware
    // hands a freed slot to the next workgroup greedily; QKV's 1248 tiles ended up as 4..6 per CU instead of 4..5)
    if (split == 1 && BM == 128 && tiles > wg_slots() && tiles % wg_slots() != 0) {
      gb.n_tiles = tiles;
      nblk = wg_slots();
    }
    const dim3 grid(nblk), block(WGM * WGN * 64);
    if constexpr (CAN_SPLIT) {
      if (split == 4) { hipLaunchKernelGGL((gemm_kernel<Op, BM, BN, WGM, WGN, Epi, 4>), grid, block, SMEM, st, gb, epi); return hipGetLastError(); }
      if (split == 2) { hipLaunchKernelGGL((gemm_kernel<Op, BM, BN, WGM, WGN, Epi, 2>), grid, block, SMEM, st, gb, epi); return hipGetLastError(); }
    }
    hipLaunchKernelGGL((gemm_kernel<Op, BM, BN, WGM, WGN, Epi, 1>), grid, block, SMEM, st, gb, epi);
    return hipGetLastError();
  }
};
// the wide-N GEMMs (QKV, FFN1, input merge) may split their left-over tiles
template <class Epi> struct EpiCanSplit { static constexpr bool value = false; };
template <class Op, bool LN> struct EpiCanSplit<EpiBiasAct<Op, LN>> { static constexpr bool value = true; };
template <class Op, bool LN> struct EpiCanSplit<EpiQKV<Op, LN>> { static constexpr bool value = true; };
template <> struct EpiCanSplit<EpiStoreF32> { static constexpr bool value = true; };

// Small tiles with a deep K pipeline (tamf_gemm_deep.h): launches of a few tiles, one workgroup each
template <class Op, int BM, int BN, int NSTG, class Epi, int WGM = 2, int WGN = 4>
struct GemmDeepLaunch {
  static constexpr int SMEM = GemmSmemDeep<BM, BN, NSTG>::TOTAL;
  static hipError_t prepare() { return lds_once<gemm_deep_kernel<Op, BM, BN, WGM, WGN, NSTG, Epi>>(SMEM); }
  static hipError_t launch(const GemmArgs<Op>& ga, const Epi& epi, hipStream_t st) {
    hipError_t e = prepare();
    if (e != hipSuccess) return e;
    if ((ga.K * Op::EB) % GEMM_BKB != 0 || ga.N % BN != 0 || ga.M <= 0) return hipErrorInvalidValue;
    const int tiles = (ga.N / BN) * ((ga.M + BM - 1) / BM);
    hipLaunchKernelGGL((gemm_deep_kernel<Op, BM, BN, WGM, WGN, NSTG, Epi>), dim3(tiles), dim3(WGM * WGN * 64), SMEM, st, ga, epi);
    return hipGetLastError();
  }
};

// A few clips per call (one, in the reference's own launcher: launch/sample.py:202-229): the tiles of the big batches would put a handful of
// workgroups on the chip and each would walk its K tiles one L2 round trip at a time.  32 x 128 tiles (64 x 128 while they still fit one
// workgroup per CU) with a four-stage K pipeline instead: a CU on every 32 rows, the same K order per element - the same bits.
// Returns false when the launch is not that small (or selection bit 1 / 16 turns the small tiles off: the A/B partner).
template <class Op, class Epi>
static bool small_m_launch(const GemmArgs<Op>& ga, const Epi& ep, hipStream_t st, hipError_t* e) {
  if ((g_sel & (1 | 16)) || ga.N % 128 != 0) return false;
  const int cus = wg_slots() / 2, ntn = ga.N / 128;
  if (((ga.M + 31) / 32) * ntn <= cus) {
    *e = GemmDeepLaunch<Op, 32, 128, 4, Epi>::launch(ga, ep, st);
    return true;
  }
  if (((ga.M + 63) / 64) * ntn <= cus) {
    *e = GemmDeepLaunch<Op, 64, 128, 4, Epi>::launch(ga, ep, st);
    return true;
  }
  return false;
}

// Clip-aligned tiles (tamf_gemm_clip.h): one M tile = one clip of NSUB MFMA row tiles.  NSUB = 13 serves the bench shape (T = 196:
// S = 201, Sp = 208), NSUB = 11 the length the reference's dataset emits (slice_max_len = 160, dataset/interaction_segment.py:291:
// S = 165, Sp = 168 - the 11th row tile holds 8 rows, the rest of it is clamped on the load side and skipped on the store side);
// a clip that is up to one row tile shorter than the template runs on it with that tile wasted.  Used when K gives an even number
// of K tiles and the tile count fills the chip's rounds well enough; everything else runs on the 128 x 128 tiles.
// row tiles of the X waves (the K tile's loaders): they carry the DMA issue, so they get fewer of the row tiles - 6 of 13 / 5 of 11
// at 256 columns (5 : 8 spills the Y waves), 2 at 128 columns (a loader wave is blocked ~850 of the ~1 900 cycles of a 128-column
// interval while its pieces queue; FFN2 at B = 64: 73.7 us with 4 : 9, 69.5 us with 2 : 11)
template <int NI, int NSUB, int PARTS, int PREC>
struct ClipXsub {
  static constexpr int XSUB_N2 = 2;
  static constexpr int XSUB_N4 = 6;  // X row tiles of a 13-row-tile clip at 256 columns; an 11-row-tile clip gets one less
  static constexpr int XSUB_PARTS = 2;  // X : Y row tiles of the 7- / 6-row-tile parts (FFN2 at B = 32: 2 : 5 46 us, 3 : 4 60 us, 4 : 3 slower still)
  // f32 at 256 columns: row tiles of the Y waves (6: they read the next K tile's fragments inside their MFMA stream,
  // clip_mma_read_y, which does not fit the registers with 7; in f32 nothing of X overlaps Y's MFMAs, so the split is free)
  static constexpr int YSUB_F32_N4 = 6;
  static constexpr int value = PARTS > 1 ? XSUB_PARTS
                               : NI >= 4 ? (PREC == 0 ? NSUB - YSUB_F32_N4 : XSUB_N4 - (13 - NSUB + 1) / 2)
                                         : XSUB_N2;
};
// NSUB: row tiles of a TILE.  PARTS = 1: the tile is a whole clip; PARTS = 2: every clip is cut into its first NSUB row tiles and
// the rest (NSUB or NSUB - 1 of them), each a tile of its own - for launches whose whole-clip tiles would fill at most half of the CUs
template <class Op, int NI, class Epi, int NSUB = 13, int PARTS = 1>
struct ClipLaunch {
  static constexpr int XSUB = ClipXsub<NI, NSUB, PARTS, Op::PREC>::value;
  typedef ClipCfg<NSUB, NI, XSUB, Epi::LANE_CHUNK> C;
  static constexpr int CLIP_ROWS_MAX = PARTS * C::MT;  // padded rows of the longest clip these tiles hold
  static hipError_t prepare() { return lds_once<clip_gemm_kernel<Op, NSUB, NI, XSUB, Epi>>(C::BYTES); }
  static bool shape_ok(int Sp, int N, int K) {
    if (g_sel & 1) return false;  // kernel benchmark hook: force the 128 x 128 tiles (A/B runs)
    if (PARTS == 1 ? (Sp > C::MT || Sp <= C::MT - 32) : (Sp > 2 * C::MT || Sp <= 2 * C::MT - 32)) return false;
    if (N % C::BN != 0 || (K * Op::EB) % GEMM_BKB != 0) return false;
    const int KT = (K * Op::EB) / GEMM_BKB;
    return KT >= 2 && !(KT & 1);
  }
  static bool applies(int n_clips, int Sp, int N, int K, int min_util = 74) {
    static_assert(PARTS == 1, "whole-clip tiles");
    if (!shape_ok(Sp, N, K)) return false;
    const int cus = wg_slots() / 2, tiles = n_clips * (N / C::BN), rounds = (tiles + cus - 1) / cus;
    return tiles * 100 >= rounds * cus * ((g_sel & 1024) ? 50 : min_util);  // >= 74 % of the workgroup slots of its rounds are used (A/B: 50 %)
  }
  static hipError_t launch(const Op*, const typename Op::elem_t* A, int lda, const typename Op::elem_t* W, int ldw, int n_clips,
                           int Sp, int N, int K, const Epi& epi, hipStream_t st) {
    if (!shape_ok(Sp, N, K)) return hipErrorInvalidValue;  // (the kernel relies on it: fewer than 32 padding rows per tile, clip_issue)
    hipError_t e = prepare();
    if (e != hipSuccess) return e;
    static_assert(PARTS == 1 || PARTS == 2, "whole clips or their two row parts");
    constexpr int split_rows = PARTS == 1 ? 0 : NSUB * 16;
    ClipGemmArgs<Op> ga{A, lda, W, ldw, n_clips, Sp, N, K, PARTS * n_clips * (N / C::BN), split_rows, 0,
                        g_krot >= 0 ? ((g_krot >> 12) & 15) | (((g_krot >> 17) & 3) << 4) : 0};
    const int cus = wg_slots() / 2;
    {  // column-split rounds (tamf_gemm_clip.h, ClipGemmArgs::colsplit): whole clips, two or more EXACT rounds, column tiles divisible
      const int ntn = N / C::BN, rounds = ga.n_tiles / cus;
      const bool fits = PARTS == 1 && ga.n_tiles > cus && ga.n_tiles % cus == 0 && ntn % rounds == 0 && NI == 4;
      if (fits && (g_sel & 32)) ga.colsplit = ntn;
    }
    hipLaunchKernelGGL((clip_gemm_kernel<Op, NSUB, NI, XSUB, Epi>), dim3(ga.n_tiles < cus ? ga.n_tiles : cus), dim3(512), C::BYTES, st, ga, epi);
    return hipGetLastError();
  }
  // row-part tiles: when whole-clip tiles would use at most half of the CUs and the parts fit one round
  static bool applies_parts(int n_clips, int Sp, int N, int K) {
    static_assert(PARTS == 2, "row-part tiles");
    if (!shape_ok(Sp, N, K) || Sp <= C::MT) return false;
    const int cus = wg_slots() / 2, whole = n_clips * (N / C::BN);
    return whole * 2 <= cus;
  }
};
// Bind NS (whole-clip row tiles: 13 or 11) and NSP (row tiles of the first of two row parts: 7 or 6) for a clip of Sp padded rows
// and run the statement(s) that follow Sp_ (variadic: template argument lists carry commas); nothing runs for other clip lengths
#define TAMF_CLIP_NSUB(Sp_, ...)                                                                                  \
  if (clip_tile_rows(Sp_) == 13 * 16) { constexpr int NS = 13, NSP = 7; (void)NSP; (void)NS; __VA_ARGS__; }      \
  else if (clip_tile_rows(Sp_) == 11 * 16) { constexpr int NS = 11, NSP = 6; (void)NSP; (void)NS; __VA_ARGS__; }

// 128 x 128 tiles, or 64 x 128 tiles (8 waves) for the short-K launches that fill at most half of the workgroup slots (the
// input-merge GEMMs at <= 32 clips: 20.7 against 23.4 us at B = 32).  Measured and left on the big tiles: QKV (624 tiles at
// B = 32: 43 against 37 us) and FFN2 (K = 2048: 58 against 56 us).
template <class Epi> struct EpiHasSmallTile { static constexpr bool value = false; };
template <class Op> struct EpiHasSmallTile<EpiBiasAct<Op>> { static constexpr bool value = true; };
template <class Op> struct EpiHasSmallTile<EpiSeqRows<Op>> { static constexpr bool value = true; };
template <class Op, class Epi>
static hipError_t gemm128(const GemmArgs<Op>& ga, const Epi& epi, hipStream_t st) {
  if constexpr (EpiHasSmallTile<Epi>::value) {
    const int t128 = ((ga.M + 127) / 128) * (ga.N / 128);
    if (!(g_sel & 1) && ga.N % 128 == 0 && t128 * 2 <= wg_slots() && ga.K * Op::EB <= 2048)
      return GemmLaunch<Op, 64, 128, Epi>::launch(ga, epi, st);
  }
  return GemmLaunch<Op, 128, 128, Epi, EpiCanSplit<Epi>::value>::launch(ga, epi, st);
}

// ---- the denoiser step: one selection function per GEMM role ----
// residual GEMM of the deferred-LayerNorm form (out-proj, FFN2; 16-bit modes): the clip's row parts where whole clips would fill at
// most half of the CUs, whole-clip tiles where they fill at least half of their rounds' slots, 128 x 128 tiles for every other shape -
// the same K order per element and the same statistics trees in all three, i.e. the same bits
template <class Op>
static hipError_t launch_resid(const GemmArgs<Op>& ga, const EpiResid<Op>& ep, int B, int Sp, hipStream_t st) {
  // a few clips per call: whole-clip or row-part tiles would put 2 N / 128 workgroups on a clip - FFN2 of ONE clip ran 34 us (f32: 100 us)
  // on 8 CUs, 40 - 55 % of the step (profiles/r05/small_batch_resid_c25.txt, ..._c27.txt)
  // one to ~ 6 clips: 32 x 64 tiles (4 waves, six stages) while they fit one workgroup per CU - half the L2 -> LDS fill per workgroup and K
  // interval of the 32 x 128 tile, which is what a one-clip FFN2 was left bound by: 19.1 -> 14.2 us (f16x3), 10.3 -> 7.3 (bf16), 46.9 -> 25.5
  // (f32); the step of one clip 434 -> 385 / 256 -> 226 / 900 -> 686 us (profiles/r05/small_batch_32x64_c37.txt; same bits)
  if (!(g_sel & (1 | 16)) && ga.N % 64 == 0 && ((ga.M + 31) / 32) * (ga.N / 64) <= wg_slots() / 2)
    return GemmDeepLaunch<Op, 32, 64, 6, EpiResid<Op>, 2, 2>::launch(ga, ep, st);
  {
    hipError_t e = hipSuccess;
    if (small_m_launch<Op>(ga, ep, st, &e)) return e;
  }
  // Between "a few clips" and the whole-clip tiles (20 - 39 clips): 64 x 128 tiles with THREE stages - 72 KB, two workgroups per CU - while
  // they fit the workgroup slots.  bf16, whose K tiles are the shortest: 0.815 against 0.850 ms per step at 32 clips on the row-part tiles
  // (-4 %; profiles/r05/mid_batch_resid_c33.txt, variants alternating); the split modes gain up to ~ 1.25 tiles per CU only (24 clips:
  // -3 %; 32 clips: 1.510 against 1.510), f32 loses (MFMA-bound: the row parts multiply with fewer staged bytes per flop).  At 64 clips
  // the whole-clip tiles win by a wide margin (b64_resid_deep_c34.txt).  Same K order per element: the same bits.
  if (!(g_sel & (1 | 16)) && Op::PREC != 0 && ga.N % 128 == 0) {
    const int t64 = ((ga.M + 63) / 64) * (ga.N / 128);
    if (Op::SPLIT ? t64 * 4 <= wg_slots() / 2 * 5 : t64 <= wg_slots()) return GemmDeepLaunch<Op, 64, 128, 3, EpiResid<Op>>::launch(ga, ep, st);
  }
  if (!(g_sel & 2)) {
    TAMF_CLIP_NSUB(Sp, {
      if (ClipLaunch<Op, 2, EpiResid<Op>, NSP, 2>::applies_parts(B, Sp, ga.N, ga.K))
        return ClipLaunch<Op, 2, EpiResid<Op>, NSP, 2>::launch(nullptr, ga.A, ga.lda, ga.W, ga.ldw, B, Sp, ga.N, ga.K, ep, st);
      if (ClipLaunch<Op, 2, EpiResid<Op>, NS>::applies(B, Sp, ga.N, ga.K, 50))
        return ClipLaunch<Op, 2, EpiResid<Op>, NS>::launch(nullptr, ga.A, ga.lda, ga.W, ga.ldw, B, Sp, ga.N, ga.K, ep, st);
    })
  }
  return gemm128<Op>(ga, ep, st);
}

// every other GEMM: the small tiles where they fit (a few clips per call), else the 128 x 128 tiles (gemm128) - or, for the head,
// N = 128 is a single column tile: 64-row tiles (8 waves) double the workgroups that share the Philox-heavy epilogue
template <class Op, class Epi>
static hipError_t launch_rows(const GemmArgs<Op>& ga, const Epi& ep, hipStream_t st) {
  hipError_t e = hipSuccess;
  if (small_m_launch<Op>(ga, ep, st, &e)) return e;
  if constexpr (std::is_same<Epi, EpiHead<Op>>::value) return GemmLaunch<Op, 64, 128, Epi>::launch(ga, ep, st);
  else return gemm128<Op>(ga, ep, st);
}

// QKV projection of B clips of Sp padded rows (ga: N = 3 d columns of in_proj).  f32 with 128-wide heads: the Q | K columns and the
// V columns as two clip launches (EpiQK, EpiVt: the fields of `ep`; off with selection bit 64); every other shape as one launch on the
// rows ladder.  `launched(name, columns)` is called behind every launch - the step profile records an event there.
template <class Op, class Launched>
static hipError_t launch_qkv(const GemmArgs<Op>& ga, const EpiQKV<Op, true>& ep, int B, int Sp, hipStream_t st, Launched&& launched) {
  const int d = ep.d;
  if constexpr (Op::PREC == 0) {
    if (!(g_sel & 64) && ep.hd == 128) {
      TAMF_CLIP_NSUB(Sp, {
        if (ClipLaunch<Op, 2, EpiQK<Op, true>, NS>::applies(B, Sp, 2 * d, ga.K) && ClipLaunch<Op, 2, EpiVt<Op, true>, NS>::applies(B, Sp, d, ga.K)) {
          EpiQK<Op, true> eq{ep.bias, ep.qk, d, ep.qscale, ACT_NONE, ep.ctl, ep.ln};
          hipError_t e = ClipLaunch<Op, 4, EpiQK<Op, true>, NS>::applies(B, Sp, 2 * d, ga.K)
                             ? ClipLaunch<Op, 4, EpiQK<Op, true>, NS>::launch(nullptr, ga.A, ga.lda, ga.W, ga.ldw, B, Sp, 2 * d, ga.K, eq, st)
                             : ClipLaunch<Op, 2, EpiQK<Op, true>, NS>::launch(nullptr, ga.A, ga.lda, ga.W, ga.ldw, B, Sp, 2 * d, ga.K, eq, st);
          if (e != hipSuccess) return e;
          launched("gemm_qk", 2 * d);
          const auto* Wv = (const typename Op::elem_t*)((const char*)ga.W + (size_t)2 * d * d * Op::EB);
          EpiVt<Op, true> ev{ep.bias + 2 * d, ep.vt, ep.H, ep.hd, ep.Skp, ACT_NONE, ep.ctl, ep.ln};
          e = ClipLaunch<Op, 2, EpiVt<Op, true>, NS>::launch(nullptr, ga.A, ga.lda, Wv, ga.ldw, B, Sp, d, ga.K, ev, st);
          if (e == hipSuccess) launched("gemm_v", d);
          return e;
        }
      })
    }
  }
  const hipError_t e = launch_rows<Op>(ga, ep, st);
  if (e == hipSuccess) launched("gemm_qkv", 3 * d);
  return e;
}

// FFN1 (bias + GELU with the row factors of the deferred LayerNorm): whole-clip tiles of 256 columns where they fill their rounds
// (off with selection bit 8), else the rows ladder
template <class Op>
static hipError_t launch_ffn1(const GemmArgs<Op>& ga, const EpiBiasAct<Op, true>& ep, int B, int Sp, hipStream_t st) {
  if (!(g_sel & 8)) {
    TAMF_CLIP_NSUB(Sp, {
      if (ClipLaunch<Op, 4, EpiBiasAct<Op, true>, NS>::applies(B, Sp, ga.N, ga.K))
        return ClipLaunch<Op, 4, EpiBiasAct<Op, true>, NS>::launch(nullptr, ga.A, ga.lda, ga.W, ga.ldw, B, Sp, ga.N, ga.K, ep, st);
    })
  }
  return launch_rows<Op>(ga, ep, st);
}

// ---- attention ----
// kernel attributes of the streaming kernel and of the resident-K kernel (its ceiling: the 160 KB of a CU)
template <class Op, int HD>
static hipError_t attn_prepare() { return lds_once<attn_kernel<Op, HD>>(AttnCfg<Op, HD>::SMEM); }
template <class Op, int HD, int NKB>
static hipError_t attn_res_prepare() { return lds_once<attn_res_kernel<Op, HD, NKB>>(160 * 1024); }

// The resident-K kernel of head width HD with NKB 32-key blocks, when the clip fits it: returns whether it launched (*e: the launch's
// error).  nqt query tiles per clip, split over `chunks` workgroups (grid) of nw waves.
template <class Op, int HD, int NKB>
static bool attn_res_launch(const AttnArgs<Op>& aa, int hd, int nqt, int chunks, int nw, dim3 grid, hipStream_t st, hipError_t* e) {
  typedef AttnRes<Op, HD, NKB> R;
  if (!(hd == HD && R::fits(aa.S, aa.Sp) && nw <= R::MAXW)) return false;
  if ((*e = attn_res_prepare<Op, HD, NKB>()) != hipSuccess) return true;
  int lds = R::smem(aa.S, aa.Sp);
  AttnArgs<Op> a2 = aa;
  int nwl = nw;
  // f32, a clip of 4 n + 1 query tiles (13 at T = 196): its last tile is key-split over four waves (tamf_attn.h) - decided by
  // the clip's length alone, so that a clip's result does not depend on the batch size or the query split.  f32 only: the
  // 16-bit modes' waves overlap on a SIMD, the split buys them nothing at B = 64 and costs 1 - 3 % at B <= 32
  // (whether the split applies is decided on the WORST case of the query split - one workgroup, nqt - 1 tile-owning waves: the
  //  partial area grows with them and the four extra waves then sit at nqt + 3 - so it cannot apply at one batch size and not
  //  at another)
  if (Op::PREC == 0 && nqt % 4 == 1 && nqt >= 5 && nqt + 3 <= R::MAXW && R::ksplit_extra(aa.S, aa.Sp, nqt - 1) >= 0) {
    const int nwq = (nqt - 1 + chunks - 1) / chunks, nlast = nqt - 1 - (chunks - 1) * nwq > 0 ? nqt - 1 - (chunks - 1) * nwq : 0;
    // the four key-split waves go to the SIMDs with the fewest tiles in the last workgroup (wave w runs on SIMD w mod 4)
    const int r = nlast % 4, nlight = r ? 4 - r : 4;
    int hw = 0, top = nwq, used = 0;
    for (int j = 0; j < 4; ++j) {
      const int simd = (r ? r : 0) + j % nlight;
      int idx = nlast + ((simd - nlast % 4) + 4) % 4;
      while (used & (1 << idx)) idx += 4;
      used |= 1 << idx; hw |= idx << (4 * j); if (idx + 1 > top) top = idx + 1;
    }
    const int extra = R::ksplit_extra(aa.S, aa.Sp, nwq);
    if (extra >= 0 && top <= R::MAXW) { a2.ksplit = 1; a2.nwq = nwq; a2.hw = hw; nwl = top; lds += extra; }
  }
  hipLaunchKernelGGL((attn_res_kernel<Op, HD, NKB>), grid, dim3(nwl * 64), lds, st, a2);
  *e = hipGetLastError();
  return true;
}

template <class Op>
static hipError_t launch_attn(const AttnArgs<Op>& aa, int B, int hd, hipStream_t st) {
  const int nqt = (aa.Sp + 15) / 16;
  const int nw_max = 16;  // one workgroup per (clip, head) up to 256 queries: K/V streamed once
  int chunks = (nqt + nw_max - 1) / nw_max;
  // fewer (clip, head) pairs than CUs (B = 32: 128): split the queries of a pair over workgroups until the chip is filled;
  // K/V are then streamed once per workgroup, which costs less than idle CUs (a query's result does not depend on the split)
  while (chunks * B * aa.H < wg_slots() / 2 && chunks * 2 <= nqt) chunks *= 2;
  if ((g_sel & 4) && chunks * 2 <= nqt) chunks *= 2;  // A/B: one more split (two workgroups per CU at B = 64)
  const int nw = (nqt + chunks - 1) / chunks;
  dim3 grid(chunks, B * aa.H);
  constexpr int smem64 = AttnCfg<Op, 64>::SMEM, smem128 = AttnCfg<Op, 128>::SMEM;
  hipError_t e = hipSuccess;
  // up to 224 keys: K resident in LDS, exact two-pass softmax, three barriers (tamf_attn.h AttnRes); the streaming kernel serves
  // longer sequences and the A/B switch (selection bit 512)
  if (!(g_sel & 512)) {
    if (attn_res_launch<Op, 64, 4>(aa, hd, nqt, chunks, nw, grid, st, &e)) return e;  // up to 128 keys
    if (attn_res_launch<Op, 64, 6>(aa, hd, nqt, chunks, nw, grid, st, &e)) return e;  // up to 192 keys: the dataset's clips (T = 160: S = 165, 11 key tiles of the 12)
    if (attn_res_launch<Op, 64, 7>(aa, hd, nqt, chunks, nw, grid, st, &e)) return e;  // up to 224 keys (T = 196)
    if (attn_res_launch<Op, 128, 4>(aa, hd, nqt, chunks, nw, grid, st, &e)) return e;
    if (attn_res_launch<Op, 128, 6>(aa, hd, nqt, chunks, nw, grid, st, &e)) return e;
    if (attn_res_launch<Op, 128, 7>(aa, hd, nqt, chunks, nw, grid, st, &e)) return e;
  }
  if (hd != 64 && hd != 128) return hipErrorInvalidValue;
  if ((e = hd == 64 ? attn_prepare<Op, 64>() : attn_prepare<Op, 128>()) != hipSuccess) return e;
  if (hd == 64) hipLaunchKernelGGL((attn_kernel<Op, 64>), grid, dim3(nw * 64), smem64, st, aa);
  else hipLaunchKernelGGL((attn_kernel<Op, 128>), grid, dim3(nw * 64), smem128, st, aa);
  return hipGetLastError();
}

// the clip-tile kernels of one clip length (NS whole-clip row tiles, NSP row tiles of a row part)
template <class Op, int NS, int NSP>
static hipError_t prepare_clip() {
  hipError_t e;
  // the encoder layers: FFN1 with the row factors of the deferred LayerNorm, the two residual GEMMs (whole clips / row parts)
  if ((e = ClipLaunch<Op, 4, EpiBiasAct<Op, true>, NS>::prepare()) != hipSuccess) return e;
  if ((e = ClipLaunch<Op, 2, EpiResid<Op>, NS>::prepare()) != hipSuccess) return e;
  if ((e = ClipLaunch<Op, 2, EpiResid<Op>, NSP, 2>::prepare()) != hipSuccess) return e;
  if constexpr (Op::PREC == 0) {  // f32: the QKV projection on clip tiles (Q | K columns; V columns transposed)
    if ((e = ClipLaunch<Op, 2, EpiQK<Op, true>, NS>::prepare()) != hipSuccess) return e;
    if ((e = ClipLaunch<Op, 4, EpiQK<Op, true>, NS>::prepare()) != hipSuccess) return e;
    if ((e = ClipLaunch<Op, 2, EpiVt<Op, true>, NS>::prepare()) != hipSuccess) return e;
  }
  // plain fp32 product (tamf_test_gemm, tamf_bench_gemm)
  if ((e = ClipLaunch<Op, 2, EpiStoreF32, NS>::prepare()) != hipSuccess) return e;
  if ((e = ClipLaunch<Op, 2, EpiStoreF32, NSP, 2>::prepare()) != hipSuccess) return e;
  return hipSuccess;
}
template <class Op>
static hipError_t prepare_all() {
  hipError_t e;
  if ((e = GemmLaunch<Op, 128, 128, EpiBiasAct<Op>, true>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 128, 128, EpiQKV<Op>, true>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 128, 128, EpiSeqRows<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 64, 128, EpiHead<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 128, 128, EpiStoreF32, true>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 128, 128, EpiBiasAct<Op, true>, true>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 128, 128, EpiQKV<Op, true>, true>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 128, 128, EpiResid<Op>>::prepare()) != hipSuccess) return e;
  // a few clips per call (small_m_launch): the encoder layers' GEMMs on 32- / 64-row tiles with the deep K pipeline
  if ((e = GemmDeepLaunch<Op, 64, 128, 4, EpiResid<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 32, 128, 4, EpiResid<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 32, 64, 6, EpiResid<Op>, 2, 2>::prepare()) != hipSuccess) return e;
  if constexpr (Op::PREC != 0) {  // 20 - 39 clips per call, 16-bit modes (launch_resid)
    if ((e = GemmDeepLaunch<Op, 64, 128, 3, EpiResid<Op>>::prepare()) != hipSuccess) return e;
  }
  if ((e = GemmDeepLaunch<Op, 64, 128, 4, EpiQKV<Op, true>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 32, 128, 4, EpiQKV<Op, true>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 64, 128, 4, EpiBiasAct<Op, true>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 32, 128, 4, EpiBiasAct<Op, true>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 64, 128, 4, EpiSeqRows<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 32, 128, 4, EpiSeqRows<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 64, 128, 4, EpiHead<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmDeepLaunch<Op, 32, 128, 4, EpiHead<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 64, 128, EpiBiasAct<Op>>::prepare()) != hipSuccess) return e;
  if ((e = GemmLaunch<Op, 64, 128, EpiSeqRows<Op>>::prepare()) != hipSuccess) return e;
  if ((e = prepare_clip<Op, 13, 7>()) != hipSuccess) return e;
  if ((e = prepare_clip<Op, 11, 6>()) != hipSuccess) return e;
  if ((e = ClipLaunch<Op, 4, EpiBiasAct<Op>>::prepare()) != hipSuccess) return e;  // (tamf_bench_gemm: FFN1 without the row factors, T = 196)
  if ((e = ClipLaunch<Op, 4, EpiStoreF32>::prepare()) != hipSuccess) return e;
  if ((e = attn_prepare<Op, 64>()) != hipSuccess) return e;
  if ((e = attn_prepare<Op, 128>()) != hipSuccess) return e;
  if ((e = attn_res_prepare<Op, 64, 7>()) != hipSuccess) return e;
  if ((e = attn_res_prepare<Op, 64, 4>()) != hipSuccess) return e;
  if ((e = attn_res_prepare<Op, 64, 6>()) != hipSuccess) return e;
  if ((e = attn_res_prepare<Op, 128, 6>()) != hipSuccess) return e;
  if ((e = attn_res_prepare<Op, 128, 7>()) != hipSuccess) return e;
  if ((e = attn_res_prepare<Op, 128, 4>()) != hipSuccess) return e;
  return hipSuccess;
}
