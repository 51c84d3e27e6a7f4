// The shape arithmetic of the sampler library, written once: the clip lengths that have clip tiles, the padded sequence shape of a
// call and of a context's workspaces, the V^T row stride, the scratch layout.  Host only and HIP-free: plain C++17 that a stand-alone
// program can #include (tests/test_scratch_layout_cpu.py, tests/test_host_mirror.py, tests/test_weight_prep_cpu.py do).  Nothing here
// launches or decides a launch: that is tamf_launch.h, which includes this header.
#pragma once

static inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The clip lengths that have clip tiles, written here and nowhere else: rows of the whole-clip tile (13 or 11 row tiles of 16) that
// holds a clip of Sp padded rows, 0 for a length without one.
static inline int clip_tile_rows(int Sp) { return (Sp > 176 && Sp <= 208) ? 208 : (Sp > 144 && Sp <= 176) ? 176 : 0; }
// ... the largest of them: what a V^T row of a context's workspaces holds at least (seq_shape_max)
static constexpr int CLIP_TILE_ROWS_MAX = 208;
// ... and for the kernel-level hooks, which take M rows and no clip length: the padded rows per clip when M is whole clips of
// T = 196 (208 rows) or of T = 160 (168 rows), else 0
static inline int clip_rows_of_m(int M) { return M % 208 == 0 ? 208 : (M % 168 == 0 ? 168 : 0); }

// share of the workgroup slots of its rounds that a launch of `tiles` workgroups uses
static inline double round_util(int tiles, int slots) { return (double)tiles / (double)(((tiles + slots - 1) / slots) * slots); }

// Keys per V^T row (the row stride of Vt_op): the sequence rounded up to whole 32-key blocks - and at least the rows of the clip tile
// that writes V^T in f32 (EpiVt stores every row tile of its 208- / 176-row tile, zeros past the clip: T = 174 is S = 179, 192 keys in
// blocks, but 13 row tiles = 208 stored positions - they ran into the next feature's row and, for the last one, past the buffer)
static inline int vt_row_keys(int S, int Sp) {
  const int tile = clip_tile_rows(Sp);
  return ((S > tile ? S : tile) + 31) / 32 * 32;
}

// The sequence shape of a call: T frames behind P prefix rows (G: 5, R: 3) are S token rows, padded to Sp rows per clip (a batch of
// B clips is M = B * Sp rows of the residual stream) and to Skp keys per V^T row.
static constexpr int PREFIX_ROWS_G = 5, PREFIX_ROWS_R = 3;
struct SeqShape {
  int S, Sp, Skp;
};
static inline SeqShape seq_shape(int T, int P) {
  SeqShape s{};
  s.S = T + P;
  s.Sp = round_up(s.S, 8);
  s.Skp = vt_row_keys(s.S, s.Sp);
  return s;
}
// ... and of the workspaces of a context of up to Tmax frames: Skp is a bound, at least vt_row_keys of every shape with T <= Tmax -
// a shorter clip may run on a clip tile whose rows exceed the longest sequence, hence the floor of the largest clip tile
static inline SeqShape seq_shape_max(int Tmax, int P) {
  SeqShape s = seq_shape(Tmax, P);
  s.Skp = round_up(s.S > CLIP_TILE_ROWS_MAX ? s.S : CLIP_TILE_ROWS_MAX, 32);
  return s;
}
// The kernels address operands with 32-bit byte offsets and int element indices: whether a context of max_batch clips of max_frames
// frames stays within them.  Conservative for R: five prefix rows are counted for both kinds.  896 = the widest fp32 state row.
static inline bool dims_fit_32bit_offsets(int max_batch, int max_frames, int ff_size, int latent_dim) {
  const long long mmax = (long long)max_batch * seq_shape(max_frames, PREFIX_ROWS_G).Sp;
  const long long widest = ff_size > 3LL * latent_dim ? ff_size : 3LL * latent_dim;
  return mmax * widest * 4 < (1LL << 32) && (long long)max_batch * max_frames * 896 * 4 < (1LL << 32);
}

// Where the per-layer scratch operands of a context live.  Q | K (Mmax x 2 d), the attention output (Mmax x d) and the input-merge
// hidden rows (B T x d) are dead before FFN1 writes the hidden activations (Mmax x ff) and the hidden activations are dead before the
// next QKV launch, on one stream: when Q | K and the attention output fit side by side into the hidden operand they are VIEWS of its
// allocation (a layer then touches Mmax ff instead of Mmax (ff + 3 d) scratch elements, and an overwrite finds the line it replaces
// still in the Infinity Cache), and the input-merge rows share the bytes of Q | K.  Otherwise `alias` is false and every buffer is an
// allocation of its own.  Offsets are bytes from the start of the allocation, multiples of 256.
//   guard == 0:  [ Q | K ][ attention output ] inside the first hidden_bytes of the allocation; h1 at the offset of Q | K
//   guard  > 0:  test builds (tamf_test_set_guard_bytes).  FFN1 stores every byte of the hidden operand, so a margin BETWEEN two views
//                inside it cannot keep a pattern; with margins the views follow the hidden operand in a longer allocation,
//                [ hidden ] g [ Q | K ] g [ attention output ] g [ h1 ], every g a margin of `guard` pattern bytes (the one behind h1
//                is the allocation's own) that tamf_test_check_guards verifies: an overrun of a view into its neighbour stays visible.  The decision `alias`
//                is that of guard == 0, so that a shape takes the same allocation path with and without margins.
struct ScratchLayout {
  bool alias;
  unsigned long long host_bytes;  // bytes of the allocation that holds the hidden operand (and, with alias, the views)
  unsigned long long qk_off, a_off, h1_off;
  unsigned long long qk_bytes, a_bytes, h1_bytes, hidden_bytes;
};
static inline ScratchLayout scratch_layout(long long Mmax, long long BT, int d, int ff, int elem_bytes, unsigned long long guard) {
  auto up = [](unsigned long long v) { return (v + 255ull) / 256ull * 256ull; };
  ScratchLayout s{};
  s.hidden_bytes = up((unsigned long long)Mmax * ff * elem_bytes);
  s.qk_bytes = up((unsigned long long)Mmax * 2 * d * elem_bytes);
  s.a_bytes = up((unsigned long long)Mmax * d * elem_bytes);
  s.h1_bytes = up((unsigned long long)BT * d * elem_bytes);
  s.host_bytes = s.hidden_bytes;
  s.alias = s.qk_bytes + s.a_bytes <= s.hidden_bytes && s.h1_bytes <= s.qk_bytes;
  if (!s.alias) return s;
  if (guard == 0) {
    s.qk_off = 0;
    s.a_off = s.qk_bytes;
    s.h1_off = 0;
  } else {
    s.qk_off = s.hidden_bytes + guard;
    s.a_off = s.qk_off + s.qk_bytes + guard;
    s.h1_off = s.a_off + s.a_bytes + guard;
    s.host_bytes = s.h1_off + s.h1_bytes;  // (the margin behind h1 is the allocation's own)
  }
  return s;
}
