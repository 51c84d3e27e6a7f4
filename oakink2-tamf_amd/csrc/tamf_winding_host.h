// Host side of libtamf_winding.so without a line of HIP: the workspace layout, the argument checks, the chunk table, the packing of
// the face records and the job records, and the launch geometry (spread the chunks over work groups, or loop over them in a thread).
// tamf_winding.hip copies what is packed here and launches; a plain C++ program can call these functions by themselves (a sanitizer
// build of the host code needs no GPU).
#pragma once
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

constexpr int WN_CHUNK = 1024;  // valid faces per partial sum (TAMF_WINDING_CHUNK)
constexpr int WN_TILE = 128;    // face records staged through LDS at a time; divides WN_CHUNK
constexpr int WN_REC = 9;       // doubles per record: a.xyz b.xyz c.xyz
constexpr int WN_NT = 256;      // threads = points per work group
constexpr unsigned WN_FORCE_LOOP = 1u, WN_FORCE_SPREAD = 2u;
constexpr long long WN_SPREAD_BELOW_GROUPS = 1024;       // spread when the points alone give fewer work groups than 4 per CU of 256
constexpr long long WN_SPREAD_MAX_BYTES = 256LL << 20;   // ... and the partials stay below this
static_assert(WN_CHUNK % WN_TILE == 0, "a tile never straddles two chunks");

// what the kernels read of one mesh: rec_off = byte offset of its records from the workspace's base
struct WnMesh {
  long long rec_off;
  int K, nchunks;  // valid faces; ceil(K / WN_CHUNK)
};
static_assert(sizeof(WnMesh) == 16, "mesh descriptor layout");

// one job of tamf_winding_points; blk0 = its first block of 256 points (an empty job shares its successor's), out0 = its first output
struct WnJob {
  double tr[12];
  long long off, len, blk0, out0;
  int mesh, nchunks;  // nchunks: of its mesh, by the host's valid_off
  long long pad;
};
static_assert(sizeof(WnJob) == 144, "job record layout");

struct WnLayout {
  int M = 0;
  long long V_total = 0, F_total = 0, K_total = 0;
  long long desc_off = 0, rec_off = 0, bytes = 0;
  std::vector<long long> rec0;  // per mesh, first record
};

struct WnPlan {
  bool spread = false;
  long long nblk = 0, n_out = 0;  // blocks of 256 points, outputs
  int max_chunks = 1;             // over the jobs that have points
  long long groups = 0;           // work groups of the first launch
  long long jobs_bytes = 0, partial_off = 0, bytes = 0;
};

static inline long long wn_align16(long long x) { return (x + 15) & ~15LL; }

// the chunk table: chunk c of K valid faces covers [first, first + count)
static inline int wn_nchunks(long long K) { return (int)((K + WN_CHUNK - 1) / WN_CHUNK); }
static inline void wn_chunk(long long K, int c, long long& first, int& count) {
  first = (long long)c * WN_CHUNK;
  const long long left = K - first;
  count = left >= WN_CHUNK ? WN_CHUNK : left > 0 ? (int)left : 0;
}

// "" or what is wrong with the offset arrays; fills `L`
static inline std::string wn_layout(int32_t M, const int64_t* vert_off, const int64_t* face_off, const int64_t* valid_off, WnLayout& L) {
  if (M < 1 || M > 65535) return "M = " + std::to_string(M) + " outside [1, 65535]";
  if (!vert_off || !face_off || !valid_off) return "null argument";
  if (vert_off[0] != 0 || face_off[0] != 0 || valid_off[0] != 0) return "the offset arrays must start at 0";
  L = WnLayout();
  L.M = M;
  L.rec0.resize((size_t)M);
  for (int m = 0; m < M; ++m) {
    const int64_t V = vert_off[m + 1] - vert_off[m], F = face_off[m + 1] - face_off[m], K = valid_off[m + 1] - valid_off[m];
    if (V < 1 || V > 0x7fffffffLL) return "mesh " + std::to_string(m) + ": " + std::to_string(V) + " vertices (1 .. 2^31 - 1)";
    if (F < 1 || F > (1LL << 26)) return "mesh " + std::to_string(m) + ": " + std::to_string(F) + " faces (1 .. 2^26)";
    if (K < 0 || K > F) return "mesh " + std::to_string(m) + ": " + std::to_string(K) + " valid faces of " + std::to_string(F);
    if (K == 0) return "mesh " + std::to_string(m) + " has no valid face";
    L.rec0[(size_t)m] = L.K_total;
    L.K_total += K;
  }
  L.V_total = vert_off[M];
  L.F_total = face_off[M];
  L.desc_off = 0;
  L.rec_off = wn_align16((long long)M * (long long)sizeof(WnMesh));
  L.bytes = wn_align16(L.rec_off + L.K_total * WN_REC * 8);
  return "";
}

// Packs [descriptors | records] into `buf` (resized to L.bytes).  "" or what is wrong with the meshes.
static inline std::string wn_pack(const WnLayout& L, const double* verts, const int32_t* faces, const int64_t* vert_off,
                                  const int64_t* face_off, const int32_t* valid, const int64_t* valid_off, std::vector<unsigned char>& buf) {
  if (!verts || !faces || !valid) return "null argument";
  buf.assign((size_t)L.bytes, 0);
  WnMesh* desc = (WnMesh*)(buf.data() + L.desc_off);
  double* recs = (double*)(buf.data() + L.rec_off);
  for (int m = 0; m < L.M; ++m) {
    const int64_t V = vert_off[m + 1] - vert_off[m], F = face_off[m + 1] - face_off[m], K = valid_off[m + 1] - valid_off[m];
    const double* v = verts + vert_off[m] * 3;
    const int32_t* f = faces + face_off[m] * 3;
    const int32_t* vl = valid + valid_off[m];
    WnMesh& d = desc[m];
    d.rec_off = L.rec_off + L.rec0[(size_t)m] * WN_REC * 8;
    d.K = (int)K;
    d.nchunks = wn_nchunks(K);
    double* r = recs + L.rec0[(size_t)m] * WN_REC;
    long long prev = -1;
    for (int64_t e = 0; e < K; ++e, r += WN_REC) {
      const int32_t fi = vl[e];
      if (fi < 0 || fi >= F) return "mesh " + std::to_string(m) + ": valid-face entry " + std::to_string(fi) + " outside [0, " + std::to_string(F) + ")";
      if (fi <= prev) return "mesh " + std::to_string(m) + ": the valid faces are not strictly ascending at entry " + std::to_string(e);
      prev = fi;
      const int32_t idx[3] = {f[fi * 3LL], f[fi * 3LL + 1], f[fi * 3LL + 2]};
      if (idx[0] < 0 || idx[0] >= V || idx[1] < 0 || idx[1] >= V || idx[2] < 0 || idx[2] >= V || idx[0] == idx[1] || idx[1] == idx[2] || idx[0] == idx[2])
        return "mesh " + std::to_string(m) + ": face " + std::to_string(fi) + " is listed as valid but has a repeated index or one outside [0, " + std::to_string(V) + ")";
      for (int c = 0; c < 3; ++c)
        for (int k = 0; k < 3; ++k) r[c * 3 + k] = v[idx[c] * 3LL + k];
    }
  }
  return "";
}

// "" or what is wrong with valid_off for M meshes (what a points call needs of it: the chunk count of every mesh)
static inline std::string wn_bad_valid_off(int32_t M, const int64_t* valid_off) {
  if (M < 1 || M > 65535) return "M = " + std::to_string(M) + " outside [1, 65535]";
  if (!valid_off) return "null argument";
  if (valid_off[0] != 0) return "the offset arrays must start at 0";
  for (int m = 0; m < M; ++m) {
    const int64_t K = valid_off[m + 1] - valid_off[m];
    if (K < 1 || K > (1LL << 26)) return "mesh " + std::to_string(m) + ": " + std::to_string(K) + " valid faces (1 .. 2^26)";
  }
  return "";
}

// The launch geometry of a points call, from its sizes alone: nblk blocks of 256 points, max_chunks the largest chunk count of a job
// with points.  Looped: nblk work groups.  Spread: nblk * max_chunks work groups (a group whose chunk its mesh does not have leaves
// at once), one partial per (chunk, output), then n_out threads add them in chunk order.  "" or why the call is refused.
static inline std::string wn_plan(int32_t J, long long nblk, long long n_out, int max_chunks, uint32_t flags, WnPlan& P) {
  if (J < 1) return "J = " + std::to_string(J) + " < 1";
  if (flags & ~(WN_FORCE_LOOP | WN_FORCE_SPREAD)) return "unknown flags " + std::to_string(flags);
  if ((flags & WN_FORCE_LOOP) && (flags & WN_FORCE_SPREAD)) return "flags force both routes";
  P = WnPlan();
  P.nblk = nblk;
  P.n_out = n_out;
  P.max_chunks = max_chunks < 1 ? 1 : max_chunks;
  const long long groups = nblk * P.max_chunks, pbytes = n_out * P.max_chunks * 8;  // (nblk < 2^31, max_chunks <= 2^16, n_out < 2^39)
  const bool fits = groups <= 0x7fffffffLL;
  if (flags & WN_FORCE_SPREAD) {
    if (!fits) return "a forced spread of " + std::to_string(groups) + " work groups is too large for one launch: split the jobs";
    P.spread = nblk > 0;
  } else if (flags & WN_FORCE_LOOP) {
    P.spread = false;
  } else {
    P.spread = nblk > 0 && nblk < WN_SPREAD_BELOW_GROUPS && P.max_chunks >= 2 && fits && pbytes <= WN_SPREAD_MAX_BYTES;
  }
  P.groups = P.spread ? groups : nblk;
  P.jobs_bytes = wn_align16((long long)J * (long long)sizeof(WnJob));
  P.partial_off = P.jobs_bytes;
  P.bytes = P.jobs_bytes + (P.spread ? pbytes : 0);
  return "";
}

// nblk, n_out and max_chunks of a call from mesh_id, pt_len and valid_off (what the workspace query and the call share); "" or what is wrong
static inline std::string wn_sizes(int32_t M, int32_t J, const int32_t* mesh_id, const int64_t* pt_len, const int64_t* valid_off, long long& nblk,
                                   long long& n_out, int& max_chunks) {
  if (!mesh_id || !pt_len) return "null argument";
  const std::string err = wn_bad_valid_off(M, valid_off);
  if (!err.empty()) return err;
  if (J < 1) return "J = " + std::to_string(J) + " < 1";
  nblk = 0;
  n_out = 0;
  max_chunks = 1;
  for (int j = 0; j < J; ++j) {
    if (mesh_id[j] < 0 || mesh_id[j] >= M) return "mesh_id[" + std::to_string(j) + "] = " + std::to_string(mesh_id[j]) + " outside [0, M)";
    const int64_t len = pt_len[j];
    if (len < 0) return "pt_len[" + std::to_string(j) + "] = " + std::to_string(len) + " is negative";
    nblk += (len + WN_NT - 1) / WN_NT;
    n_out += len;
    if (nblk > 0x7fffffffLL) return "too many points for one call: split the jobs";
    const int nc = wn_nchunks(valid_off[mesh_id[j] + 1] - valid_off[mesh_id[j]]);
    if (len > 0 && nc > max_chunks) max_chunks = nc;
  }
  return "";
}

// the job records; "" or what is wrong (after wn_sizes accepted the same arrays)
static inline std::string wn_jobs(int32_t M, int64_t P_total, int32_t J, const int32_t* mesh_id, const double* transf, const int64_t* pt_off,
                                  const int64_t* pt_len, const int64_t* valid_off, std::vector<WnJob>& jobs) {
  if (!mesh_id || !transf || !pt_off || !pt_len || !valid_off) return "null argument";
  if (M < 1 || M > 65535 || J < 1 || P_total < 0)
    return "bad shape (M = " + std::to_string(M) + ", J = " + std::to_string(J) + ", P_total = " + std::to_string(P_total) + ")";
  jobs.resize((size_t)J);
  long long nblk = 0, n_out = 0;
  for (int j = 0; j < J; ++j) {
    if (mesh_id[j] < 0 || mesh_id[j] >= M) return "mesh_id[" + std::to_string(j) + "] = " + std::to_string(mesh_id[j]) + " outside [0, M)";
    const int64_t off = pt_off[j], len = pt_len[j];
    if (off < 0 || len < 0 || off > P_total || len > P_total - off)
      return "slice of job " + std::to_string(j) + " [" + std::to_string(off) + ", +" + std::to_string(len) + ") leaves the " + std::to_string(P_total) + " points";
    WnJob& r = jobs[(size_t)j];
    std::memset(&r, 0, sizeof(WnJob));
    std::memcpy(r.tr, transf + (size_t)j * 12, 12 * sizeof(double));
    r.off = off;
    r.len = len;
    r.blk0 = nblk;
    r.out0 = n_out;
    r.mesh = mesh_id[j];
    r.nchunks = wn_nchunks(valid_off[mesh_id[j] + 1] - valid_off[mesh_id[j]]);
    nblk += (len + WN_NT - 1) / WN_NT;
    n_out += len;
  }
  return "";
}
