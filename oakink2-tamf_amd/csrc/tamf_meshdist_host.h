// Host side of libtamf_meshdist.so without a line of HIP: the workspace layout, the argument checks and the packing of the triangle
// tiles, their boxes and the job records.  tamf_meshdist.hip copies what is packed here and launches; a plain C++ program can call
// these functions by themselves (a sanitizer build of the host code needs no GPU).
#pragma once
#include <stdint.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

constexpr int MD_TILE = 64;        // triangle records per tile (TAMF_MESHDIST_TILE)
constexpr int MD_REC = 10;         // doubles per record: a.xyz b.xyz c.xyz | the original face index (int64 bits)
constexpr int MD_BOX = 6;          // doubles per tile box: lo.xyz hi.xyz
constexpr int MD_NT = 256;         // threads = points per work group
constexpr int MD_TC = 16;          // doubles per record of the inside test (MESH_TC of tamf_mesh.h)
constexpr double MD_MARGIN = 9.5367431640625e-07;  // 2^-20 (TAMF_MESHDIST_BOX_MARGIN)

// what the kernels read of one mesh: byte offsets from the workspace's base
struct MdMesh {
  long long tiles_off, boxes_off, tc_off, verts_off, faces_off;
  int ntiles, F, V, pad;
  double sc[3], tr[3];
  double res, pad2[2];
};
static_assert(sizeof(MdMesh) == 128, "mesh descriptor layout");

// one job of tamf_meshdist_points; blk0 = its first work group (an empty job shares its successor's), out0 = its first output
struct MdJob {
  double tr[12];
  long long off, len, blk0, out0;
  int mesh, pad;
  long long pad2;
};
static_assert(sizeof(MdJob) == 144, "job record layout");

struct MdLayout {
  int M = 0;
  long long V_total = 0, F_total = 0, tiles_total = 0;
  long long desc_off = 0, tiles_off = 0, boxes_off = 0, verts_off = 0, faces_off = 0, tc_off = 0, bytes = 0;
  long long upload_bytes = 0;  // [descriptors | tiles | boxes | verts | faces]: what the host packs; the tc records follow
  std::vector<long long> tile0;  // per mesh, first tile
};

static inline long long md_align16(long long x) { return (x + 15) & ~15LL; }

// "" or what is wrong with the offset arrays; fills `L`
static inline std::string md_layout(int32_t M, const int64_t* vert_off, const int64_t* face_off, const int64_t* perm_off, MdLayout& L) {
  if (M < 1 || M > 65535) return "M = " + std::to_string(M) + " outside [1, 65535]";
  if (!vert_off || !face_off || !perm_off) return "null argument";
  if (vert_off[0] != 0 || face_off[0] != 0 || perm_off[0] != 0) return "the offset arrays must start at 0";
  L = MdLayout();
  L.M = M;
  L.tile0.resize((size_t)M);
  for (int m = 0; m < M; ++m) {
    const int64_t V = vert_off[m + 1] - vert_off[m], F = face_off[m + 1] - face_off[m], K = perm_off[m + 1] - perm_off[m];
    if (V < 1 || V > 0x7fffffffLL) return "mesh " + std::to_string(m) + ": " + std::to_string(V) + " vertices (1 .. 2^31 - 1)";
    if (F < 1 || F > (1LL << 26)) return "mesh " + std::to_string(m) + ": " + std::to_string(F) + " faces (1 .. 2^26)";
    if (K < 0 || K > F) return "mesh " + std::to_string(m) + ": " + std::to_string(K) + " valid faces of " + std::to_string(F);
    if (K == 0) return "mesh " + std::to_string(m) + " has no valid face";
    L.tile0[(size_t)m] = L.tiles_total;
    L.tiles_total += (K + MD_TILE - 1) / MD_TILE;
  }
  L.V_total = vert_off[M];
  L.F_total = face_off[M];
  L.desc_off = 0;
  L.tiles_off = md_align16((long long)M * (long long)sizeof(MdMesh));
  L.boxes_off = L.tiles_off + L.tiles_total * MD_TILE * MD_REC * 8;
  L.verts_off = L.boxes_off + L.tiles_total * MD_BOX * 8;
  L.faces_off = L.verts_off + L.V_total * 3 * 8;
  L.upload_bytes = md_align16(L.faces_off + L.F_total * 3 * 4);
  L.tc_off = L.upload_bytes;
  L.bytes = L.tc_off + L.F_total * MD_TC * 8;
  return "";
}

// Packs [descriptors | tiles | boxes | verts | faces] into `buf` (resized to L.upload_bytes).  "" or what is wrong with the meshes.
// The last tile of a mesh is filled up with copies of the mesh's last record: the same (d2, f) again never replaces the best.
static inline std::string md_pack(const MdLayout& L, const double* verts, const int32_t* faces, const int64_t* vert_off,
                                  const int64_t* face_off, const int32_t* perm, const int64_t* perm_off, const double* scale3,
                                  const double* translate3, int32_t hash_resolution, std::vector<unsigned char>& buf) {
  if (!verts || !faces || !perm || !scale3 || !translate3) return "null argument";
  if (hash_resolution < 2) return "hash_resolution = " + std::to_string(hash_resolution) + " < 2";
  buf.assign((size_t)L.upload_bytes, 0);
  MdMesh* desc = (MdMesh*)(buf.data() + L.desc_off);
  double* tiles = (double*)(buf.data() + L.tiles_off);
  double* boxes = (double*)(buf.data() + L.boxes_off);
  std::memcpy(buf.data() + L.verts_off, verts, (size_t)L.V_total * 3 * 8);
  std::memcpy(buf.data() + L.faces_off, faces, (size_t)L.F_total * 3 * 4);
  std::vector<unsigned char> seen;
  for (int m = 0; m < L.M; ++m) {
    const int64_t V = vert_off[m + 1] - vert_off[m], F = face_off[m + 1] - face_off[m], K = perm_off[m + 1] - perm_off[m];
    const double* v = verts + vert_off[m] * 3;
    const int32_t* f = faces + face_off[m] * 3;
    const int32_t* pm = perm + perm_off[m];
    const long long t0 = L.tile0[(size_t)m], nt = (K + MD_TILE - 1) / MD_TILE;
    MdMesh& d = desc[m];
    d.tiles_off = L.tiles_off + t0 * MD_TILE * MD_REC * 8;
    d.boxes_off = L.boxes_off + t0 * MD_BOX * 8;
    d.tc_off = L.tc_off + face_off[m] * MD_TC * 8;
    d.verts_off = L.verts_off + vert_off[m] * 3 * 8;
    d.faces_off = L.faces_off + face_off[m] * 3 * 4;
    d.ntiles = (int)nt;
    d.F = (int)F;
    d.V = (int)V;
    for (int k = 0; k < 3; ++k) {
      d.sc[k] = scale3[m * 3 + k];
      d.tr[k] = translate3[m * 3 + k];
    }
    d.res = (double)hash_resolution;
    seen.assign((size_t)F, 0);
    for (long long t = 0; t < nt; ++t) {
      double* rec = tiles + (t0 + t) * MD_TILE * MD_REC;
      double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
      for (int j = 0; j < MD_TILE; ++j) {
        const int64_t e = t * MD_TILE + j;
        double* r = rec + j * MD_REC;
        if (e >= K) {  // (never the first record of a tile)
          std::memcpy(r, r - MD_REC, MD_REC * 8);
          continue;
        }
        const int32_t fi = pm[e];
        if (fi < 0 || fi >= F) return "mesh " + std::to_string(m) + ": permutation entry " + std::to_string(fi) + " outside [0, " + std::to_string(F) + ")";
        if (seen[(size_t)fi]) return "mesh " + std::to_string(m) + ": face " + std::to_string(fi) + " is listed twice";
        seen[(size_t)fi] = 1;
        const int32_t i0 = f[fi * 3LL], i1 = f[fi * 3LL + 1], i2 = f[fi * 3LL + 2];
        if (i0 < 0 || i0 >= V || i1 < 0 || i1 >= V || i2 < 0 || i2 >= V || i0 == i1 || i1 == i2 || i0 == i2)
          return "mesh " + std::to_string(m) + ": face " + std::to_string(fi) + " is listed as valid but has a repeated index or one outside [0, " + std::to_string(V) + ")";
        const int32_t idx[3] = {i0, i1, i2};
        for (int c = 0; c < 3; ++c)
          for (int k = 0; k < 3; ++k) {
            const double x = v[idx[c] * 3LL + k];
            r[c * 3 + k] = x;
            if (x < lo[k]) lo[k] = x;
            if (x > hi[k]) hi[k] = x;
          }
        const long long tag = fi;
        std::memcpy(r + 9, &tag, 8);
      }
      double amax = 0.0;
      for (int k = 0; k < 3; ++k) {
        if (std::fabs(lo[k]) > amax) amax = std::fabs(lo[k]);
        if (std::fabs(hi[k]) > amax) amax = std::fabs(hi[k]);
      }
      const double mg = MD_MARGIN * amax;  // (a box with a NaN or infinite corner never lets its tile be skipped: the bound is NaN)
      double* bx = boxes + (t0 + t) * MD_BOX;
      for (int k = 0; k < 3; ++k) {
        bx[k] = lo[k] - mg;
        bx[3 + k] = hi[k] + mg;
      }
    }
  }
  return "";
}

// the job records and the number of work groups; "" or what is wrong
static inline std::string md_jobs(int32_t M, int64_t P_total, int32_t J, const int32_t* mesh_id, const double* transf, const int64_t* pt_off,
                                  const int64_t* pt_len, std::vector<MdJob>& jobs, long long& nblk, long long& n_out) {
  if (!mesh_id || !transf || !pt_off || !pt_len) return "null argument";
  if (M < 1 || M > 65535 || J < 1 || P_total < 0)
    return "bad shape (M = " + std::to_string(M) + ", J = " + std::to_string(J) + ", P_total = " + std::to_string(P_total) + ")";
  jobs.resize((size_t)J);
  nblk = 0;
  n_out = 0;
  for (int j = 0; j < J; ++j) {
    if (mesh_id[j] < 0 || mesh_id[j] >= M) return "mesh_id[" + std::to_string(j) + "] = " + std::to_string(mesh_id[j]) + " outside [0, M)";
    const int64_t off = pt_off[j], len = pt_len[j];
    if (off < 0 || len < 0 || off > P_total || len > P_total - off)
      return "slice of job " + std::to_string(j) + " [" + std::to_string(off) + ", +" + std::to_string(len) + ") leaves the " + std::to_string(P_total) + " points";
    MdJob& r = jobs[(size_t)j];
    std::memset(&r, 0, sizeof(MdJob));
    std::memcpy(r.tr, transf + (size_t)j * 12, 12 * sizeof(double));
    r.off = off;
    r.len = len;
    r.blk0 = nblk;
    r.out0 = n_out;
    r.mesh = mesh_id[j];
    nblk += (len + MD_NT - 1) / MD_NT;
    n_out += len;
    if (nblk > 0x7fffffffLL) return "too many points for one call: split the jobs";
  }
  return "";
}
