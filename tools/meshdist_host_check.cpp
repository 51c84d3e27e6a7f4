// The host code of libtamf_meshdist.so by itself: csrc/tamf_meshdist_host.h has no HIP in it, so its layout, packing and argument
// checks run on any CPU.  tests/test_meshdist_cpu.py builds and runs this plainly; built with -fsanitize=address,undefined it is the
// sanitizer run of the library's host side (no GPU, nothing loaded into another process).
//
//   c++ -std=c++17 -fsanitize=address,undefined -I oakink2-tamf_amd/csrc -o meshdist_host_check tools/meshdist_host_check.cpp && ./meshdist_host_check
#include <cstdio>
#include <cstdlib>

#include "tamf_meshdist_host.h"

static int failures = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                                    \
    }                                                                \
  } while (0)

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

int main() {
  // mesh 0: a strip of 70 triangles over 72 vertices (two tiles: 64 + 6 records, 58 padded); mesh 1: one triangle of three faces listed
  std::vector<double> verts;
  std::vector<int32_t> faces, perm;
  for (int i = 0; i < 72; ++i) {
    verts.push_back(0.5 * (i / 2));
    verts.push_back((double)(i % 2));
    verts.push_back(-3.0 + 0.01 * i);
  }
  for (int i = 0; i < 70; ++i) {
    faces.push_back(i);
    faces.push_back(i + 1);
    faces.push_back(i + 2);
  }
  for (int i = 69; i >= 0; --i) perm.push_back(i);  // (any order is a permutation)
  const double tri[9] = {10, 10, 10, 11, 10, 10, 10, 11, 10};
  verts.insert(verts.end(), tri, tri + 9);
  const int32_t f1[9] = {0, 0, 1, 0, 1, 2, 0, 1, 7};  // a repeated index, a valid face, an index outside the mesh
  faces.insert(faces.end(), f1, f1 + 9);
  perm.push_back(1);
  const int64_t vert_off[3] = {0, 72, 75}, face_off[3] = {0, 70, 73}, perm_off[3] = {0, 70, 71};
  const double sc[6] = {1, 2, 3, 4, 5, 6}, tr[6] = {-1, -2, -3, -4, -5, -6};

  MdLayout L;
  CHECK(md_layout(2, vert_off, face_off, perm_off, L).empty());
  CHECK(L.tiles_total == 3 && L.tile0[0] == 0 && L.tile0[1] == 2 && L.V_total == 75 && L.F_total == 73);
  CHECK(L.tiles_off == 256 && L.boxes_off == L.tiles_off + 3 * MD_TILE * MD_REC * 8 && L.verts_off == L.boxes_off + 3 * MD_BOX * 8);
  CHECK(L.faces_off == L.verts_off + 75 * 24 && L.upload_bytes % 16 == 0 && L.upload_bytes >= L.faces_off + 73 * 12 && L.bytes == L.tc_off + 73 * MD_TC * 8);

  std::vector<unsigned char> buf;
  CHECK(md_pack(L, verts.data(), faces.data(), vert_off, face_off, perm.data(), perm_off, sc, tr, 512, buf).empty());
  CHECK((long long)buf.size() == L.upload_bytes);
  const MdMesh* d = (const MdMesh*)buf.data();
  CHECK(d[0].ntiles == 2 && d[0].F == 70 && d[0].V == 72 && d[1].ntiles == 1 && d[1].F == 3 && d[1].V == 3);
  CHECK(d[0].tiles_off == L.tiles_off && d[1].tiles_off == L.tiles_off + 2 * MD_TILE * MD_REC * 8 && d[1].boxes_off == L.boxes_off + 2 * MD_BOX * 8);
  CHECK(d[1].tc_off == L.tc_off + 70 * MD_TC * 8 && d[1].verts_off == L.verts_off + 72 * 24 && d[1].faces_off == L.faces_off + 70 * 12);
  CHECK(d[0].sc[2] == 3 && d[1].sc[0] == 4 && d[1].tr[2] == -6 && d[0].res == 512.0);
  const double* tiles = (const double*)(buf.data() + L.tiles_off);
  const double* boxes = (const double*)(buf.data() + L.boxes_off);
  for (int e = 0; e < 2 * MD_TILE; ++e) {  // record e of mesh 0 is face perm[e], the padding repeats the last one
    const double* r = tiles + e * MD_REC;
    const int fi = perm[e < 70 ? e : 69];
    long long tag;
    std::memcpy(&tag, r + 9, 8);
    CHECK(tag == fi);
    for (int c = 0; c < 3; ++c)
      for (int k = 0; k < 3; ++k) CHECK(r[c * 3 + k] == verts[(size_t)faces[fi * 3 + c] * 3 + k]);
  }
  long long tag1;
  std::memcpy(&tag1, tiles + 2 * MD_TILE * MD_REC + 9, 8);
  CHECK(tag1 == 1);  // the original index, local to mesh 1
  // tile 0 of mesh 0 holds faces 69 .. 6, i.e. vertices 6 .. 71: its box, inflated by 2^-20 of its largest |coordinate| (17.5)
  const double mg = MD_MARGIN * 17.5;
  CHECK(boxes[0] == 1.5 - mg && boxes[3] == 17.5 + mg && boxes[1] == 0.0 - mg && boxes[4] == 1.0 + mg && boxes[2] == (-3.0 + 0.01 * 6) - mg &&
        boxes[5] == (-3.0 + 0.01 * 71) + mg);
  CHECK(boxes[2 * MD_BOX + 0] == 10.0 - MD_MARGIN * 11.0 && boxes[2 * MD_BOX + 4] == 11.0 + MD_MARGIN * 11.0);
  CHECK(std::memcmp(buf.data() + L.verts_off, verts.data(), verts.size() * 8) == 0 && std::memcmp(buf.data() + L.faces_off, faces.data(), faces.size() * 4) == 0);

  // refusals of the layout
  MdLayout X;
  CHECK(has(md_layout(0, vert_off, face_off, perm_off, X), "outside [1, 65535]"));
  CHECK(has(md_layout(2, nullptr, face_off, perm_off, X), "null"));
  const int64_t no_valid[3] = {0, 70, 70}, too_many[3] = {0, 71, 72}, no_vert[3] = {0, 72, 72}, shifted[3] = {1, 72, 75};
  CHECK(has(md_layout(2, vert_off, face_off, no_valid, X), "mesh 1 has no valid face"));
  CHECK(has(md_layout(2, vert_off, face_off, too_many, X), "valid faces of"));
  CHECK(has(md_layout(2, no_vert, face_off, perm_off, X), "vertices"));
  CHECK(has(md_layout(2, shifted, face_off, perm_off, X), "start at 0"));
  // refusals of the packing
  std::vector<int32_t> bad = perm;
  bad[3] = 70;
  CHECK(has(md_pack(L, verts.data(), faces.data(), vert_off, face_off, bad.data(), perm_off, sc, tr, 512, buf), "outside [0, 70)"));
  bad = perm;
  bad[5] = bad[4];
  CHECK(has(md_pack(L, verts.data(), faces.data(), vert_off, face_off, bad.data(), perm_off, sc, tr, 512, buf), "listed twice"));
  for (int32_t listed : {0, 2}) {  // the repeated index, the index outside the mesh
    bad = perm;
    bad[70] = listed;
    CHECK(has(md_pack(L, verts.data(), faces.data(), vert_off, face_off, bad.data(), perm_off, sc, tr, 512, buf), "listed as valid"));
  }
  CHECK(has(md_pack(L, verts.data(), faces.data(), vert_off, face_off, perm.data(), perm_off, sc, tr, 1, buf), "hash_resolution"));
  CHECK(has(md_pack(L, nullptr, faces.data(), vert_off, face_off, perm.data(), perm_off, sc, tr, 512, buf), "null"));

  // the job records
  const int32_t mesh_id[4] = {1, 0, 0, 1};
  const int64_t off[4] = {0, 10, 300, 0}, len[4] = {10, 257, 0, 1};
  double transf[48];
  for (int i = 0; i < 48; ++i) transf[i] = i;
  std::vector<MdJob> jobs;
  long long nblk = -1, n_out = -1;
  CHECK(md_jobs(2, 300, 4, mesh_id, transf, off, len, jobs, nblk, n_out).empty());
  CHECK(nblk == 4 && n_out == 268 && jobs.size() == 4);
  CHECK(jobs[0].blk0 == 0 && jobs[1].blk0 == 1 && jobs[2].blk0 == 3 && jobs[3].blk0 == 3 && jobs[1].out0 == 10 && jobs[3].out0 == 267);
  CHECK(jobs[2].tr[0] == 24 && jobs[3].tr[11] == 47 && jobs[1].mesh == 0 && jobs[1].off == 10 && jobs[1].len == 257);
  int32_t bad_id[4] = {1, 2, 0, 1};
  CHECK(has(md_jobs(2, 300, 4, bad_id, transf, off, len, jobs, nblk, n_out), "mesh_id[1] = 2"));
  int64_t bad_len[4] = {10, 291, 0, 1};
  CHECK(has(md_jobs(2, 300, 4, mesh_id, transf, off, bad_len, jobs, nblk, n_out), "leaves the 300 points"));
  bad_len[1] = -1;
  CHECK(has(md_jobs(2, 300, 4, mesh_id, transf, off, bad_len, jobs, nblk, n_out), "slice of job 1"));
  CHECK(has(md_jobs(2, 300, 0, mesh_id, transf, off, len, jobs, nblk, n_out), "bad shape"));
  CHECK(has(md_jobs(2, 300, 4, mesh_id, nullptr, off, len, jobs, nblk, n_out), "null"));

  if (failures) {
    std::printf("%d host checks failed\n", failures);
    return 1;
  }
  std::printf("host check ok\n");
  return 0;
}
