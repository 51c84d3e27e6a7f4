// The host code of libtamf_winding.so by itself: csrc/tamf_winding_host.h has no HIP in it, so its argument checks, its chunk table,
// its packing and its launch geometry run on any CPU.  tests/test_winding_cpu.py builds and runs this plainly; built with
// -fsanitize=address,undefined it is the sanitizer run of the library's host side (no GPU, nothing loaded into another process).
//
//   c++ -std=c++17 -fsanitize=address,undefined -I oakink2-tamf_amd/csrc -o winding_host_check tools/winding_host_check.cpp && ./winding_host_check
#include <cstdio>
#include <cstdlib>

#include "tamf_winding_host.h"

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
  // ---- the chunk table -----------------------------------------------------------------------------------------------------------
  struct {
    long long K;
    int n, last;
  } table[] = {{1, 1, 1}, {1023, 1, 1023}, {1024, 1, 1024}, {1025, 2, 1}, {2049, 3, 1}, {5120, 5, 1024}, {100352, 98, 1024}};
  for (auto& t : table) {
    CHECK(wn_nchunks(t.K) == t.n);
    long long covered = 0;
    for (int c = 0; c < t.n; ++c) {
      long long first;
      int count;
      wn_chunk(t.K, c, first, count);
      CHECK(first == covered && count >= 1 && count <= WN_CHUNK);
      CHECK(count == (c + 1 < t.n ? WN_CHUNK : t.last));
      covered += count;
    }
    CHECK(covered == t.K);
    long long first;
    int count;
    wn_chunk(t.K, t.n, first, count);  // (past the end: empty)
    CHECK(count == 0);
  }

  // ---- the layout and its refusals -----------------------------------------------------------------------------------------------
  // two meshes: a tetrahedron (4 faces, all valid) and a square of two triangles plus one face that is not listed
  const double verts[] = {0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, 1, /* mesh 1 */ 0, 0, 0, 1, 0, 0, 1, 1, 0, 0, 1, 0};
  const int32_t faces[] = {0, 2, 1, 0, 1, 3, 0, 3, 2, 1, 2, 3, /* mesh 1 */ 0, 1, 2, 1, 1, 2, 0, 2, 3};
  const int64_t voff[] = {0, 4, 8}, foff[] = {0, 4, 7}, koff[] = {0, 4, 6};
  const int32_t valid[] = {0, 1, 2, 3, 0, 2};
  WnLayout L;
  CHECK(wn_layout(2, voff, foff, koff, L).empty());
  CHECK(L.K_total == 6 && L.rec_off == 32 && L.bytes == 32 + 6 * 72 && L.rec0[0] == 0 && L.rec0[1] == 4);
  CHECK(has(wn_layout(0, voff, foff, koff, L), "outside [1, 65535]") && has(wn_layout(65536, voff, foff, koff, L), "outside [1, 65535]"));
  CHECK(has(wn_layout(2, nullptr, foff, koff, L), "null") && has(wn_layout(2, voff, nullptr, koff, L), "null") && has(wn_layout(2, voff, foff, nullptr, L), "null"));
  {
    const int64_t bad0[] = {1, 4, 8};
    CHECK(has(wn_layout(2, bad0, foff, koff, L), "start at 0") && has(wn_layout(2, voff, bad0, koff, L), "start at 0") && has(wn_layout(2, voff, foff, bad0, L), "start at 0"));
    const int64_t nov[] = {0, 0, 8}, nof[] = {0, 0, 7}, nok[] = {0, 0, 2}, many[] = {0, 5, 6}, dec[] = {0, 4, 3};
    CHECK(has(wn_layout(2, nov, foff, koff, L), "0 vertices"));
    CHECK(has(wn_layout(2, voff, nof, koff, L), "0 faces"));
    CHECK(has(wn_layout(2, voff, foff, nok, L), "no valid face"));
    CHECK(has(wn_layout(2, voff, foff, many, L), "5 valid faces of 4"));
    CHECK(has(wn_layout(2, voff, foff, dec, L), "-1 valid faces"));
  }

  // ---- the packing and its refusals ----------------------------------------------------------------------------------------------
  CHECK(wn_layout(2, voff, foff, koff, L).empty());
  std::vector<unsigned char> buf;
  CHECK(wn_pack(L, verts, faces, voff, foff, valid, koff, buf).empty());
  CHECK((long long)buf.size() == L.bytes);
  {
    const WnMesh* d = (const WnMesh*)buf.data();
    CHECK(d[0].rec_off == 32 && d[0].K == 4 && d[0].nchunks == 1 && d[1].rec_off == 32 + 4 * 72 && d[1].K == 2 && d[1].nchunks == 1);
    const double* r = (const double*)(buf.data() + d[1].rec_off) + WN_REC;  // mesh 1, second record = face 2 = (0, 2, 3)
    CHECK(r[0] == 0 && r[1] == 0 && r[3] == 1 && r[4] == 1 && r[6] == 0 && r[7] == 1);
  }
  CHECK(has(wn_pack(L, nullptr, faces, voff, foff, valid, koff, buf), "null") && has(wn_pack(L, verts, nullptr, voff, foff, valid, koff, buf), "null") &&
        has(wn_pack(L, verts, faces, voff, foff, nullptr, koff, buf), "null"));
  {
    const int32_t same[] = {0, 1, 2, 3, 2, 2}, desc[] = {0, 1, 3, 2, 0, 2}, outside[] = {0, 1, 2, 3, 0, 3}, negative[] = {0, 1, 2, 3, -1, 2},
                  repeated[] = {0, 1, 2, 3, 0, 1};
    CHECK(has(wn_pack(L, verts, faces, voff, foff, same, koff, buf), "not strictly ascending"));
    CHECK(has(wn_pack(L, verts, faces, voff, foff, desc, koff, buf), "not strictly ascending"));
    CHECK(has(wn_pack(L, verts, faces, voff, foff, outside, koff, buf), "outside [0, 3)"));
    CHECK(has(wn_pack(L, verts, faces, voff, foff, negative, koff, buf), "outside [0, 3)"));
    CHECK(has(wn_pack(L, verts, faces, voff, foff, repeated, koff, buf), "repeated index"));
    int32_t far[21];
    std::memcpy(far, faces, sizeof(far));
    far[2] = 4;  // face 0 of mesh 0 names vertex 4 of 4
    CHECK(has(wn_pack(L, verts, far, voff, foff, valid, koff, buf), "outside [0, 4)"));
    far[2] = -1;
    CHECK(has(wn_pack(L, verts, far, voff, foff, valid, koff, buf), "outside [0, 4)"));
  }

  // ---- the sizes and the jobs of a points call -----------------------------------------------------------------------------------
  const int64_t big_koff[] = {0, 5, 5 + 2049, 5 + 2049 + 1024};  // chunk counts 1, 3, 1
  const int32_t mesh_id[] = {1, 0, 2, 1};
  const int64_t pt_off[] = {0, 10, 0, 300}, pt_len[] = {257, 0, 256, 1};
  double tr[48];
  for (int i = 0; i < 48; ++i) tr[i] = i;
  long long nblk, n_out;
  int maxc;
  CHECK(wn_sizes(3, 4, mesh_id, pt_len, big_koff, nblk, n_out, maxc).empty());
  CHECK(nblk == 2 + 0 + 1 + 1 && n_out == 514 && maxc == 3);
  {
    const int32_t only0[] = {0, 1};
    const int64_t len0[] = {5, 0};  // the job on the 3-chunk mesh has no point: it does not count
    CHECK(wn_sizes(3, 2, only0, len0, big_koff, nblk, n_out, maxc).empty() && maxc == 1 && nblk == 1 && n_out == 5);
    const int32_t badm[] = {0, 3}, negm[] = {-1, 0};
    CHECK(has(wn_sizes(3, 2, badm, len0, big_koff, nblk, n_out, maxc), "outside [0, M)") && has(wn_sizes(3, 2, negm, len0, big_koff, nblk, n_out, maxc), "outside [0, M)"));
    const int64_t neglen[] = {5, -1};
    CHECK(has(wn_sizes(3, 2, only0, neglen, big_koff, nblk, n_out, maxc), "negative"));
    CHECK(has(wn_sizes(3, 0, only0, len0, big_koff, nblk, n_out, maxc), "J = 0"));
    CHECK(has(wn_sizes(3, 2, nullptr, len0, big_koff, nblk, n_out, maxc), "null") && has(wn_sizes(3, 2, only0, nullptr, big_koff, nblk, n_out, maxc), "null") &&
          has(wn_sizes(3, 2, only0, len0, nullptr, nblk, n_out, maxc), "null"));
    CHECK(has(wn_sizes(0, 2, only0, len0, big_koff, nblk, n_out, maxc), "outside [1, 65535]"));
    const int64_t empty_mesh[] = {0, 5, 5, 9}, bad_start[] = {2, 5, 7, 9};
    CHECK(has(wn_sizes(3, 2, only0, len0, empty_mesh, nblk, n_out, maxc), "0 valid faces") && has(wn_sizes(3, 2, only0, len0, bad_start, nblk, n_out, maxc), "start at 0"));
    const int64_t huge[] = {(1LL << 39), (1LL << 39)};
    CHECK(has(wn_sizes(3, 2, only0, huge, big_koff, nblk, n_out, maxc), "split the jobs"));
  }
  std::vector<WnJob> jobs;
  CHECK(wn_jobs(3, 301, 4, mesh_id, tr, pt_off, pt_len, big_koff, jobs).empty());
  CHECK(jobs.size() == 4 && jobs[0].blk0 == 0 && jobs[1].blk0 == 2 && jobs[2].blk0 == 2 && jobs[3].blk0 == 3);
  CHECK(jobs[0].out0 == 0 && jobs[1].out0 == 257 && jobs[2].out0 == 257 && jobs[3].out0 == 513);
  CHECK(jobs[0].nchunks == 3 && jobs[1].nchunks == 1 && jobs[2].nchunks == 1 && jobs[3].mesh == 1 && jobs[3].off == 300 && jobs[3].tr[11] == 47);
  CHECK(has(wn_jobs(3, 300, 4, mesh_id, tr, pt_off, pt_len, big_koff, jobs), "leaves the 300 points"));  // (job 3 ends at 301)
  {
    const int64_t negoff[] = {0, -1, 0, 300}, pastoff[] = {0, 302, 0, 300};
    CHECK(has(wn_jobs(3, 301, 4, mesh_id, tr, negoff, pt_len, big_koff, jobs), "leaves") && has(wn_jobs(3, 301, 4, mesh_id, tr, pastoff, pt_len, big_koff, jobs), "leaves"));
    const int32_t badm[] = {1, 0, 3, 1};
    CHECK(has(wn_jobs(3, 301, 4, badm, tr, pt_off, pt_len, big_koff, jobs), "outside [0, M)"));
    CHECK(has(wn_jobs(3, -1, 4, mesh_id, tr, pt_off, pt_len, big_koff, jobs), "bad shape") && has(wn_jobs(3, 301, 0, mesh_id, tr, pt_off, pt_len, big_koff, jobs), "bad shape") &&
          has(wn_jobs(0, 301, 4, mesh_id, tr, pt_off, pt_len, big_koff, jobs), "bad shape"));
    CHECK(has(wn_jobs(3, 301, 4, mesh_id, nullptr, pt_off, pt_len, big_koff, jobs), "null") && has(wn_jobs(3, 301, 4, mesh_id, tr, nullptr, pt_len, big_koff, jobs), "null"));
  }

  // ---- spread the chunks or loop over them ---------------------------------------------------------------------------------------
  WnPlan P;
  CHECK(wn_plan(32, 98, 24896, 98, 0, P).empty());  // one clip's PD call against 100 352 faces: few groups, many chunks -> spread
  CHECK(P.spread && P.groups == 98 * 98 && P.jobs_bytes == 32 * 144 && P.partial_off == P.jobs_bytes && P.bytes == P.jobs_bytes + 24896LL * 98 * 8);
  CHECK(wn_plan(32, 98, 24896, 1, 0, P).empty() && !P.spread && P.groups == 98 && P.bytes == P.jobs_bytes);  // one chunk: nothing to spread
  CHECK(wn_plan(1, 1023, 1023 * 256, 2, 0, P).empty() && P.spread && P.groups == 2046);
  CHECK(wn_plan(1, 1024, 1024 * 256, 2, 0, P).empty() && !P.spread && P.groups == 1024);  // enough groups from the points alone
  CHECK(wn_plan(1, 1000, 256000, 200, 0, P).empty() && !P.spread);  // 409.6 MB of partials: above the limit
  CHECK(wn_plan(1, 1000, 256000, 200, WN_FORCE_SPREAD, P).empty() && P.spread && P.bytes == P.jobs_bytes + 256000LL * 200 * 8);
  CHECK(wn_plan(32, 98, 24896, 98, WN_FORCE_LOOP, P).empty() && !P.spread && P.groups == 98 && P.bytes == P.jobs_bytes);
  CHECK(wn_plan(32, 98, 24896, 1, WN_FORCE_SPREAD, P).empty() && P.spread && P.groups == 98 && P.bytes == P.jobs_bytes + 24896LL * 8);
  CHECK(wn_plan(3, 0, 0, 1, 0, P).empty() && !P.spread && P.groups == 0);  // every slice empty
  CHECK(wn_plan(3, 0, 0, 1, WN_FORCE_SPREAD, P).empty() && !P.spread && P.groups == 0);
  CHECK(has(wn_plan(1, 1LL << 20, 1LL << 28, 65536, WN_FORCE_SPREAD, P), "too large for one launch"));
  CHECK(wn_plan(1, 1LL << 20, 1LL << 28, 65536, 0, P).empty() && !P.spread);
  CHECK(has(wn_plan(1, 1, 1, 1, 4, P), "unknown flags") && has(wn_plan(1, 1, 1, 1, 3, P), "both routes") && has(wn_plan(0, 1, 1, 1, 0, P), "J = 0"));
  CHECK(wn_align16(0) == 0 && wn_align16(1) == 16 && wn_align16(16) == 16 && wn_align16(17) == 32);

  if (failures) {
    std::printf("%d host checks failed\n", failures);
    return 1;
  }
  std::printf("host check ok\n");
  return 0;
}
