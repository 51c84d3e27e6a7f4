// The host code of libtamf_sdfgrid.so by itself: csrc/tamf_sdfgrid_host.h has no HIP in it, so its argument checks and its launch
// geometry run on any CPU.  tests/test_sdfgrid_cpu.py builds and runs this plainly; built with -fsanitize=address,undefined it is the
// sanitizer run of the library's host side (no GPU, nothing loaded into another process).
//
//   c++ -std=c++17 -fsanitize=address,undefined -I oakink2-tamf_amd/csrc -o sdfgrid_host_check tools/sdfgrid_host_check.cpp && ./sdfgrid_host_check
#include <cstdio>
#include <cstdlib>

#include "tamf_sdfgrid_host.h"

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
  // accepted shapes, the edges included
  CHECK(sg_bad_shape(1, 1, 1, 1, 1).empty());
  CHECK(sg_bad_shape(3, 64, 160, 778, 2).empty());
  CHECK(sg_bad_shape(1, 65535, 1, 1, 1).empty() && sg_bad_shape(1, 1, 1, 1, 65535).empty() && sg_bad_shape(7, 255, 3, 5, 257).empty());
  CHECK(sg_bad_shape(1, 1, 0x7fffffff, 1, 1).empty() && sg_bad_shape(1, 1, 1, 0x7fffffff, 1).empty());
  // refusals of the shape
  CHECK(has(sg_bad_shape(0, 1, 1, 1, 1), "grid set is empty"));
  CHECK(has(sg_bad_shape(-1, 1, 1, 1, 1), "grid set is empty"));
  CHECK(has(sg_bad_shape(1, 0, 1, 1, 1), "at least 1") && has(sg_bad_shape(1, 1, 0, 1, 1), "at least 1"));
  CHECK(has(sg_bad_shape(1, 1, 1, 0, 1), "at least 1") && has(sg_bad_shape(1, 1, 1, 1, 0), "at least 1") && has(sg_bad_shape(1, -4, 1, 1, 1), "B = -4"));
  CHECK(has(sg_bad_shape(1, 65536, 1, 1, 1), "B * nobj above 65535") && has(sg_bad_shape(1, 256, 1, 1, 256), "split the batch"));
  CHECK(has(sg_bad_shape(1, 0x7fffffff, 1, 1, 0x7fffffff), "B * nobj"));  // (the product is taken in 64 bits)
  CHECK(has(sg_bad_shape(1, 1, 65536, 32768, 1), "T * V above") && has(sg_bad_shape(1, 1, 0x7fffffff, 0x7fffffff, 1), "T * V above"));
  // refusals of the pointers: every mandatory one by itself
  int x = 0;
  const void* p = &x;
  CHECK(sg_bad_pointers(p, p, p, p, p, p, p, p, p, "depth_out").empty());
  for (int k = 0; k < 9; ++k) {
    const void* a[9] = {p, p, p, p, p, p, p, p, p};
    a[k] = nullptr;
    const std::string msg = sg_bad_pointers(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], "g_hand_out");
    CHECK(has(msg, "null argument"));
    CHECK(has(msg, k < 5 ? "grid set" : k < 8 ? "hand_verts, obj_traj and grid_id" : "g_hand_out"));
  }
  // the launch geometry: fc frames per work group, fc * min(poses per frame, SG_POSES) <= SG_POSES, the chunks cover T
  for (int T : {1, 2, 7, 8, 9, 160, 1000})
    for (int per : {1, 2, 7, 8, 9, 33, 64, 65, 4000}) {
      int32_t fc = -1, nchunks = -1;
      sg_chunks(T, per, fc, nchunks);
      const int kept = per > SG_POSES ? SG_POSES : per;
      CHECK(fc >= 1 && fc <= SG_FC && fc <= T && fc * kept <= SG_POSES);
      CHECK((long long)nchunks * fc >= T && (long long)(nchunks - 1) * fc < T);
    }
  int32_t fc, nchunks;
  sg_chunks(160, 1, fc, nchunks);
  CHECK(fc == 8 && nchunks == 20);
  sg_chunks(160, 2, fc, nchunks);
  CHECK(fc == 8 && nchunks == 20);
  sg_chunks(3, 16, fc, nchunks);
  CHECK(fc == 3 && nchunks == 1);
  sg_chunks(160, 66, fc, nchunks);
  CHECK(fc == 1 && nchunks == 160);
  sg_chunks(5, 0, fc, nchunks);  // (never asked for: treated as one pose per frame)
  CHECK(fc == 5 && nchunks == 1);

  if (failures) {
    std::printf("%d host checks failed\n", failures);
    return 1;
  }
  std::printf("host check ok\n");
  return 0;
}
