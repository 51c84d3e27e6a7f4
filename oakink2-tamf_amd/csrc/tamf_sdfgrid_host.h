// Host side of libtamf_sdfgrid.so without a line of HIP: the argument checks and the launch geometry.  tamf_sdfgrid.hip launches what is
// decided here; a plain C++ program can call these functions by themselves (a sanitizer build of the host code needs no GPU).
#pragma once
#include <stdint.h>

#include <string>

constexpr int SG_NT = 256;           // threads of a work group
constexpr int SG_FC = 8;             // frames of a work group, at most
constexpr int SG_POSES = 64;         // poses a work group keeps in LDS (12 doubles each)
constexpr long long SG_GRID_Y = 65535;
constexpr int SG_MIN_RES = 2, SG_MAX_RES = 512;  // TAMF_SDFGRID_MIN_RES / _MAX_RES

// the limits of include/tamf_sdfgrid.h on the shape; "" when it is accepted
static inline std::string sg_bad_shape(int32_t G, int32_t B, int32_t T, int32_t V, int32_t nobj) {
  const std::string dims = "G = " + std::to_string(G) + ", B = " + std::to_string(B) + ", T = " + std::to_string(T) + ", V = " + std::to_string(V) +
                           ", nobj = " + std::to_string(nobj);
  if (G < 1) return "the grid set is empty (" + dims + ")";
  if (B < 1 || T < 1 || V < 1 || nobj < 1) return "B, T, V and nobj must be at least 1 (" + dims + ")";
  if ((long long)B * nobj > SG_GRID_Y) return "B * nobj above " + std::to_string(SG_GRID_Y) + ": split the batch (" + dims + ")";
  if ((long long)T * V > 0x7fffffffLL) return "T * V above 2^31 - 1: split the clip (" + dims + ")";
  return "";
}

// "" or the names of the mandatory pointers when one of them is null
static inline std::string sg_bad_pointers(const void* values, const void* grid_off, const void* res, const void* origin, const void* step,
                                          const void* hand, const void* traj, const void* grid_id, const void* out, const char* out_name) {
  if (!values || !grid_off || !res || !origin || !step) return "null argument: the grid set needs values, grid_off, res, origin and step";
  if (!hand || !traj || !grid_id) return "null argument: hand_verts, obj_traj and grid_id are required";
  if (!out) return std::string("null argument: ") + out_name + " is required";
  return "";
}

// frames per work group and the number of frame chunks.  The forward owns one object per work group and keeps a pose per frame; the
// backward owns a clip and keeps the poses of min(nobj, SG_POSES) objects per frame (an object beyond them has its pose computed per
// vertex), so its chunk shrinks as nobj grows.
static inline void sg_chunks(int32_t T, int32_t poses_per_frame, int32_t& fc, int32_t& nchunks) {
  int per = poses_per_frame < 1 ? 1 : (poses_per_frame > SG_POSES ? SG_POSES : poses_per_frame);
  fc = SG_POSES / per;
  if (fc > SG_FC) fc = SG_FC;
  if (fc > T) fc = T;
  if (fc < 1) fc = 1;
  nchunks = (T + fc - 1) / fc;
}
