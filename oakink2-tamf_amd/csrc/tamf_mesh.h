// The triangle record of the point-in-closed-mesh test (dev_fn/external/libmesh/inside_mesh.py:8-149) and the kernel that prepares it:
// shared by mesh_contains_kernel (tamf_geom.h, libtamf_hip.so) and the lattice / batched kernels of tamf_voxel.h (libtamf_eval.so).
// Per triangle (rescaled to the hash-grid frame) 16 doubles: t3.xy, the 2D edge matrix a00 a01 a10 a11, sign/abs of its determinant,
// the normal's x, y, sign/abs of its z, t1.xy and t1.z * |n_z|.  float64, the reference's operation order, no fused multiply-adds.
#pragma once
#include "tamf_device.h"

constexpr int MESH_TC = 16;
// the record of one rescaled triangle t[corner][xyz]: one set of expressions for every kernel that prepares records
TAMF_DEV void mesh_record(const double (&t)[3][3], double* __restrict__ o) {
#pragma clang fp contract(off)
  const double a00 = t[0][0] - t[2][0], a01 = t[1][0] - t[2][0], a10 = t[0][1] - t[2][1], a11 = t[1][1] - t[2][1];
  const double det = a00 * a11 - a01 * a10;
  const double v1x = t[2][0] - t[0][0], v1y = t[2][1] - t[0][1], v1z = t[2][2] - t[0][2];
  const double v2x = t[1][0] - t[0][0], v2y = t[1][1] - t[0][1], v2z = t[1][2] - t[0][2];
  const double nx = v1y * v2z - v1z * v2y, ny = v1z * v2x - v1x * v2z, nz = v1x * v2y - v1y * v2x;
  const double an = fabs(nz), sn = nz > 0.0 ? 1.0 : (nz < 0.0 ? -1.0 : 0.0);
  o[0] = t[2][0]; o[1] = t[2][1];
  o[2] = a00; o[3] = a01; o[4] = a10; o[5] = a11;
  o[6] = det > 0.0 ? 1.0 : (det < 0.0 ? -1.0 : 0.0);
  o[7] = fabs(det);
  o[8] = nx; o[9] = ny; o[10] = sn; o[11] = an;
  o[12] = t[0][0]; o[13] = t[0][1];
  o[14] = t[0][2] * an;
  o[15] = 0.0;
}

__global__ void mesh_prepare_kernel(const double* __restrict__ verts, const int* __restrict__ faces, int F, double sx, double sy,
                                    double sz, double tx, double ty, double tz, double* __restrict__ tc) {
#pragma clang fp contract(off)
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= F) return;
  double t[3][3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double* v = verts + (long)faces[f * 3 + k] * 3;
    t[k][0] = sx * v[0] + tx;
    t[k][1] = sy * v[1] + ty;
    t[k][2] = sz * v[2] + tz;
  }
  mesh_record(t, tc + (long)f * MESH_TC);
}
