// tamf_raster.h - the kernels of libtamf_render.so (include/tamf_render.h holds the definition they implement): projection to
// 1/256-pixel fixed point, the tiled triangle / point-splat rasteriser with its depth test, and the shading passes.
//
// Rasteriser layout: grid (tiles across, tiles down, frames), one workgroup of 256 threads per 16 x 16-pixel tile and frame, one
// pixel per thread.  Primitives are taken in ascending chunks of 256: every thread sets one primitive up and tests its bounding
// box against the tile, the survivors are compacted IN ORDER into LDS (64-bit wave ballot + a prefix over the four waves), and
// every pixel then walks the list front to back with a strict `<` depth test.  So within a call the lowest index wins an exact
// tie, and against what the buffers held the earlier call wins - without atomics, one writer per pixel.  A frame's pixels depend on
// that frame's inputs only.
//
// Coverage is exact: the edge functions are int64 in 1/256-pixel units, evaluated once per triangle at the tile's first pixel
// centre and stepped across the tile by whole pixels (A * 256 dx + B * 256 dy, one v_mad_i64_i32 each).  |coordinate| <= 2^28
// (tamf_render_project's validity bound) keeps differences inside int32 and the edge functions inside int64 (< 2^59).
//
// Depth peeling: the rasteriser and the splatter take a template parameter FLOOR.  The FLOOR instantiation reads a floor (depth, id)
// per pixel and admits only candidates that come strictly after it in the order (depth, id); everything else, the depth expression
// included, is the one body, so a fragment's depth has the same bits in every pass.  The plain instantiation compiles to the code it
// was before the parameter existed.  The colour passes are template parameters of the shading kernels in the same way.  Composite and
// resolve are one thread per output pixel; the number of layers, items and sub-samples are host values: no loop runs on device data.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr int RS_TILE = 16;                  // pixels per tile side
constexpr int RS_NT = RS_TILE * RS_TILE;     // threads per workgroup = pixels per tile = primitives per chunk
constexpr int RS_SUB = 256;                  // fixed-point units per pixel
constexpr int RS_INVALID = INT32_MIN;        // both xy coordinates of an invalid vertex
constexpr float RS_XY_LIMIT = 268435456.0f;  // 2^28
constexpr int RS_MAX_LIGHTS = 8;

struct RsCamera {
  float view[12];  // (3,4) row-major, world -> camera
  float fx, fy, cx, cy, near;
};

struct RsLights {
  float dir[RS_MAX_LIGHTS][3];  // unit, camera frame: the direction the light travels
  float strength[RS_MAX_LIGHTS];
  float ambient;
  int n;
};

// ---- projection -------------------------------------------------------------------------------------------------------------
// one thread per (frame, vertex)
__global__ void __launch_bounds__(256) render_project_kernel(const float* __restrict__ verts, const float* __restrict__ model, RsCamera cam,
                                                             int F, int V, int per_frame, float* __restrict__ pos_cam, int* __restrict__ xy) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)F * V) return;
  const int f = (int)(i / V), v = (int)(i - (long)f * V);
  const float* p = verts + ((per_frame ? (long)f * V : 0L) + v) * 3;
  float x = p[0], y = p[1], z = p[2];
  if (model) {
    const float* m = model + (long)f * 12;
    const float wx = m[0] * x + m[1] * y + m[2] * z + m[3];
    const float wy = m[4] * x + m[5] * y + m[6] * z + m[7];
    const float wz = m[8] * x + m[9] * y + m[10] * z + m[11];
    x = wx, y = wy, z = wz;
  }
  const float cx_ = cam.view[0] * x + cam.view[1] * y + cam.view[2] * z + cam.view[3];
  const float cy_ = cam.view[4] * x + cam.view[5] * y + cam.view[6] * z + cam.view[7];
  const float cz_ = cam.view[8] * x + cam.view[9] * y + cam.view[10] * z + cam.view[11];
  pos_cam[i * 3 + 0] = cx_;
  pos_cam[i * 3 + 1] = cy_;
  pos_cam[i * 3 + 2] = cz_;
  int sx = RS_INVALID, sy = RS_INVALID;
  if (isfinite(cx_) && isfinite(cy_) && isfinite(cz_) && cz_ >= cam.near) {
    const float u = rintf((cam.fx * cx_ / cz_ + cam.cx) * (float)RS_SUB);  // round half to even
    const float w = rintf((cam.fy * cy_ / cz_ + cam.cy) * (float)RS_SUB);
    if (fabsf(u) <= RS_XY_LIMIT && fabsf(w) <= RS_XY_LIMIT) {  // (false for NaN)
      sx = (int)u;
      sy = (int)w;
    }
  }
  xy[i * 2 + 0] = sx;
  xy[i * 2 + 1] = sy;
}

// ---- clear / fill -----------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) render_clear_kernel(float* __restrict__ depth, int* __restrict__ prim_id, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  depth[i] = __builtin_inff();
  prim_id[i] = -1;
}

__global__ void __launch_bounds__(256) render_fill_kernel(const int* __restrict__ prim_id, unsigned char* __restrict__ rgb, long n, int r, int g, int b) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || prim_id[i] != -1) return;
  rgb[i * 3 + 0] = (unsigned char)r;
  rgb[i * 3 + 1] = (unsigned char)g;
  rgb[i * 3 + 2] = (unsigned char)b;
}

// ---- what the rasteriser and the shader share: a triangle's oriented setup ------------------------------------------------------
struct RsTri {
  int x[3], y[3];   // snapped, vertices 1 and 2 swapped when the doubled area was negative
  int v[3];         // their vertex indices, in that order
  long long area2;  // > 0 when ok
  bool ok;
};

// faces row t of frame f; not ok: an index outside [0, V), an invalid vertex, zero area
__device__ inline RsTri rs_setup(const int* __restrict__ xy_f, const int* __restrict__ faces, int t, int V) {
  RsTri r;
  r.ok = false;
  r.area2 = 0;
  for (int k = 0; k < 3; ++k) r.v[k] = faces[(long)t * 3 + k];
  if ((unsigned)r.v[0] >= (unsigned)V || (unsigned)r.v[1] >= (unsigned)V || (unsigned)r.v[2] >= (unsigned)V) return r;
  for (int k = 0; k < 3; ++k) {
    r.x[k] = xy_f[(long)r.v[k] * 2 + 0];
    r.y[k] = xy_f[(long)r.v[k] * 2 + 1];
  }
  if (r.x[0] == RS_INVALID || r.x[1] == RS_INVALID || r.x[2] == RS_INVALID) return r;
  long long a2 = (long long)(r.x[1] - r.x[0]) * (r.y[2] - r.y[0]) - (long long)(r.y[1] - r.y[0]) * (r.x[2] - r.x[0]);
  if (a2 == 0) return r;
  if (a2 < 0) {
    int s;
    s = r.x[1], r.x[1] = r.x[2], r.x[2] = s;
    s = r.y[1], r.y[1] = r.y[2], r.y[2] = s;
    s = r.v[1], r.v[1] = r.v[2], r.v[2] = s;
    a2 = -a2;
  }
  r.area2 = a2;
  r.ok = true;
  return r;
}

// edge k is the one OPPOSITE vertex k: from a = vertex k+1 to b = vertex k+2.  E = A px + B py + C.
__device__ inline void rs_edge(const RsTri& r, int k, int& A, int& B, long long& C) {
  const int a = (k + 1) % 3, b = (k + 2) % 3;
  A = r.y[a] - r.y[b];
  B = r.x[b] - r.x[a];
  C = (long long)r.x[a] * r.y[b] - (long long)r.y[a] * r.x[b];
}

// the top-left rule: 1 when a centre ON the edge belongs to the triangle
__device__ inline int rs_owns_zero(int A, int B) { return (A > 0 || (A == 0 && B < 0)) ? 1 : 0; }

// order-preserving compaction of the workgroup's `keep` flags: -> this thread's slot (valid when keep) and the total in *total.
// wave_count: LDS int[RS_NT / 64].  Ends with a barrier; the caller's next barrier protects wave_count's reuse.
__device__ inline int rs_compact(bool keep, int* wave_count, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long mask = __ballot(keep);
  if (lane == 0) wave_count[wave] = __popcll(mask);
  __syncthreads();
  int base = 0, sum = 0;
  for (int w = 0; w < RS_NT / 64; ++w) {
    const int c = wave_count[w];
    if (w < wave) base += c;
    sum += c;
  }
  *total = sum;
  return base + __popcll(mask & ((1ull << lane) - 1ull));
}

// ---- triangles --------------------------------------------------------------------------------------------------------------
struct RsTriSlot {
  long long e[3];  // edge functions at the tile's first pixel centre
  int a[3], b[3];  // their x / y steps per 1/256 pixel
  float q[3];      // (1 / z_k) / area2: inv_z = sum_k E_k q_k
  int own;         // bit k: edge k owns E == 0
  int index;       // triangle index
};

// FLOOR: admit a candidate only where floor_id >= 0 and (d, id) comes strictly after (floor_depth, floor_id); both null otherwise
template <bool FLOOR>
__global__ void __launch_bounds__(RS_NT) render_raster_kernel(const int* __restrict__ xy, const float* __restrict__ pos_cam,
                                                             const int* __restrict__ faces, int Nf, int V, int W, int H, int prim_base,
                                                             float* __restrict__ depth, int* __restrict__ prim_id,
                                                             const float* __restrict__ floor_depth, const int* __restrict__ floor_id) {
  __shared__ RsTriSlot slot[RS_NT];
  __shared__ int wave_count[RS_NT / 64];
  const int f = blockIdx.z;
  const int tx0 = blockIdx.x * RS_TILE, ty0 = blockIdx.y * RS_TILE;
  const int dx = threadIdx.x % RS_TILE, dy = threadIdx.x / RS_TILE;
  const int px = tx0 + dx, py = ty0 + dy;
  bool live = px < W && py < H;
  const long pix = ((long)f * H + py) * W + px;
  const int* xy_f = xy + (long)f * V * 2;
  const float* pos_f = pos_cam + (long)f * V * 3;
  float fd = 0.0f;
  int fid = -1;
  if constexpr (FLOOR) {
    if (live) fd = floor_depth[pix], fid = floor_id[pix];
    live = live && fid >= 0;  // nothing lies behind a pixel whose previous layer is empty
  }
  // the tile's pixel centres in fixed point (clipped to the image: the overhang holds no pixel)
  const int cx0 = tx0 * RS_SUB + RS_SUB / 2, cy0 = ty0 * RS_SUB + RS_SUB / 2;
  const int cx1 = (min(tx0 + RS_TILE, W) - 1) * RS_SUB + RS_SUB / 2, cy1 = (min(ty0 + RS_TILE, H) - 1) * RS_SUB + RS_SUB / 2;
  float best = __builtin_inff();
  int best_id = -1;
  if (live) best = depth[pix], best_id = prim_id[pix];
  const float first = best;
  const int first_id = best_id;
  const int sx = dx * RS_SUB, sy = dy * RS_SUB;

  for (int c0 = 0; c0 < Nf; c0 += RS_NT) {
    const int t = c0 + threadIdx.x;
    RsTri tri;
    tri.ok = false;
    if (t < Nf) tri = rs_setup(xy_f, faces, t, V);
    bool keep = tri.ok;
    if (keep) {
      const int x_lo = min(tri.x[0], min(tri.x[1], tri.x[2])), x_hi = max(tri.x[0], max(tri.x[1], tri.x[2]));
      const int y_lo = min(tri.y[0], min(tri.y[1], tri.y[2])), y_hi = max(tri.y[0], max(tri.y[1], tri.y[2]));
      keep = x_hi >= cx0 && x_lo <= cx1 && y_hi >= cy0 && y_lo <= cy1;
    }
    int n;
    const int at = rs_compact(keep, wave_count, &n);
    if (keep) {
      RsTriSlot s;
      const float area = (float)tri.area2;
      s.own = 0;
      for (int k = 0; k < 3; ++k) {
        long long C;
        rs_edge(tri, k, s.a[k], s.b[k], C);
        s.e[k] = (long long)s.a[k] * cx0 + (long long)s.b[k] * cy0 + C;
        s.own |= rs_owns_zero(s.a[k], s.b[k]) << k;
        s.q[k] = (1.0f / pos_f[(long)tri.v[k] * 3 + 2]) / area;
      }
      s.index = t;
      slot[at] = s;
    }
    __syncthreads();
    if (live) {
      for (int i = 0; i < n; ++i) {
        const RsTriSlot& s = slot[i];
        const long long e0 = s.e[0] + (long long)s.a[0] * sx + (long long)s.b[0] * sy;
        if (e0 < 0 || (e0 == 0 && !(s.own & 1))) continue;
        const long long e1 = s.e[1] + (long long)s.a[1] * sx + (long long)s.b[1] * sy;
        if (e1 < 0 || (e1 == 0 && !(s.own & 2))) continue;
        const long long e2 = s.e[2] + (long long)s.a[2] * sx + (long long)s.b[2] * sy;
        if (e2 < 0 || (e2 == 0 && !(s.own & 4))) continue;
        const float inv_z = (float)e0 * s.q[0] + (float)e1 * s.q[1] + (float)e2 * s.q[2];
        const float d = 1.0f / inv_z;
        if constexpr (FLOOR) {
          if (!(d > fd || (d == fd && prim_base + s.index > fid))) continue;
        }
        if (d < best) best = d, best_id = prim_base + s.index;
      }
    }
    __syncthreads();
  }
  if (live && (best_id != first_id || best != first)) depth[pix] = best, prim_id[pix] = best_id;
}

// ---- point splats -----------------------------------------------------------------------------------------------------------
struct RsPointSlot {
  int px, py;  // the pixel that holds the projection
  float z;
  int index;
};

template <bool FLOOR>
__global__ void __launch_bounds__(RS_NT) render_points_kernel(const int* __restrict__ xy, const float* __restrict__ pos_cam, int P, int W, int H,
                                                             int half, int prim_base, float* __restrict__ depth, int* __restrict__ prim_id,
                                                             const float* __restrict__ floor_depth, const int* __restrict__ floor_id) {
  __shared__ RsPointSlot slot[RS_NT];
  __shared__ int wave_count[RS_NT / 64];
  const int f = blockIdx.z;
  const int tx0 = blockIdx.x * RS_TILE, ty0 = blockIdx.y * RS_TILE;
  const int px = tx0 + threadIdx.x % RS_TILE, py = ty0 + threadIdx.x / RS_TILE;
  bool live = px < W && py < H;
  const long pix = ((long)f * H + py) * W + px;
  const int* xy_f = xy + (long)f * P * 2;
  const float* pos_f = pos_cam + (long)f * P * 3;
  float fd = 0.0f;
  int fid = -1;
  if constexpr (FLOOR) {
    if (live) fd = floor_depth[pix], fid = floor_id[pix];
    live = live && fid >= 0;
  }
  const int tx1 = min(tx0 + RS_TILE, W) - 1, ty1 = min(ty0 + RS_TILE, H) - 1;
  float best = __builtin_inff();
  int best_id = -1;
  if (live) best = depth[pix], best_id = prim_id[pix];
  const float first = best;
  const int first_id = best_id;

  for (int c0 = 0; c0 < P; c0 += RS_NT) {
    const int t = c0 + threadIdx.x;
    bool keep = false;
    int qx = 0, qy = 0;
    if (t < P) {
      const int x = xy_f[(long)t * 2], y = xy_f[(long)t * 2 + 1];
      if (x != RS_INVALID) {
        qx = x >> 8, qy = y >> 8;  // floor(xy / 256): |x| <= 2^28, so qx +- half cannot overflow
        keep = qx + half >= tx0 && qx - half <= tx1 && qy + half >= ty0 && qy - half <= ty1;
      }
    }
    int n;
    const int at = rs_compact(keep, wave_count, &n);
    if (keep) {
      RsPointSlot s;
      s.px = qx, s.py = qy, s.z = pos_f[(long)t * 3 + 2], s.index = t;
      slot[at] = s;
    }
    __syncthreads();
    if (live) {
      for (int i = 0; i < n; ++i) {
        const RsPointSlot& s = slot[i];
        if (abs(px - s.px) > half || abs(py - s.py) > half) continue;
        if constexpr (FLOOR) {
          if (!(s.z > fd || (s.z == fd && prim_base + s.index > fid))) continue;
        }
        if (s.z < best) best = s.z, best_id = prim_base + s.index;
      }
    }
    __syncthreads();
  }
  if (live && (best_id != first_id || best != first)) depth[pix] = best, prim_id[pix] = best_id;
}

// ---- shading ----------------------------------------------------------------------------------------------------------------
__device__ inline unsigned char rs_byte(float base, float I) {
  const float c = fminf(fmaxf(base * I, 0.0f), 1.0f);
  return (unsigned char)floorf(255.0f * c + 0.5f);
}

// one thread per pixel of (F, H, W); writes only where prim_id lies in [prim_base, prim_base + Nf).  COLORS: the base colour is the
// blend of vertex_rgb (V,3), or (F,V,3) when col_per_frame, by the weights of the normals, taken as c_0 + w_1 (c_1 - c_0) + w_2 (c_2 - c_0):
// three equal colours give exactly that colour, and so the bytes of the constant-colour pass.
template <bool COLORS>
__global__ void __launch_bounds__(256) render_shade_mesh_kernel(const int* __restrict__ prim_id, const int* __restrict__ xy, const float* __restrict__ pos_cam,
                                                                const float* __restrict__ normals, const int* __restrict__ faces, int Nf, int V, int F,
                                                                int W, int H, int prim_base, float br, float bg, float bb, RsLights L,
                                                                unsigned char* __restrict__ rgb, const float* __restrict__ vertex_rgb, int col_per_frame) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)F * H * W) return;
  const int id = prim_id[i];
  if (id < prim_base || id - prim_base >= Nf) return;
  const int px = (int)(i % W), py = (int)((i / W) % H), f = (int)(i / ((long)W * H));
  const RsTri tri = rs_setup(xy + (long)f * V * 2, faces, id - prim_base, V);
  if (!tri.ok) return;  // (an id the rasteriser cannot have written for these inputs)
  const float* pos_f = pos_cam + (long)f * V * 3;
  const int cx = px * RS_SUB + RS_SUB / 2, cy = py * RS_SUB + RS_SUB / 2;
  float w[3], wsum = 0.0f, p[3][3];
  for (int k = 0; k < 3; ++k) {
    int A, B;
    long long C;
    rs_edge(tri, k, A, B, C);
    const long long e = (long long)A * cx + (long long)B * cy + C;
    for (int c = 0; c < 3; ++c) p[k][c] = pos_f[(long)tri.v[k] * 3 + c];
    w[k] = (float)e / p[k][2];
    wsum += w[k];
  }
  for (int k = 0; k < 3; ++k) w[k] /= wsum;
  float n[3], at[3];
  for (int c = 0; c < 3; ++c) at[c] = w[0] * p[0][c] + w[1] * p[1][c] + w[2] * p[2][c];
  if (normals) {
    const float* nf = normals + (long)f * V * 3;
    for (int c = 0; c < 3; ++c) n[c] = w[0] * nf[(long)tri.v[0] * 3 + c] + w[1] * nf[(long)tri.v[1] * 3 + c] + w[2] * nf[(long)tri.v[2] * 3 + c];
  } else {
    const float ux = p[1][0] - p[0][0], uy = p[1][1] - p[0][1], uz = p[1][2] - p[0][2];
    const float vx = p[2][0] - p[0][0], vy = p[2][1] - p[0][1], vz = p[2][2] - p[0][2];
    n[0] = uy * vz - uz * vy, n[1] = uz * vx - ux * vz, n[2] = ux * vy - uy * vx;
  }
  const float len = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  float I = L.ambient;
  if (len > 0.0f) {  // (a zero normal is lit by the ambient term alone)
    const float s = (n[0] * at[0] + n[1] * at[1] + n[2] * at[2] > 0.0f ? -1.0f : 1.0f) / len;  // towards the viewer
    for (int c = 0; c < 3; ++c) n[c] *= s;
    for (int l = 0; l < L.n; ++l) I += L.strength[l] * fmaxf(0.0f, -(n[0] * L.dir[l][0] + n[1] * L.dir[l][1] + n[2] * L.dir[l][2]));
  }
  if constexpr (COLORS) {
    const float* cf = vertex_rgb + (col_per_frame ? (long)f * V * 3 : 0L);
    const float* c0 = cf + (long)tri.v[0] * 3;
    const float* c1 = cf + (long)tri.v[1] * 3;
    const float* c2 = cf + (long)tri.v[2] * 3;
    br = c0[0] + w[1] * (c1[0] - c0[0]) + w[2] * (c2[0] - c0[0]);
    bg = c0[1] + w[1] * (c1[1] - c0[1]) + w[2] * (c2[1] - c0[1]);
    bb = c0[2] + w[1] * (c1[2] - c0[2]) + w[2] * (c2[2] - c0[2]);
  }
  rgb[i * 3 + 0] = rs_byte(br, I);
  rgb[i * 3 + 1] = rs_byte(bg, I);
  rgb[i * 3 + 2] = rs_byte(bb, I);
}

// COLORS: the pixel's own point's colour, point_rgb (P,3), or (F,P,3) when col_per_frame (frame_pixels = H * W), unlit
template <bool COLORS>
__global__ void __launch_bounds__(256) render_shade_points_kernel(const int* __restrict__ prim_id, long n, int prim_base, int P, int r, int g, int b,
                                                                  unsigned char* __restrict__ rgb, const float* __restrict__ point_rgb, int col_per_frame,
                                                                  long frame_pixels) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int id = prim_id[i];
  if (id < prim_base || id - prim_base >= P) return;
  if constexpr (COLORS) {
    const float* c = point_rgb + ((col_per_frame ? (i / frame_pixels) * P : 0L) + (id - prim_base)) * 3;
    rgb[i * 3 + 0] = rs_byte(c[0], 1.0f);
    rgb[i * 3 + 1] = rs_byte(c[1], 1.0f);
    rgb[i * 3 + 2] = rs_byte(c[2], 1.0f);
    return;
  }
  rgb[i * 3 + 0] = (unsigned char)r;
  rgb[i * 3 + 1] = (unsigned char)g;
  rgb[i * 3 + 2] = (unsigned char)b;
}

// ---- composite and resolve ---------------------------------------------------------------------------------------------------
constexpr int RS_MAX_ITEMS = 64;
constexpr int RS_MAX_LAYERS = 8;

struct RsItems {
  int base[RS_MAX_ITEMS], count[RS_MAX_ITEMS];
  float alpha[RS_MAX_ITEMS];
  int n;
};

// one thread per pixel of (F, H, W): C = bg, then the K layers back to front, C = a byte / 255 + (1 - a) C where the layer's id belongs
// to an item of alpha a; a layer whose id is negative or belongs to no item leaves C as it is.  n = F * H * W.
__global__ void __launch_bounds__(256) render_composite_kernel(const unsigned char* __restrict__ layer_rgb, const int* __restrict__ layer_id, int K, long n,
                                                               RsItems items, float bg_r, float bg_g, float bg_b, unsigned char* __restrict__ rgb) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float c[3] = {bg_r, bg_g, bg_b};
  for (int k = K - 1; k >= 0; --k) {
    const int id = layer_id[(long)k * n + i];
    float a = 0.0f;
    bool hit = false;
    for (int j = 0; j < items.n; ++j)
      if (id >= items.base[j] && id - items.base[j] < items.count[j]) a = items.alpha[j], hit = true;
    if (!hit) continue;
    const unsigned char* p = layer_rgb + ((long)k * n + i) * 3;
    for (int ch = 0; ch < 3; ++ch) c[ch] = a * ((float)p[ch] / 255.0f) + (1.0f - a) * c[ch];
  }
  for (int ch = 0; ch < 3; ++ch) rgb[i * 3 + ch] = rs_byte(c[ch], 1.0f);
}

// one thread per output pixel of (F, H, W): the rounded mean of its s x s block of in (F, s H, s W, 3), in integers
__global__ void __launch_bounds__(256) render_resolve_kernel(const unsigned char* __restrict__ in, int F, int H, int W, int s, unsigned char* __restrict__ out) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)F * H * W) return;
  const int px = (int)(i % W), py = (int)((i / W) % H);
  const long f = i / ((long)W * H);
  const long row = (long)s * W * 3;
  const unsigned char* p = in + (f * s * H + (long)py * s) * row + (long)px * s * 3;
  int sum[3] = {0, 0, 0};
  for (int y = 0; y < s; ++y)
    for (int x = 0; x < s; ++x)
      for (int ch = 0; ch < 3; ++ch) sum[ch] += p[y * row + x * 3 + ch];
  const int nn = s * s;
  for (int ch = 0; ch < 3; ++ch) out[i * 3 + ch] = (unsigned char)((sum[ch] + nn / 2) / nn);
}
