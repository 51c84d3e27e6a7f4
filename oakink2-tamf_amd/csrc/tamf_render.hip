// libtamf_render.so: the C-ABI of include/tamf_render.h - the offscreen renderer.  One translation unit.
#include "../../include/tamf_render.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "tamf_raster.h"

static_assert(TAMF_RENDER_MAX_LIGHTS == RS_MAX_LIGHTS, "the header's light count is the kernels'");
static_assert(TAMF_RENDER_MAX_ITEMS == RS_MAX_ITEMS && TAMF_RENDER_MAX_LAYERS == RS_MAX_LAYERS, "the header's composite limits are the kernels'");

static thread_local std::string g_render_error;

static int fail(int code, const std::string& msg) {
  g_render_error = msg;
  return code;
}

extern "C" const char* tamf_render_last_error(void) { return g_render_error.c_str(); }

constexpr long RN_INT_MAX = 2147483647L;

// the limits of include/tamf_render.h on a (F, H, W) buffer; "" when accepted
static std::string bad_image(int F, int H, int W) {
  const std::string dims = "F = " + std::to_string(F) + ", H = " + std::to_string(H) + ", W = " + std::to_string(W);
  if (W < 1 || W > TAMF_RENDER_MAX_SIDE || H < 1 || H > TAMF_RENDER_MAX_SIDE)
    return "W and H must lie in [1, " + std::to_string(TAMF_RENDER_MAX_SIDE) + "] (" + dims + ")";
  if (F < 1 || F > 65535) return "F outside [1, 65535] (" + dims + ")";
  if ((long)F * H * W > RN_INT_MAX) return "F * H * W above 2^31 - 1: split the frames (" + dims + ")";
  return "";
}

// on F frames of n elements (vertices or points) and `count` primitives numbered from prim_base
static std::string bad_prims(int F, int n, int count, int prim_base) {
  const std::string dims = "F = " + std::to_string(F) + ", elements = " + std::to_string(n) + ", primitives = " + std::to_string(count) +
                           ", prim_base = " + std::to_string(prim_base);
  if (n < 1 || count < 1) return "a mesh needs at least one vertex and one face, a cloud one point (" + dims + ")";
  if ((long)F * n > RN_INT_MAX / 3 || count > RN_INT_MAX / 3) return "F * V (or F * P), or the face count, above (2^31 - 1) / 3 (" + dims + ")";
  if (prim_base < 0 || (long)prim_base + count > RN_INT_MAX) return "prim_base < 0 or prim_base + count above 2^31 - 1 (" + dims + ")";
  return "";
}

static int launched() {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(TAMF_ERR_HIP, hipGetErrorString(e));
  return 0;
}

static dim3 tiles(int F, int H, int W) { return dim3((W + RS_TILE - 1) / RS_TILE, (H + RS_TILE - 1) / RS_TILE, F); }
static unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }
static int to_byte(float c) { return (int)std::floor(255.0f * std::fmin(std::fmax(c, 0.0f), 1.0f) + 0.5f); }
static bool finite3(const float* c) { return std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]); }

extern "C" int tamf_render_project(const float* verts, const float* model, const tamf_render_camera* camera, int32_t F, int32_t V,
                                   int32_t per_frame, float* pos_cam, int32_t* xy, void* stream) {
  if (!verts || !camera || !pos_cam || !xy) return fail(TAMF_ERR_INVALID, "null argument: verts, camera, pos_cam_out and xy_out are required");
  if (F < 1 || F > 65535 || V < 1 || (long)F * V > RN_INT_MAX / 3)
    return fail(TAMF_ERR_INVALID, "F outside [1, 65535], V < 1 or F * V above (2^31 - 1) / 3 (F = " + std::to_string(F) + ", V = " + std::to_string(V) + ")");
  RsCamera cam;
  for (int i = 0; i < 12; ++i) {
    if (!std::isfinite(camera->view[i])) return fail(TAMF_ERR_INVALID, "camera: a non-finite view entry");
    cam.view[i] = camera->view[i];
  }
  cam.fx = camera->fx, cam.fy = camera->fy, cam.cx = camera->cx, cam.cy = camera->cy, cam.near = camera->near;
  if (!std::isfinite(cam.fx) || !std::isfinite(cam.fy) || !std::isfinite(cam.cx) || !std::isfinite(cam.cy))
    return fail(TAMF_ERR_INVALID, "camera: non-finite intrinsics");
  if (!(cam.near > 0.0f) || !std::isfinite(cam.near)) return fail(TAMF_ERR_INVALID, "camera: near must be positive and finite");
  hipLaunchKernelGGL(render_project_kernel, dim3(blocks((long)F * V)), dim3(256), 0, (hipStream_t)stream, verts, model, cam, F, V,
                     per_frame ? 1 : 0, pos_cam, (int*)xy);
  return launched();
}

extern "C" int tamf_render_clear(float* depth, int32_t* prim_id, int32_t F, int32_t H, int32_t W, void* stream) {
  if (!depth || !prim_id) return fail(TAMF_ERR_INVALID, "null argument: depth and prim_id are required");
  const std::string bad = bad_image(F, H, W);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  const long n = (long)F * H * W;
  hipLaunchKernelGGL(render_clear_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, depth, (int*)prim_id, n);
  return launched();
}

// floor: both null (the plain pass) or both given (a peel pass)
template <bool FLOOR>
static int raster(const int32_t* xy, const float* pos_cam, const int32_t* faces, int32_t F, int32_t V, int32_t Nf, int32_t H, int32_t W, int32_t prim_base,
                  const float* floor_depth, const int32_t* floor_id, float* depth, int32_t* prim_id, void* stream) {
  if (!xy || !pos_cam || !faces || !depth || !prim_id) return fail(TAMF_ERR_INVALID, "null argument: xy, pos_cam, faces, depth and prim_id are required");
  if (FLOOR && (!floor_depth || !floor_id)) return fail(TAMF_ERR_INVALID, "null argument: floor_depth and floor_id are required");
  if (FLOOR && (floor_depth == depth || floor_id == prim_id)) return fail(TAMF_ERR_INVALID, "the floor buffers must not be the buffers drawn into");
  std::string bad = bad_image(F, H, W);
  if (bad.empty()) bad = bad_prims(F, V, Nf, prim_base);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  hipLaunchKernelGGL(render_raster_kernel<FLOOR>, tiles(F, H, W), dim3(RS_NT), 0, (hipStream_t)stream, (const int*)xy, pos_cam, (const int*)faces, Nf, V,
                     W, H, prim_base, depth, (int*)prim_id, floor_depth, (const int*)floor_id);
  return launched();
}

extern "C" int tamf_render_raster(const int32_t* xy, const float* pos_cam, const int32_t* faces, int32_t F, int32_t V, int32_t Nf, int32_t H,
                                  int32_t W, int32_t prim_base, float* depth, int32_t* prim_id, void* stream) {
  return raster<false>(xy, pos_cam, faces, F, V, Nf, H, W, prim_base, nullptr, nullptr, depth, prim_id, stream);
}

extern "C" int tamf_render_raster_behind(const int32_t* xy, const float* pos_cam, const int32_t* faces, int32_t F, int32_t V, int32_t Nf, int32_t H,
                                         int32_t W, int32_t prim_base, const float* floor_depth, const int32_t* floor_id, float* depth,
                                         int32_t* prim_id, void* stream) {
  return raster<true>(xy, pos_cam, faces, F, V, Nf, H, W, prim_base, floor_depth, floor_id, depth, prim_id, stream);
}

template <bool FLOOR>
static int points(const int32_t* xy, const float* pos_cam, int32_t F, int32_t P, int32_t H, int32_t W, int32_t point_size, int32_t prim_base,
                  const float* floor_depth, const int32_t* floor_id, float* depth, int32_t* prim_id, void* stream) {
  if (!xy || !pos_cam || !depth || !prim_id) return fail(TAMF_ERR_INVALID, "null argument: xy, pos_cam, depth and prim_id are required");
  if (FLOOR && (!floor_depth || !floor_id)) return fail(TAMF_ERR_INVALID, "null argument: floor_depth and floor_id are required");
  if (FLOOR && (floor_depth == depth || floor_id == prim_id)) return fail(TAMF_ERR_INVALID, "the floor buffers must not be the buffers drawn into");
  std::string bad = bad_image(F, H, W);
  if (bad.empty()) bad = bad_prims(F, P, P, prim_base);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  if (point_size < 1 || point_size > TAMF_RENDER_MAX_POINT_SIZE || point_size % 2 == 0)
    return fail(TAMF_ERR_INVALID, "point_size must be odd and lie in [1, " + std::to_string(TAMF_RENDER_MAX_POINT_SIZE) + "], got " + std::to_string(point_size));
  hipLaunchKernelGGL(render_points_kernel<FLOOR>, tiles(F, H, W), dim3(RS_NT), 0, (hipStream_t)stream, (const int*)xy, pos_cam, P, W, H, point_size / 2,
                     prim_base, depth, (int*)prim_id, floor_depth, (const int*)floor_id);
  return launched();
}

extern "C" int tamf_render_points(const int32_t* xy, const float* pos_cam, int32_t F, int32_t P, int32_t H, int32_t W, int32_t point_size,
                                  int32_t prim_base, float* depth, int32_t* prim_id, void* stream) {
  return points<false>(xy, pos_cam, F, P, H, W, point_size, prim_base, nullptr, nullptr, depth, prim_id, stream);
}

extern "C" int tamf_render_points_behind(const int32_t* xy, const float* pos_cam, int32_t F, int32_t P, int32_t H, int32_t W, int32_t point_size,
                                         int32_t prim_base, const float* floor_depth, const int32_t* floor_id, float* depth, int32_t* prim_id,
                                         void* stream) {
  return points<true>(xy, pos_cam, F, P, H, W, point_size, prim_base, floor_depth, floor_id, depth, prim_id, stream);
}

// base_rgb: 3 HOST floats (the plain pass); vertex_rgb: device colours (the colour pass).  Exactly one of the two.
template <bool COLORS>
static int shade_mesh(const int32_t* prim_id, const int32_t* xy, const float* pos_cam, const float* normals, const int32_t* faces, int32_t F, int32_t V,
                      int32_t Nf, int32_t H, int32_t W, int32_t prim_base, const float* base_rgb, const float* vertex_rgb, int32_t col_per_frame,
                      float ambient, const float* lights, int32_t L, uint8_t* rgb, void* stream) {
  if (!prim_id || !xy || !pos_cam || !faces || !(COLORS ? vertex_rgb : base_rgb) || !rgb)
    return fail(TAMF_ERR_INVALID, COLORS ? "null argument: prim_id, xy, pos_cam, faces, vertex_rgb and rgb are required"
                                         : "null argument: prim_id, xy, pos_cam, faces, base_rgb and rgb are required");
  if (L < 0 || L > RS_MAX_LIGHTS || (L > 0 && !lights))
    return fail(TAMF_ERR_INVALID, "L outside [0, " + std::to_string(RS_MAX_LIGHTS) + "], or lights null with L > 0 (L = " + std::to_string(L) + ")");
  std::string bad = bad_image(F, H, W);
  if (bad.empty()) bad = bad_prims(F, V, Nf, prim_base);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  if ((!COLORS && !finite3(base_rgb)) || !std::isfinite(ambient)) return fail(TAMF_ERR_INVALID, "non-finite base colour or ambient term");
  RsLights Ls = {};
  Ls.ambient = ambient;
  Ls.n = L;
  for (int l = 0; l < L; ++l) {
    if (!finite3(lights + 4 * l) || !std::isfinite(lights[4 * l + 3])) return fail(TAMF_ERR_INVALID, "light " + std::to_string(l) + " is not finite");
    for (int c = 0; c < 3; ++c) Ls.dir[l][c] = lights[4 * l + c];
    Ls.strength[l] = lights[4 * l + 3];
  }
  const long n = (long)F * H * W;
  hipLaunchKernelGGL(render_shade_mesh_kernel<COLORS>, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const int*)prim_id, (const int*)xy, pos_cam, normals,
                     (const int*)faces, Nf, V, F, W, H, prim_base, COLORS ? 0.0f : base_rgb[0], COLORS ? 0.0f : base_rgb[1], COLORS ? 0.0f : base_rgb[2], Ls,
                     rgb, vertex_rgb, col_per_frame ? 1 : 0);
  return launched();
}

extern "C" int tamf_render_shade_mesh(const int32_t* prim_id, const int32_t* xy, const float* pos_cam, const float* normals, const int32_t* faces,
                                      int32_t F, int32_t V, int32_t Nf, int32_t H, int32_t W, int32_t prim_base, const float* base_rgb, float ambient,
                                      const float* lights, int32_t L, uint8_t* rgb, void* stream) {
  return shade_mesh<false>(prim_id, xy, pos_cam, normals, faces, F, V, Nf, H, W, prim_base, base_rgb, nullptr, 0, ambient, lights, L, rgb, stream);
}

extern "C" int tamf_render_shade_mesh_colors(const int32_t* prim_id, const int32_t* xy, const float* pos_cam, const float* normals, const int32_t* faces,
                                             int32_t F, int32_t V, int32_t Nf, int32_t H, int32_t W, int32_t prim_base, const float* vertex_rgb,
                                             int32_t per_frame, float ambient, const float* lights, int32_t L, uint8_t* rgb, void* stream) {
  return shade_mesh<true>(prim_id, xy, pos_cam, normals, faces, F, V, Nf, H, W, prim_base, nullptr, vertex_rgb, per_frame, ambient, lights, L, rgb, stream);
}

extern "C" int tamf_render_shade_points(const int32_t* prim_id, int32_t F, int32_t H, int32_t W, int32_t prim_base, int32_t P, const float* base_rgb,
                                        uint8_t* rgb, void* stream) {
  if (!prim_id || !base_rgb || !rgb) return fail(TAMF_ERR_INVALID, "null argument: prim_id, base_rgb and rgb are required");
  std::string bad = bad_image(F, H, W);
  if (bad.empty()) bad = bad_prims(F, 1, P, prim_base);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  if (!finite3(base_rgb)) return fail(TAMF_ERR_INVALID, "non-finite base colour");
  const long n = (long)F * H * W;
  hipLaunchKernelGGL(render_shade_points_kernel<false>, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const int*)prim_id, n, prim_base, P,
                     to_byte(base_rgb[0]), to_byte(base_rgb[1]), to_byte(base_rgb[2]), rgb, (const float*)nullptr, 0, (long)H * W);
  return launched();
}

extern "C" int tamf_render_shade_points_colors(const int32_t* prim_id, int32_t F, int32_t H, int32_t W, int32_t prim_base, int32_t P,
                                               const float* point_rgb, int32_t per_frame, uint8_t* rgb, void* stream) {
  if (!prim_id || !point_rgb || !rgb) return fail(TAMF_ERR_INVALID, "null argument: prim_id, point_rgb and rgb are required");
  std::string bad = bad_image(F, H, W);
  if (bad.empty()) bad = bad_prims(F, P, P, prim_base);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  const long n = (long)F * H * W;
  hipLaunchKernelGGL(render_shade_points_kernel<true>, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const int*)prim_id, n, prim_base, P, 0, 0, 0, rgb,
                     point_rgb, per_frame ? 1 : 0, (long)H * W);
  return launched();
}

extern "C" int tamf_render_fill(const int32_t* prim_id, int32_t F, int32_t H, int32_t W, const float* bg_rgb, uint8_t* rgb, void* stream) {
  if (!prim_id || !bg_rgb || !rgb) return fail(TAMF_ERR_INVALID, "null argument: prim_id, bg_rgb and rgb are required");
  const std::string bad = bad_image(F, H, W);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  if (!finite3(bg_rgb)) return fail(TAMF_ERR_INVALID, "non-finite background colour");
  const long n = (long)F * H * W;
  hipLaunchKernelGGL(render_fill_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, (const int*)prim_id, rgb, n, to_byte(bg_rgb[0]),
                     to_byte(bg_rgb[1]), to_byte(bg_rgb[2]));
  return launched();
}

extern "C" int tamf_render_composite(const uint8_t* layer_rgb, const int32_t* layer_id, int32_t K, int32_t F, int32_t H, int32_t W,
                                     const int32_t* item_base, const int32_t* item_count, const float* item_alpha, int32_t n_items,
                                     const float* bg_rgb, uint8_t* rgb, void* stream) {
  if (!layer_rgb || !layer_id || !item_base || !item_count || !item_alpha || !bg_rgb || !rgb)
    return fail(TAMF_ERR_INVALID, "null argument: layer_rgb, layer_id, the item table, bg_rgb and rgb are required");
  if (K < 1 || K > RS_MAX_LAYERS) return fail(TAMF_ERR_INVALID, "K outside [1, " + std::to_string(RS_MAX_LAYERS) + "], got " + std::to_string(K));
  if (n_items < 1 || n_items > RS_MAX_ITEMS)
    return fail(TAMF_ERR_INVALID, "the item table holds 1 to " + std::to_string(RS_MAX_ITEMS) + " rows, got " + std::to_string(n_items));
  const std::string bad = bad_image(F, H, W);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  if (!finite3(bg_rgb)) return fail(TAMF_ERR_INVALID, "non-finite background colour");
  if (rgb == layer_rgb) return fail(TAMF_ERR_INVALID, "rgb must not be the layers' buffer");
  RsItems items = {};
  items.n = n_items;
  long end = 0;  // rows ascending and disjoint: an id belongs to one row at most
  for (int i = 0; i < n_items; ++i) {
    const std::string row = "item " + std::to_string(i) + ": ";
    if (item_base[i] < 0 || item_count[i] < 1 || (long)item_base[i] + item_count[i] > RN_INT_MAX)
      return fail(TAMF_ERR_INVALID, row + "prim_base < 0, count < 1 or prim_base + count above 2^31 - 1");
    if (item_base[i] < end) return fail(TAMF_ERR_INVALID, row + "the rows must ascend in prim_base and must not overlap");
    if (!(item_alpha[i] > 0.0f && item_alpha[i] <= 1.0f)) return fail(TAMF_ERR_INVALID, row + "alpha must lie in (0, 1]");
    end = (long)item_base[i] + item_count[i];
    items.base[i] = item_base[i], items.count[i] = item_count[i], items.alpha[i] = item_alpha[i];
  }
  const long n = (long)F * H * W;
  const auto clamp01 = [](float c) { return std::fmin(std::fmax(c, 0.0f), 1.0f); };
  hipLaunchKernelGGL(render_composite_kernel, dim3(blocks(n)), dim3(256), 0, (hipStream_t)stream, layer_rgb, (const int*)layer_id, K, n, items,
                     clamp01(bg_rgb[0]), clamp01(bg_rgb[1]), clamp01(bg_rgb[2]), rgb);
  return launched();
}

extern "C" int tamf_render_resolve(const uint8_t* rgb_in, int32_t F, int32_t H, int32_t W, int32_t s, uint8_t* rgb, void* stream) {
  if (!rgb_in || !rgb) return fail(TAMF_ERR_INVALID, "null argument: rgb_in and rgb are required");
  if (s < 2 || s > 4) return fail(TAMF_ERR_INVALID, "s must be 2, 3 or 4, got " + std::to_string(s));
  if (rgb_in == rgb) return fail(TAMF_ERR_INVALID, "rgb must not be rgb_in");
  std::string bad = bad_image(F, H, W);
  if (bad.empty() && ((long)s * W > TAMF_RENDER_MAX_SIDE || (long)s * H > TAMF_RENDER_MAX_SIDE))
    bad = "s * W and s * H must not exceed " + std::to_string(TAMF_RENDER_MAX_SIDE) + " (s = " + std::to_string(s) + ", H = " + std::to_string(H) +
          ", W = " + std::to_string(W) + ")";
  if (bad.empty()) bad = bad_image(F, s * H, s * W);
  if (!bad.empty()) return fail(TAMF_ERR_INVALID, bad);
  hipLaunchKernelGGL(render_resolve_kernel, dim3(blocks((long)F * H * W)), dim3(256), 0, (hipStream_t)stream, rgb_in, F, H, W, s, rgb);
  return launched();
}
