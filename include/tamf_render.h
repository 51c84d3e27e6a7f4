/*
 * tamf_render.h - C-ABI of the offscreen renderer (libtamf_render.so), 14 functions: projection, a triangle / point-splat rasteriser
 * with a depth and a primitive-id buffer, Lambert shading with a constant or per-vertex colour, depth peeling for see-through items,
 * a compositing pass and a supersampling resolve.  It stands where the reference's viewers and its dev_fn/util/vis_pyrender_util.py
 * PyMultiObjRenderer need Open3D or pyrender with OpenGL and a display: a headless MI355X node has neither.
 *
 * The image is THIS PACKAGE'S definition, not pyrender's: OpenGL rasterisation is not reproducible bit for bit and pyrender shades
 * with a PBR model.  No textures, no shadows, no clipping: a triangle with a vertex in front of the near plane is dropped whole, in
 * every layer.  Anti-aliasing is a box filter over s x s sub-samples (tamf_render_resolve), nothing finer.
 * The definition is restated in numpy in tests/render_restatement.py.
 *
 * Camera: pinhole, OpenCV frame (x right, y down, z forward; what PyMultiObjRenderer's cam_intr and PYRENDER_EXTR imply).
 *   tamf_render_camera.view (3,4) row-major, world -> camera; fx, fy, cx, cy the intrinsics in pixels; near > 0.
 *   The centre of pixel (column i, row j) is at (i + 0.5, j + 0.5).  1 <= W, H <= 4096.
 *
 * Fixed point: screen coordinates are int32 in units of 1/256 pixel.  An INVALID vertex (non-finite, z < near, or a snapped
 * coordinate of magnitude above 2^28) carries INT32_MIN in both coordinates.  With |coordinate| <= 2^28 the differences fit int32 and
 * the edge functions fit int64, so coverage is exact integer arithmetic.
 *
 * Coverage of a triangle (vertices 0, 1, 2 with snapped x_k, y_k and camera depth z_k):
 *   - dropped whole when a vertex is invalid or a face index lies outside [0, V); dropped when the doubled area
 *     a2 = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0) is 0; when a2 < 0, vertices 1 and 2 are swapped first (both windings are drawn)
 *   - edge k runs from a = vertex k+1 to b = vertex k+2 (mod 3): A = y_a - y_b, B = x_b - x_a, C = x_a y_b - y_a x_b,
 *     E_k = A px + B py + C at the centre (px, py) = (256 i + 128, 256 j + 128)
 *   - the centre is inside edge k iff E_k > 0, or E_k == 0 and (A > 0 or (A == 0 and B < 0)): the top-left rule of a y-up frame
 *     (with y pointing down, the image's left and bottom edges own their centres), so a centre on an edge shared by two triangles
 *     belongs to exactly one of them
 *   - depth (fp32) = 1 / inv_z, inv_z = (E_0 / z_0 + E_1 / z_1 + E_2 / z_2) / a2: perspective-correct
 * Depth test: a candidate replaces the stored (depth, id) only when its depth is strictly smaller.  Within a call the lowest
 * primitive index wins an exact tie; across calls the earlier call wins.  The stored id is prim_base + primitive index; -1 is none.
 *
 * Depth peeling (tamf_render_raster_behind, tamf_render_points_behind): with a floor (floor_depth, floor_id) per pixel, a candidate of
 * depth d and global id = prim_base + index is ADMITTED only where floor_id >= 0 and (d > floor_depth, or d == floor_depth and
 * id > floor_id); admitted candidates go through the unchanged depth test.  d is computed by the device code of tamf_render_raster /
 * tamf_render_points (one kernel body, two instantiations), so a fragment's depth has the same bits in every pass and the comparison
 * against the library's own earlier output is exact.  The calls of a pass over several items MUST be made in ascending prim_base:
 * then "the earlier call wins a tie" and "the lower id wins a tie" are one rule, the order (depth, id) is total, and with layer 0
 * drawn by the plain calls and layer k by the _behind calls over ALL items with layer k - 1 as floor, layer k holds at every pixel the
 * k-th fragment of that order, each fragment once.  The number of passes K is the caller's: fragments beyond layer K - 1 are dropped.
 *
 * Compositing (tamf_render_composite), per pixel and channel in fp32: C = clamp(bg, 0, 1); for k = K - 1 down to 0, where layer k's
 * id is >= 0 and belongs to item i: C = alpha_i * (byte_k / 255) + (1 - alpha_i) * C; byte = floor(255 * clamp(C, 0, 1) + 0.5).
 * Resolve (tamf_render_resolve): output byte = (sum of the s * s bytes + s * s / 2) / (s * s) in integers.
 *
 * Determinism: no atomics, one writer per output element.  The same call gives the same bits, and frame f of a call over F frames
 * gives the bits it gives in a call of its own.
 *
 * Limits (anything else is TAMF_ERR_INVALID with a message, and nothing is launched): 1 <= W, H <= 4096; 1 <= F <= 65535 and
 * F * H * W < 2^31; 1 <= V, P, Nf and V, P, F * V, F * P < 2^31 / 3; prim_base >= 0 and prim_base + count < 2^31; point_size odd in
 * [1, 15]; 0 <= L <= 8; near > 0 and finite intrinsics; a null mandatory pointer; 1 <= K <= 8 layers; 1 to 64 item rows, ascending in
 * prim_base and disjoint, alpha in (0, 1]; s in {2, 3, 4} with s * W, s * H <= 4096; a floor or input buffer that is also the output.
 *
 * Conventions: those of tamf_hip.h (included for the tamf_status enum only).  Every function returns 0 or a negative tamf_status;
 * the message of the calling thread's last failure is tamf_render_last_error().  `stream` is a hipStream_t passed as void*.
 * Nothing synchronises.  Pointers named *_dev are C-contiguous device memory owned by the caller; the camera, the colours and the
 * lights are small HOST structures read during the call.
 */
#ifndef TAMF_RENDER_H
#define TAMF_RENDER_H

#include <stdint.h>

#include "tamf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define TAMF_RENDER_MAX_LIGHTS 8
#define TAMF_RENDER_MAX_SIDE 4096
#define TAMF_RENDER_MAX_POINT_SIZE 15
#define TAMF_RENDER_MAX_LAYERS 8
#define TAMF_RENDER_MAX_ITEMS 64

typedef struct tamf_render_camera {
  float view[12]; /* (3,4) row-major, world -> camera */
  float fx, fy, cx, cy;
  float near;
} tamf_render_camera;

/* message of the last failure of a call made by THIS thread ("" when none) */
const char* tamf_render_last_error(void);

/* verts (V,3) f32, or (F,V,3) when per_frame != 0; model (F,3,4) f32 row-major, the rigid pose of frame f applied before the view,
 * or NULL for identity.  -> pos_cam (F,V,3) f32 camera-space positions (written for invalid vertices too) and xy (F,V,2) i32 =
 * round-half-even(256 * (fx x / z + cx, fy y / z + cy)), or INT32_MIN twice for an invalid vertex. */
int tamf_render_project(const float* verts_dev, const float* model_dev, const tamf_render_camera* camera, int32_t F, int32_t V,
                        int32_t per_frame, float* pos_cam_out_dev, int32_t* xy_out_dev, void* stream);

/* depth (F,H,W) f32 := +inf, prim_id (F,H,W) i32 := -1 */
int tamf_render_clear(float* depth_dev, int32_t* prim_id_dev, int32_t F, int32_t H, int32_t W, void* stream);

/* Triangles faces (Nf,3) i32 over the vertices xy (F,V,2), pos_cam (F,V,3) of tamf_render_project, depth-tested into depth / prim_id
 * (F,H,W), which are read and updated. */
int tamf_render_raster(const int32_t* xy_dev, const float* pos_cam_dev, const int32_t* faces_dev, int32_t F, int32_t V, int32_t Nf,
                       int32_t H, int32_t W, int32_t prim_base, float* depth_dev, int32_t* prim_id_dev, void* stream);

/* Points xy (F,P,2), pos_cam (F,P,3): each valid point is a square of point_size x point_size pixels centred on the pixel that
 * holds its projection (floor(xy / 256)), of the point's constant depth z, through the same depth test. */
int tamf_render_points(const int32_t* xy_dev, const float* pos_cam_dev, int32_t F, int32_t P, int32_t H, int32_t W, int32_t point_size,
                       int32_t prim_base, float* depth_dev, int32_t* prim_id_dev, void* stream);

/* Writes rgb (F,H,W,3) u8 ONLY at pixels whose id lies in [prim_base, prim_base + Nf); xy, pos_cam, faces: what the raster call
 * of this mesh was given.  With w_k = (E_k / z_k) / sum_j (E_j / z_j) at the pixel centre:
 *   normal   normals_dev == NULL: the unit face normal from pos_cam; else the normalised blend sum_k w_k n_k of the camera-space
 *            vertex normals (F,V,3); either one flipped to face the viewer: negated when n . p > 0 at p = sum_k w_k pos_cam_k
 *   I      = ambient + sum over the L lights of strength * max(0, -n . dir)      lights (L,4) HOST rows: unit dir (the direction the
 *            light travels, camera frame), strength
 *   byte   = floor(255 * clamp(base * I, 0, 1) + 0.5) per channel of base_rgb (3 HOST floats) */
int tamf_render_shade_mesh(const int32_t* prim_id_dev, const int32_t* xy_dev, const float* pos_cam_dev, const float* normals_dev,
                           const int32_t* faces_dev, int32_t F, int32_t V, int32_t Nf, int32_t H, int32_t W, int32_t prim_base,
                           const float* base_rgb, float ambient, const float* lights, int32_t L, uint8_t* rgb_dev, void* stream);

/* rgb := byte(base_rgb), unlit, at pixels whose id lies in [prim_base, prim_base + P) */
int tamf_render_shade_points(const int32_t* prim_id_dev, int32_t F, int32_t H, int32_t W, int32_t prim_base, int32_t P,
                             const float* base_rgb, uint8_t* rgb_dev, void* stream);

/* rgb := byte(bg_rgb) where the id is -1 */
int tamf_render_fill(const int32_t* prim_id_dev, int32_t F, int32_t H, int32_t W, const float* bg_rgb, uint8_t* rgb_dev, void* stream);

/* tamf_render_raster behind a floor: floor_depth (F,H,W) f32 and floor_id (F,H,W) i32, the depth / prim_id of the previous layer (not
 * the buffers drawn into).  See "Depth peeling" above: calls in ascending prim_base. */
int tamf_render_raster_behind(const int32_t* xy_dev, const float* pos_cam_dev, const int32_t* faces_dev, int32_t F, int32_t V, int32_t Nf,
                              int32_t H, int32_t W, int32_t prim_base, const float* floor_depth_dev, const int32_t* floor_id_dev,
                              float* depth_dev, int32_t* prim_id_dev, void* stream);

/* tamf_render_points behind a floor, in the same way */
int tamf_render_points_behind(const int32_t* xy_dev, const float* pos_cam_dev, int32_t F, int32_t P, int32_t H, int32_t W, int32_t point_size,
                              int32_t prim_base, const float* floor_depth_dev, const int32_t* floor_id_dev, float* depth_dev,
                              int32_t* prim_id_dev, void* stream);

/* tamf_render_shade_mesh with the colours vertex_rgb (V,3) f32, or (F,V,3) when per_frame != 0, in place of base_rgb: the pixel's
 * base colour is sum_k w_k c_k with the w_k that blend the normals, evaluated as c_0 + w_1 (c_1 - c_0) + w_2 (c_2 - c_0) (the w_k sum
 * to 1), so three equal colours c give the bytes of tamf_render_shade_mesh with base_rgb = c. */
int tamf_render_shade_mesh_colors(const int32_t* prim_id_dev, const int32_t* xy_dev, const float* pos_cam_dev, const float* normals_dev,
                                  const int32_t* faces_dev, int32_t F, int32_t V, int32_t Nf, int32_t H, int32_t W, int32_t prim_base,
                                  const float* vertex_rgb_dev, int32_t per_frame, float ambient, const float* lights, int32_t L,
                                  uint8_t* rgb_dev, void* stream);

/* rgb := byte(colour of the pixel's own point), unlit, at pixels whose id lies in [prim_base, prim_base + P); point_rgb (P,3) f32, or
 * (F,P,3) when per_frame != 0 */
int tamf_render_shade_points_colors(const int32_t* prim_id_dev, int32_t F, int32_t H, int32_t W, int32_t prim_base, int32_t P,
                                    const float* point_rgb_dev, int32_t per_frame, uint8_t* rgb_dev, void* stream);

/* K layers layer_rgb (K,F,H,W,3) u8 and layer_id (K,F,H,W) i32 -> rgb (F,H,W,3) u8 by "Compositing" above.  The item table is n_items
 * HOST rows (item_base[i], item_count[i], item_alpha[i]): the ids [base, base + count) are drawn with that alpha.  Every id >= 0 of
 * the layers must belong to a row: the table is checked on the host (ascending, disjoint, alpha in (0, 1]); an id outside every row is
 * the caller's error, and such a layer leaves the pixel as the layers behind it made it. */
int tamf_render_composite(const uint8_t* layer_rgb_dev, const int32_t* layer_id_dev, int32_t K, int32_t F, int32_t H, int32_t W,
                          const int32_t* item_base, const int32_t* item_count, const float* item_alpha, int32_t n_items, const float* bg_rgb,
                          uint8_t* rgb_dev, void* stream);

/* rgb_in (F, s H, s W, 3) u8 -> rgb (F,H,W,3) u8: the rounded mean of every s x s block, s in {2, 3, 4} */
int tamf_render_resolve(const uint8_t* rgb_in_dev, int32_t F, int32_t H, int32_t W, int32_t s, uint8_t* rgb_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* TAMF_RENDER_H */
