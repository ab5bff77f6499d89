/* rv3d_render.h -- the debug panels of the training loop and mmcv's IoU ops (csrc/render.hip): a companion of rv3d.h, which
 * it includes (rvStream, the error contract: an int-returning entry returns non-zero and rv_last_error() says why).  A C / C++ caller
 * includes this file; the Python binding (`_lib.py`, `companion_prototypes()`) types its entries exactly as it types rv3d.h's. */
#ifndef RV3D_RENDER_H_
#define RV3D_RENDER_H_
#include "rv3d.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------
 * Debug panels of the training loop and mmcv's IoU ops (csrc/render.hip).  What the reference's
 * rendering/tensorboard.py (to_logger / draw_detections, called from nn/arch/detector.py:297-306, 355-364) builds on the host
 * from tensors it first copies there, built where the tensors are: one planar uint8 image (3, H_total, W_total), which the
 * caller zeroes once, filled block by block.  Pinned to the reference: the plane ops, normalize_apply_colormap with kornia's
 * normalize_min_max, the colour tables, build_bev / world_to_image, the panel order and the padding (tests/golden/render/).
 * DECLARED, because cv2 and mmcv are not part of the reference tree: the line raster, rv_boxes_iou3d's conventions, and that the aux
 * panels carry no text label (there is no cv2 font).  All entries are asynchronous on `stream`, own no memory and return non-zero
 * before anything is launched for a null required pointer, a non-positive size or a block that does not fit the image.
 *
 * Scalar planes.  rv_render_plane: src = a (C, H, W) fp32 slice with `channel_stride` elements between channels -> plane (H, W) fp32,
 * an output the caller can read, by
 *   RV_PLANE_NORM        C = 3:  sqrtf((x*x + y*y) + z*z), in this order;
 *   RV_PLANE_LIKELIHOOD  1 / (1 + expf(-max_c logit)) -- the sigmoid is monotone, so this equals sigmoid().max(dim=0); the maximum is
 *                        fmaxf's (a NaN logit is passed over);
 *   RV_PLANE_ABS         C = 1:  fabsf(x);
 *   RV_PLANE_IDENTITY    C = 1:  x (a plane the caller already has: normalize_apply_colormap as a function of its own);
 * every step one fp32 IEEE operation (no fused multiply-add), expf the device library's (1 to 2 ulps).  The same launch reduces the
 * plane's minimum and maximum over ALL pixels, masked ones included, into `minmax`: two 32-bit words that the caller zeroes before the
 * call, holding order-preserving integer keys of the two floats (opaque; only rv_render_colormap reads them).  The reduction is an
 * integer maximum, so its result does not depend on the order.
 *
 * normalize_apply_colormap.  rv_render_colormap: idx = (long)(((x - min) / ((max - min) + 1e-6f)) * 255.0f), each step one fp32
 * operation, the division correctly rounded; idx is clamped to 0 .. 255 and a NaN takes 0.  A constant plane maps to index 0.
 * rgb = lut[ch][idx] * (mask[pixel] != 0) (mask (H, W) u8, or NULL = keep all) goes to image[ch][row0 + r][col0 + c] for the three
 * channels; `lut` is a DEVICE table (3, 256) u8.  Columns of the image outside the block are not touched (they stay 0).
 *
 * Colour tables.  RV_CMAP_GREYS (matplotlib binary_r), RV_CMAP_TURBO_R, RV_CMAP_VIRIDIS: 256 x 3 bytes each, uint8(cmap(i)[:3] * 255.0)
 * in fp64, truncating, as tensorboard.py:27-44 makes them; csrc/colormaps.h, written by csrc/gen_colormaps.py, holds the only copy.
 * rv_render_colormap_table copies table `table` out to 768 HOST bytes, (256, 3) row-major (needs no device).
 *
 * Bird's-eye view.  side = int(math.ceil(max_side * 2 / meter_per_px)) is computed by the caller with exactly this Python expression
 * (1000 for 75 / 0.15); 1 <= side <= 4096.  The view is the block [row0, row0 + side) x [col0, col0 + side) of the image.
 * world_to_image of one coordinate v (fp32): u = (v + (float)max_side) / (float)meter_per_px; kept iff 0 < u < upper with
 * upper = (float)(max_side / meter_per_px * 2.0); pixel = floorf(size - u) with size = (float)(max_side * 2.0 / meter_per_px); the two
 * constants are the reference's fp64 Python expressions, rounded to fp32 where they meet the tensor.  row comes from x, column from y.
 * rv_render_bev_points: cart = (3, n) fp32 x, y, z planes `channel_stride` apart.  A point with sqrtf((x*x + y*y) + z*z) > 0 whose x
 * and y are both kept sets pixel (row, col) to 255 in all three channels; a row or column outside 0 .. side - 1 (`side` itself, where the
 * reference would raise) is dropped.
 * rv_render_bev_boxes: boxes (n, 7) fp32 [x, y, z, l, w, h, yaw] drawn in row order, a later box over an earlier one; scores (n) fp32
 * or NULL (= 1); channels (n) u8, bit 0 red, bit 1 green, bit 2 blue.  Footprint corners 6, 2, 3, 7 of cuboids_to_vertices
 * (polytope.py:76-107), i.e. rear-right, front-right, front-left, rear-left: (x, y) + R(yaw) (+-l/2, +-w/2) with halves 0.5f * l,
 * sin / cos the fp32 roundings of the fp64 values, x' = x + (hx c - hy s), y' = y + (hx s + hy c) unfused.  Each corner goes through
 * world_to_image and is truncated to int32; corners that are not kept are removed and the open polyline (the rear edge stays open)
 * runs through those that remain, nothing being drawn for fewer than two.  DECLARED raster rule (the reference draws with
 * cv2.polylines(thickness=2, LINE_AA), which is not available), integers only: pixel p belongs to segment a -> b iff its squared
 * distance to the segment is <= 1; with d = b - a, L2 = d.d, t = clamp((p - a).d, 0, L2) the test is
 * |(p - a) * L2 - t * d|^2 <= L2 * L2 in int64, |p - a|^2 <= 1 for L2 == 0, evaluated over the segment's bounding box grown by one pixel
 * and clipped to the view.  (The kernel evaluates the three cases t = 0, t = L2 and 0 < t < L2 of the same inequality divided by L2,
 * which are exact and cannot overflow.)  A pixel of a segment takes value = uint8(rintf(255.0f * score)) (saturating) in the box's
 * channels and 0 in the others.  Order: atomicMax of the draw index (row + 1) on `zbuf`, side x side 32-bit words owned by the caller
 * and cleared by the call, then one resolve pass: the result does not depend on scheduling.  Three stream operations.
 *
 * rv_boxes_iou3d -- mmcv.ops.boxes_iou3d.  a (n, 7) x b (m, 7) rows [x, y, z, dx, dy, dz, yaw] with z the box CENTRE -> out (n, m) fp32,
 * one thread per pair: the 3-D IoU of "IoU of a pair" in rv3d.h (rv_waymo_iou), the same device function, so the two agree bit for
 * bit; no limit on n or m beyond 2^31 - 1 each.  DECLARED: mmcv is not in the reference tree (its LiDAR boxes put z at the bottom face
 * in some versions; this entry takes the centre, which is what tensorboard.py:296-314 passes).
 * rv_rotated_iou_pairs -- the ALIGNED form of rv_rotated_iou: out[k] = IoU(a[k], b[k]) for rectangles (n, 5) [x1, y1, x2, y2, ry], per
 * pair (no n x n table), bit-equal to the diagonal of rv_rotated_iou.
 * ------------------------------------------------------------------------------------- */
#define RV_PLANE_NORM 0
#define RV_PLANE_LIKELIHOOD 1
#define RV_PLANE_ABS 2
#define RV_PLANE_IDENTITY 3
#define RV_CMAP_GREYS 0
#define RV_CMAP_TURBO_R 1
#define RV_CMAP_VIRIDIS 2
int rv_render_colormap_table(int32_t table, uint8_t* host_out);
int rv_render_plane(const float* src, int64_t channel_stride, int32_t C, int32_t H, int32_t W, int32_t op, float* plane, void* minmax,
                    rvStream stream);
int rv_render_colormap(const float* plane, const uint8_t* mask, int32_t H, int32_t W, const void* minmax, const uint8_t* lut,
                       uint8_t* image, int32_t H_total, int32_t W_total, int32_t row0, int32_t col0, rvStream stream);
int rv_render_bev_points(const float* cart, int64_t channel_stride, int64_t n, double max_side, double meter_per_px, int32_t side,
                         uint8_t* image, int32_t H_total, int32_t W_total, int32_t row0, int32_t col0, rvStream stream);
int rv_render_bev_boxes(const float* boxes, const float* scores, const uint8_t* channels, int64_t n, double max_side, double meter_per_px,
                        int32_t side, void* zbuf, uint8_t* image, int32_t H_total, int32_t W_total, int32_t row0, int32_t col0,
                        rvStream stream);
int rv_boxes_iou3d(const float* a, int64_t n, const float* b, int64_t m, float* out, rvStream stream);
int rv_rotated_iou_pairs(const float* a, const float* b, int64_t n, float* out, rvStream stream);

#ifdef __cplusplus
}
#endif
#endif /* RV3D_RENDER_H_ */
