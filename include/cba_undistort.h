/*
 * cba_undistort.h -- undistortion of a central-generic camera's images to pinhole images with libcalib_ba_hip.so: the
 * undistortion map of a device-resident model (include/cba.h: cba_model) and the cba_remap handle that applies it to 8-bit images.
 * A header of its own next to cba.h, as cba_rccl.h is: cba.h holds what mirrors the reference, and this has no reference function.
 * The reference's Readme ("Which camera model to choose?") gives undistortion as the reason to prefer the central model, and its
 * stereo tool builds per-pixel un-projection lookups instead (APP/tools/stereo_depth_estimation.cc:134-168).
 * Non-central models cannot be undistorted without scene geometry: CBA_ERR_ARG.  Error codes and conventions are cba.h's.
 */
#ifndef CBA_UNDISTORT_H_
#define CBA_UNDISTORT_H_
#include "cba.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t width, height;                   /* target (pinhole) image */
  double fx, fy, cx, cy;                   /* "pixel corner" convention, as every pixel in cba.h */
  double rotation[9];                      /* row-major source_r_target: source ray = R * target ray */
  int32_t initial_estimate;                /* 0 = centre of the calibrated area (CameraModel::Project); 1 = target pixel centre scaled by
                                              (source width / width, source height / height), clamped into [min, max + 0.999] as
                                              cba_compare_options does.  The two starts stop at different iterates of the projection's
                                              LM: their results differ by its stopping threshold (about 1e-7 px) */
  int32_t straggler_threshold;             /* as cba_compare_options: scheduling only */
} cba_undistort_options;
/* Per target pixel (u, v): t = normalize(((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy, 1), g = R t, Project(g) into the model from the
 * chosen start, in two launches as cba_model_compare (pixels that reach the iteration cap are finished by a second launch;
 * n_second_launch (optional) counts them).  Each output may be NULL, not all three:
 *   source_pixels  2 width height: the projection, pixel-corner convention, NaN where it fails
 *   ok             width height: its return value
 *   map_xy         2 width height: (float)(source pixel - 0.5), pixel-centre convention, NaN where not ok: what cba_remap_apply reads
 * CBA_ERR_ARG (before any device call): a model that is not central-generic, width or height < 1, fx or fy not finite or not
 * positive, an unknown initial_estimate, every output NULL. */
int cba_model_undistortion_map(cba_model* m, const cba_undistort_options* o, double* source_pixels, uint8_t* ok, float* map_xy,
                               int64_t* n_second_launch);
/* A device-resident map and the bilinear remap of 8-bit images through it.  cba_remap_create builds the map on the model's device
 * (no host copy); cba_remap_create_from_map uploads width x height entries (x, y).
 * Images: n of src_w x src_h x channels (1 or 3) bytes, row-major, densely packed; dst: n x height x width x channels.
 * THE ARITHMETIC IS FIXED (float = IEEE binary32, every operation rounded on its own, nothing fused):
 *   (sx, sy) = the map entry.  NaN, or a magnitude above 2^24, in either: every channel of the pixel is `fill`.
 *   x0 = floorf(sx), wx = sx - x0, x1 = x0 + 1; then both indices are clamped into [0, src_w - 1] (the border is replicated); y alike.
 *   per channel: top = p00 + wx * (p10 - p00), bot = p01 + wx * (p11 - p01), v = top + wy * (bot - top), p_xy the bytes at
 *   (x_x, y_y) as floats; byte = (uint8_t)(int)(v + 0.5f), which cannot exceed 255.
 * cba_remap_apply stages through the handle's own buffers on the engine's stream of the handle's device and returns when dst is
 * written.  cba_remap_apply_device only launches on `hip_stream` (a hipStream_t; device pointers of the handle's device) and returns.
 * CBA_ERR_ARG (nothing is launched): a NULL pointer, channels other than 1 or 3, src_w or src_h < 1, n < 1 or n > 65535, a bad
 * device ordinal. */
typedef struct cba_remap cba_remap;
int cba_remap_create(cba_model* m, const cba_undistort_options* o, cba_remap** out);
int cba_remap_create_from_map(int32_t width, int32_t height, const float* map_xy, int32_t device, cba_remap** out);
void cba_remap_destroy(cba_remap* r);
int cba_remap_get_map(cba_remap* r, float* map_xy);
int cba_remap_apply(cba_remap* r, int32_t n, int32_t src_w, int32_t src_h, int32_t channels, const uint8_t* src, uint8_t* dst, uint8_t fill);
int cba_remap_apply_device(cba_remap* r, int32_t n, int32_t src_w, int32_t src_h, int32_t channels, const uint8_t* d_src, uint8_t* d_dst,
                           uint8_t fill, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* CBA_UNDISTORT_H_ */
