/*
 * cba_point_cloud.h -- comparison of two stereo results of the same image on the device: the reference's ComparePointClouds
 * (APP/tools/compare_point_clouds.cc:73-191, --compare_point_clouds).  Two depth maps are intersected, the two clouds of the common
 * pixels are aligned with a similarity transform, and the distance that remains is written per pixel.  THIS HEADER IS THE DEFINITION:
 * it fixes the order of the points, the arithmetic and every deviation from the reference; tests/point_cloud_reference.py restates it
 * in numpy.  Error codes and conventions are cba.h's (a header of its own, as cba_stereo.h is).
 *
 * TERMS.  W, H: the size of both maps; r: the context radius of the stereo run.
 *   inner region     r <= x < W - r, r <= y < H - r, walked row-major (y outer, x inner)
 *   valid in a map   the map's value at the pixel != 0 (-0.0 is invalid, NaN is valid)
 *   cloud of a map   one point per valid inner pixel, in that order: what the stereo tool writes as point_cloud.ply
 *   common pixels    the inner pixels valid in both maps, in that order.  Common pixel k is paired with point rank_t(k) of the target
 *                    cloud and point rank_s(k) of the source cloud; a rank is the number of valid inner pixels of that map before
 *                    the pixel (the two running indices of compare_point_clouds.cc:114-132).
 *
 * COMPACTION.  Three launches, integers only, no workgroup waits on another: (i) every workgroup counts the pixels valid in the
 * target, valid in the source and common over its span of CBA_CLOUD_PIXELS_PER_BLOCK consecutive inner pixels; (ii) exclusive scans of
 * the per-workgroup counts; (iii) every workgroup ranks its pixels (ballots, wavefront offsets in LDS) and gathers the common pairs.
 *
 * ARITHMETIC.  Points of the in-memory path: depth = 1.f / m, x = depth * ux, y = depth * uy, z = depth in float32 with IEEE division
 * (what stereo.point_cloud computes).  Moments: every term is formed in fp64 from the float32 coordinates, nothing contracted, and
 * summed in a fixed order (a fixed number of workgroups, a fixed tree in each, the partials folded in ascending order): identical from
 * run to run.  Alignment: p' = ((A0 x + A1 y) + A2 z) + t0 and likewise rows 1 and 2, d = sqrt((dx dx + dy dy) + dz dz) with
 * (dx, dy, dz) = target - p', all float32, nothing contracted, IEEE square root.  PRECONDITION: every coordinate, A and t are finite
 * (the maximum compares bit patterns).
 *
 * DEVIATIONS from the reference.  It runs Eigen's umeyama in float over all points; here the moments are fp64 fixed-order sums, the
 * 3 x 3 SVD is the caller's on the host in fp64 (camera_calibration_amd/point_clouds.py: umeyama_from_moments), and the result is
 * rounded once to the float32 A = c R and t that the device applies.  The reference shows the distance image in a window, leaves
 * saving it as a TODO (:181-184) and waits for a key press; the tool here saves it and does not wait.
 */
#ifndef CBA_POINT_CLOUD_H_
#define CBA_POINT_CLOUD_H_
#include "cba.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the span of consecutive inner pixels that one workgroup counts and ranks */
enum { CBA_CLOUD_PIXELS_PER_BLOCK = 1024 };

typedef struct cba_cloud_pair cba_cloud_pair;

/* Both constructors: CBA_ERR_ARG before any device call for a NULL pointer (the grey arrays may be NULL: grey values are then 0),
 * width or height < 1, context_radius < 0, width * height > 2^30, an empty inner region, n_target or n_source < 0.  Both return
 * after the gather; the maps and the whole clouds are released then, the handle keeps the common pairs.
 * The 2^30 limit keeps every count and pixel index in an int32.  The scans of launch (ii) run on one workgroup each, 1024 counts per
 * trip, one row of counts after the other: 3 x 3 trips at 1920 x 1200, but 3 x 1024 serial trips at the limit (2^20 spans).  The
 * constructors are meant for camera-sized images; at the limit the scan, not the streaming launches, is what a call waits for. */

/* The files' path.  depth_*: width * height floats; xyz_*: n_* x 3 floats; grey_*: n_* bytes.  Builds the masks, the per-workgroup
 * counts, the scans and the three totals, reads the totals back in one host wait and returns CBA_ERR_ARG when the number of valid
 * inner pixels of a map differs from its n (the reference's CHECK_EQ at :135); no kernel indexes a cloud before that check. */
int cba_cloud_pair_create(int32_t width, int32_t height, int32_t context_radius, const float* depth_target, const float* depth_source,
                          const float* xyz_target, int64_t n_target, const uint8_t* grey_target,
                          const float* xyz_source, int64_t n_source, const uint8_t* grey_source, int32_t device, cba_cloud_pair** out);

/* The in-memory path for two stereo results.  inv_depth_*: width * height floats; unprojection_*: width * height x 2 floats
 * (dx / dz, dy / dz per pixel); grey_image_*: width * height bytes.  The points of a common pixel are computed in the gather. */
int cba_cloud_pair_create_from_depth(int32_t width, int32_t height, int32_t context_radius,
                                     const float* inv_depth_target, const float* unprojection_target, const uint8_t* grey_image_target,
                                     const float* inv_depth_source, const float* unprojection_source, const uint8_t* grey_image_source,
                                     int32_t device, cba_cloud_pair** out);

void cba_cloud_pair_destroy(cba_cloud_pair* h);

/* out[3]: valid inner pixels of the target, of the source, common pixels */
int cba_cloud_pair_counts(cba_cloud_pair* h, int64_t* out);

/* out[17] with x the source and y the target points of the n common pairs: [0] n, [1..3] mean of x, [4..6] mean of y,
 * [7..15] sum (y - mean y)(x - mean x)^T / n row-major, [16] sum ((dx dx + dy dy) + dz dz) / n with d = x - mean x.  Two passes, the
 * means first; a mean is its sum / n, the second pass subtracts these means.  n < 3: CBA_ERR_ARG. */
int cba_cloud_pair_moments(cba_cloud_pair* h, double* out);

/* Transforms the (untransformed) source points with A (3 x 3 row-major) and t and keeps the result on the device.
 * distance_image: width * height floats, 0 at every pixel that is not common; stats[3]: n, sum d, sum d^2 (fp64 terms from the
 * float32 d, fixed order); max_distance: the largest d, by an integer atomic maximum on the bits (0 without a common pixel).
 * distance_image, stats and max_distance may each be NULL. */
int cba_cloud_pair_align(cba_cloud_pair* h, const float* A, const float* t, float* distance_image, double* stats, float* max_distance);

/* The two intersected clouds in common-pixel order: n x 3 floats and n bytes each (each pointer may be NULL); the source after the
 * last cba_cloud_pair_align, or untransformed if none ran. */
int cba_cloud_pair_get_clouds(cba_cloud_pair* h, float* xyz_target_common, uint8_t* grey_target_common, float* xyz_source_aligned,
                              uint8_t* grey_source_common);

#ifdef __cplusplus
}
#endif
#endif /* CBA_POINT_CLOUD_H_ */
