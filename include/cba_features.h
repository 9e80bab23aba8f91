/*
 * cba_features.h -- refinement of predicted star-pattern feature positions in an 8-bit image with libcalib_ba_hip.so: the GPU
 * stage of the reference's feature extraction, FeatureDetectorTaggedPattern::RefineFeatureDetections
 * (APP/feature_detection/feature_detector_tagged_pattern.cc:1427-1648; cpu_refinement_by_matching.h, cpu_refinement_by_symmetry.h).
 * A header of its own next to cba.h: it needs no model and no problem, a detector includes it alone.  Error codes are cba.h's.
 * Positions are in the "pixel centre" convention ((0, 0) is the centre of the top left pixel), as FeatureDetection::position.
 *
 * THE ARITHMETIC IS FIXED: per sample fp32 with every operation rounded on its own, in the order the
 * reference's CPU headers write it, sampling as Image::InterpolateBilinear / InterpolateBilinearWithJacobian /
 * ContainsPixelCenterConv; cost, b and H are fp64 sums of those fp32 terms in one fixed order; the solve is an fp64 LDL^T of
 * H + lambda I without pivoting.  The sample set is an input (the reference draws it from Vec2f::Random() after srand(0)).
 */
#ifndef CBA_FEATURES_H_
#define CBA_FEATURES_H_
#include "cba.h"
#ifdef __cplusplus
extern "C" {
#endif

/* the reference's FeatureRefinement enum; its GPU branch refuses GradientMagnitude (1) and NoRefinement (3), and so does this */
#define CBA_FEATURE_REFINEMENT_GRADIENTS_XY 0
#define CBA_FEATURE_REFINEMENT_INTENSITIES 2

/* status of a feature */
#define CBA_FEATURE_REFINED 0
#define CBA_FEATURE_MATCHING_OUTSIDE_IMAGE 1  /* matching: a sample left the image */
#define CBA_FEATURE_MATCHING_LEFT_WINDOW 2    /* matching: the position left the window */
#define CBA_FEATURE_MATCHING_NOT_CONVERGED 3
#define CBA_FEATURE_MATCHING_BAD_FACTOR 4     /* matching: factor <= 0 */
#define CBA_FEATURE_SYMMETRY_OUTSIDE_IMAGE 5
#define CBA_FEATURE_SYMMETRY_LEFT_WINDOW 6
#define CBA_FEATURE_SYMMETRY_NOT_CONVERGED 7

typedef struct cba_feature_refiner cba_feature_refiner;

/* samples_xy: n_samples points (x, y) in [-1, 1]^2, scaled by window_half_extent; the matching stage uses the first n_samples / 8.
 * CBA_ERR_ARG (before any device call): a NULL pointer, width or height < 2, window_half_extent < 1, n_samples < 8, a refinement
 * type other than 0 and 2. */
int cba_feature_refiner_create(int32_t width, int32_t height, int32_t window_half_extent, int32_t refinement_type, int32_t n_samples,
                               const float* samples_xy, int32_t device, cba_feature_refiner** out);
void cba_feature_refiner_destroy(cba_feature_refiner* r);
/* Uploads width x height bytes (row-major, densely packed) and computes the gradient image; both stay resident.
 * gradient(x, y) = ((I(px, y) - I(mx, y)) / (px - mx), (I(x, py) - I(x, my)) / (py - my)), neighbours clamped into the image. */
int cba_feature_refiner_set_image(cba_feature_refiner* r, const uint8_t* gray_u8);
/* 2 width height floats (dx, dy per pixel) */
int cba_feature_refiner_get_gradient(cba_feature_refiner* r, float* float2_out);
/* Both stages for n predictions in one call.  positions: 2 n; local_pixel_tr_pattern: 9 n, row-major, the homography from pattern
 * offsets to pixel offsets at each feature (its inverse is the fp64 adjugate divided by the determinant, rounded to fp32).
 * Outputs: matched_positions 2 n (after the matching stage), positions_out 2 n, final_cost n (the symmetry cost), status n.
 * A feature whose matching stage fails skips the symmetry stage; a failed feature has NaN positions (matched_positions too when the
 * matching stage failed) and final_cost -1.  n = 0 launches nothing.  CBA_ERR_ARG: a NULL pointer (with n > 0), n < 0, no image. */
int cba_feature_refiner_refine(cba_feature_refiner* r, int32_t n, int32_t num_star_segments, const float* positions,
                               const float* local_pixel_tr_pattern, float* matched_positions, float* positions_out, float* final_cost,
                               int32_t* status);
/* Device time (events on the engine's stream) of the two kernels of the last cba_feature_refiner_refine with n > 0, without its
 * transfers.  CBA_ERR_ARG before such a call. */
int cba_feature_refiner_last_kernel_seconds(cba_feature_refiner* r, double* seconds);
/* Tests only: ONE pass of one stage for one feature.  stage 0 = matching, 1 = symmetry; with_jacobian 1 = the Jacobian pass, 0 = the
 * cost pass.  state: matching (x, y, factor, bias), symmetry the first 8 entries of pixel_tr_pattern_samples; NULL = the stage's
 * initial state at `position` (matching: with the closed-form factor and bias).  Outputs (each may be NULL):
 *   state_out  4 or 8 floats: the state of the pass
 *   rendered   n_samples / 8 floats: the rendered pattern (matching)
 *   valid      per sample of the stage (n_samples / 8 or n_samples) 1 when inside the image; an invalid sample has no record
 *   residual   2 per sample (the second one: GradientsXY); jacobian  16 per sample: two rows of 8 (matching: 4 of the first row)
 *   sums       45 doubles: cost, b, the upper triangle of H row by row (matching: 15; the cost pass: sums[0])
 *   pass_ok    0 when a sample was outside the image */
int cba_feature_refiner_debug_pass(cba_feature_refiner* r, int32_t stage, int32_t with_jacobian, int32_t num_star_segments,
                                   const float* position, const float* local_pixel_tr_pattern, const float* state, float* state_out,
                                   float* rendered, uint8_t* valid, float* residual, float* jacobian, double* sums, int32_t* pass_ok);

#ifdef __cplusplus
}
#endif
#endif /* CBA_FEATURES_H_ */
