/*
 * cba_stereo_post.h -- the post-processing of a cba_stereo handle's depth map on the device: 3 x 3 median, bilateral filter, hole
 * filling, removal of small connected components, and the whole chain of the reference's ComputeDepthMap after the matching.
 * THE DEFINITION OF EVERY STAGE IS THE "POST-PROCESSING" SECTION OF cba_stereo.h; this header holds the declarations only (a header of
 * its own, as cba_stereo.h is next to cba_undistort.h).  Error codes and conventions are cba.h's.
 */
#ifndef CBA_STEREO_POST_H_
#define CBA_STEREO_POST_H_
#include "cba_stereo.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {                   /* 0 selects the default of every member */
  float bilateral_sigma_xy;        /* 1.5f */
  float bilateral_radius_factor;   /* 2.0f */
  float bilateral_sigma_inv_depth; /* 0.005f */
  int32_t hole_filling_iterations; /* 3; -1 = none; at most 64 */
  int32_t min_component_size;      /* 50 (the tool's); -1 = keep every component */
  float similar_depth_ratio;       /* 1.005f (the tool's) */
} cba_stereo_post_options;

enum { CBA_STEREO_POST_MEDIAN = 0, CBA_STEREO_POST_BILATERAL = 1, CBA_STEREO_POST_FILL_HOLES = 2, CBA_STEREO_POST_COMPONENTS = 3 };
enum { CBA_STEREO_POST_MAX_RADIUS = 32, CBA_STEREO_POST_MAX_HOLE_FILLING_ITERATIONS = 64 };

/* Both calls: CBA_ERR_ARG before any device call for what cba_stereo.h's calls refuse, a NULL pointer (cost_in and cost_out may be
 * NULL except for the median; other_inv_depth may be NULL), an unknown stage, a sigma or radius factor that is (after the default is
 * put in) not finite or not positive, a bilateral radius above CBA_STEREO_POST_MAX_RADIUS, hole_filling_iterations < -1 or above
 * CBA_STEREO_POST_MAX_HOLE_FILLING_ITERATIONS, min_component_size < -1, similar_depth_ratio < 1 or NaN.  Both return after the
 * download of their result. */

/* one stage on caller-given maps (W H floats each); the handle's state is not touched; cost_in / cost_out only for MEDIAN;
 * FILL_HOLES is one round whatever hole_filling_iterations says */
int cba_stereo_post_stage(cba_stereo* s, const cba_stereo_options* o, const cba_stereo_post_options* po, int32_t stage,
                          const float* inv_depth_in, const float* cost_in, float* inv_depth_out, float* cost_out);

/* the whole chain on the device: median of the state (the state's inv_depth and cost become the filtered ones, normals stay),
 * the filter of cba_stereo_filter with other_inv_depth (stereo_width x stereo_height floats, may be NULL), bilateral, hole filling,
 * components; out: W H floats.  No intermediate map leaves the device. */
int cba_stereo_finish(cba_stereo* s, const cba_stereo_options* o, const cba_stereo_post_options* po,
                      const float* other_inv_depth, float* out);

#ifdef __cplusplus
}
#endif
#endif /* CBA_STEREO_POST_H_ */
