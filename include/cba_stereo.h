/*
 * cba_stereo.h -- dense two-view stereo depth for a calibrated generic rig with libcalib_ba_hip.so: PatchMatch stereo in the
 * unrectified images of two central-generic cameras, after the reference's --stereo_depth_estimation tool
 * (APP/tools/stereo_depth_estimation.cc over libvis/cuda/patch_match_stereo*).  A header of its own next to cba_undistort.h.
 * Error codes and conventions are cba.h's.
 *
 * NO REFERENCE-PRODUCED VECTOR CAN EXIST (the reference draws from curand, and its propagation reads neighbours while other threads
 * write them), so this header is the definition, and it FIXES THE ARITHMETIC: float = IEEE binary32, every operation rounded on its
 * own, nothing contracted, division and square root correctly rounded.  A float32 numpy restatement reproduces every bit.
 *
 * INPUTS OF A HANDLE
 *   reference image W x H and stereo image Ws x Hs, 8 bit, 1 channel, row-major.
 *   unprojection   2 W H floats: per reference pixel centre (x + 0.5, y + 0.5) the (dx / dz, dy / dz) of its direction, NaN where
 *                  Unproject fails or dz <= 0.
 *   the projector of the stereo camera: a pinhole grid (fx, fy, cx, cy in the pixel-corner convention, PW x PH) and
 *   projection     2 PW PH floats: the stereo-image position, pixel-centre convention, of the ray through grid pixel centre
 *                  (u + 0.5, v + 0.5), NaN where it fails: map_xy of cba_model_undistortion_map with the identity rotation.  The
 *                  reference projects each sample with a Gauss-Newton iteration instead (pixel_corner_projector.cuh:371-478); the
 *                  table is "only approximate" in the way the reference's own un-projection lookup is.
 *   stereo_tr_reference   12 floats, row-major 3 x 4.
 * STATE, on the device: inv_depth (float, W H), normal (2 x int8, W H), cost (float, W H), and second buffers for the ping-pong.
 * INNER REGION: r <= x <= W - 1 - r, r <= y <= H - 1 - r, r = context_radius.  Nothing outside it is a hypothesis or a neighbour; the
 * state outside it is never changed.
 *
 * lerp(a, b, w) = a + w * (b - a).  bilinear(T, n_x, n_y, px, py), the remap's rule (cba_undistort.h): x0 = floorf(px), wx = px - x0,
 * x1 = x0 + 1, both indices clamped into [0, n_x - 1], y alike; lerp(lerp(T00, T10, wx), lerp(T01, T11, wx), wy); bytes as floats.
 *
 * COST of a hypothesis (inv_depth, normal q) at pixel (x, y)  (patch_match_stereo_cost.cuh:138-227 with the changes named here)
 *   unless inv_depth >= 1e-5f the cost is NaN.
 *   n = (qx / 127.f, qy / 127.f), nz = -sqrtf(max(0, (1 - nx nx) - ny ny)); depth = 1 / inv_depth; c = unprojection[y W + x];
 *   plane_d = ((c.x depth) nx + (c.y depth) ny) + depth nz.
 *   81 samples, OUR OWN 9 x 9 GRID (the reference's table of sample positions is not copied): for j = 0..8 (outer), i = 0..8:
 *   (ox, oy) = (r ((i - 4) / 4.f), r ((j - 4) / 4.f)), p = (x + ox, y + oy).
 *     reference side: g = bilinear(unprojection, W, H, p) per component, rv = bilinear(reference image, W, H, p).
 *     pd = plane_d / ((g.x nx + g.y ny) + nz); P = (g.x pd, g.y pd, pd); t_k = ((M[k][0] P.x + M[k][1] P.y) + M[k][2] P.z) + M[k][3].
 *     valid only if t_z > 0;  a = (fx (t_x / t_z) + cx) - 0.5f, b alike, valid only if 0 <= a <= PW - 1 and 0 <= b <= PH - 1;
 *     s = bilinear(projection, PW, PH, (a, b)) per component (NaN in any of the four entries gives NaN), valid only if
 *     0 <= s.x <= Ws - 1 and 0 <= s.y <= Hs - 1;  sv = bilinear(stereo image, Ws, Hs, s).
 *     One invalid sample (any comparison above that is false, NaN included) makes the cost NaN.
 *     sum_a += sv, sq_a += sv sv, sum_b += rv, sq_b += rv rv, prod += sv rv   (five float sums in sample order)
 *   k = 1.f / 81; num = prod - k (sum_a sum_b); den_a = sq_a - (k sum_a) sum_a; den_b = sq_b - (k sum_b) sum_b;
 *   cost = 1 where den_a < 0.1f or den_b < 0.1f, else 0.5f (1 - num / sqrtf(den_a den_b))   (sqrt and a division: the reference's
 *   rsqrtf is not correctly rounded).
 *
 * RANDOM NUMBERS  u(stage, pass, p, draw) = (mix(mix(mix(seed + 4 pass + stage) + p) + draw) >> 40) * 2^-24, p = y W + x, mix the
 * generator of cba_model_localization_accuracy (64-bit wrapping sums), stage 0 = init, 1 = mutation.
 *
 * PROPOSED NORMALS  a float normal (nx, ny) is clamped (l = sqrtf(nx nx + ny ny); if l > max_normal_2d_length both are multiplied
 * by max_normal_2d_length / l) and QUANTISED TO int8 BY TRUNCATION OF 127.f n BEFORE ITS COST IS EVALUATED: a stored cost is always
 * the cost of the stored state (the reference stores the cost of the unquantised normal).
 * ACCEPTANCE  proposals are visited in order; one whose cost is not NaN and not >= the cost held so far replaces it.
 *
 * STAGES, one launch over the inner region each; inv_min = 1.f / min_depth, inv_max = 1.f / max_depth
 *   init (kernel_init.cu:42-89)           n = (u0 - 0.5f, u1 - 0.5f), inv_depth = inv_max + (inv_min - inv_max) u2, and its cost (may be NaN).
 *   mutation (kernel_mutation.cu:66-126)  step = 0.5^min(pass + 1, 6) (inv_min - inv_max); d' = max(1e-5f, fabsf(d + step (u0 - 0.5f)));
 *                                         n' = (qx / 127.f + (u1 - 0.5f), qy / 127.f + (u2 - 0.5f)); proposals (d', n'), (d', n), (d, n'),
 *                                         ALL FROM THE SAME CURRENT STATE (the reference: three launches, each from the last one's result).
 *   propagation (kernel_propagation.cu:42-103)  neighbours (dx, dy) = (0, -1), (-1, 0), (1, 0), (0, 1); one outside the inner region is
 *                                         skipped (the reference reads uninitialised memory).  With the neighbour's (d_o, n_o) and
 *                                         o = unprojection at the neighbour: od = 1 / d_o, pl = ((o.x od) n_o.x + (o.y od) n_o.y) + od n_o.z,
 *                                         proposal (((c.x n_o.x + c.y n_o.y) + n_o.z) / pl, q_o).  NEIGHBOURS ARE READ FROM THE STATE
 *                                         BEFORE THE LAUNCH, results go to the second buffers, which then become the state.
 *   refinement (kernel_refinement.cu:42-79)  k = 0..19: ((1 + (0.02f * 2) ((k / 19.f) - 0.5f)) d, q).
 *   match = init (pass 0), then for it = 0 .. iterations - 1: mutation (pass it), propagation; then refinement.
 *
 * FILTER  one launch writes inv_depth, or 0 where invalid and 0 outside the inner region.  Valid needs all of:
 *   cost <= cost_threshold (NaN fails);  inv_depth > inv_max;
 *   the angle test ON THE STORED PLANE NORMAL (the reference estimates one from depth differences):
 *     ((nx c.x + ny c.y) + nz) / sqrtf((c.x c.x + c.y c.y) + 1) <= -(float)cos((double)angle_threshold);
 *   with another direction's map (Ws x Hs), kernel_consistency.cu:42-97: depth = 1 / inv_depth, t = M (depth c.x, depth c.y, depth),
 *     t_z > 0, s = the projection of t as in the cost, q = (s.x + 0.5f, s.y + 0.5f) with r <= q.x < Ws - 1 - r, r <= q.y < Hs - 1 - r,
 *     l = other[(int)q.y Ws + (int)q.x] != 0, f = t_z l, f = 1 / f if f < 1, f <= lr_consistency_factor_threshold.
 * Small connected components are removed by the caller on the host, or by the COMPONENTS stage below.
 *
 * POST-PROCESSING (declared in cba_stereo_post.h; libvis/cuda/patch_match_stereo.cu and ComputeDepthMap's order: median, the FILTER
 * above, bilateral, hole filling, components).  "Invalid" is inv_depth == 0.  Every stage reads one map and writes another and never
 * reads what its own launch writes.  A pixel outside the inner region ALWAYS GETS 0 (and cost NaN where a cost is written): the one
 * exception to "the state outside it is never changed" is cba_stereo_finish, whose median leaves 0 / NaN there.  The arithmetic rule
 * above holds; the one operation outside it is the bilateral's fp64 exp.
 *   MEDIAN (:41-143, without the second-best cost)  an invalid inner pixel stays invalid, cost NaN.  Otherwise gather (inv_depth,
 *     cost) pairs: THE CENTRE FIRST, then the valid ones of its eight neighbours THAT LIE IN THE INNER REGION in row-major order (dy
 *     outer, dx inner).  Partial selection: for i = 0..4, for k = i + 1 .. count - 1: swap pairs i and k if d[i] > d[k], STRICTLY (a
 *     tie never swaps, so among equal depths the gather order decides whose cost is taken).  Odd count: entry count / 2.  Even count:
 *     avg = 0.5f (d[count/2 - 1] + d[count/2]); the lower entry only if fabsf(avg - lower) < fabsf(avg - upper), else the upper one
 *     (so the upper one when both are equally near).  The cost written is the chosen entry's; it may be NaN.
 *   BILATERAL (:172-225)  radius = (int)(radius_factor sigma_xy + 0.5f), denom_xy = (2.f sigma_xy) sigma_xy, denom_v = (2.f sigma_v)
 *     sigma_v.  An invalid centre stays 0.  Otherwise the samples of the window [x - radius, x + radius] x [y - radius, y + radius]
 *     CLIPPED TO THE IMAGE (not to the inner region: after the FILTER the map is 0 outside it anyway) are visited in row-major order;
 *     those with g = dx dx + dy dy > radius radius and the invalid ones are skipped.  For the others v = centre - sample,
 *     a = (-(float)g / denom_xy) + (-(v v) / denom_v), w = (float)exp((double)a), sum += w sample, weight += w (float sums; the
 *     centre itself has w = 1, so weight is never 0).  Result sum / weight.  DEVIATION: the reference calls CUDA's float exp.  Two
 *     fp64 exp implementations may differ in the last place, so this stage alone is not bit-reproducible against numpy.
 *   FILL_HOLES, one round (:254-328)  a valid inner pixel keeps its value.  For an invalid one, over its valid 8-neighbours THAT LIE
 *     IN THE INNER REGION in row-major order: avg = (float sum) / (float)count (no valid neighbour: 0 / 0 = NaN, and the pixel stays 0);
 *     then over the same neighbours f = d / avg, f = 1 / f if f < 1, and those with f <= 1.01f are summed and counted again; with at
 *     least 6 of them the pixel gets sum / (float)count, else it stays 0.  The reference runs over the image minus a one-pixel rim;
 *     its input is 0 outside the inner region, where a pixel has at most three neighbours inside and can never be filled: the same
 *     rule, and nothing outside the inner region is touched.
 *   COMPONENTS  4-connectivity inside the inner region; a valid pixel a and its valid right or lower neighbour b are joined if
 *     q = a / b, q = 1 / q if q < 1, q < similar_depth_ratio, STRICTLY; components of fewer than min_component_size pixels are set to 0
 *     (stereo.remove_small_components is the same rule on the host).  Labels are unions by integer atomicMin on roots (a component's
 *     label is its smallest pixel index), a compression pass, integer atomicAdd counts per root and a clearing pass: integer atomics
 *     only, so the result does not depend on scheduling.
 *
 * NOT BUILT: the second-best pass, the epipolar-gradient and required-range tests, the reference's depth-difference normal in the
 * angle test, more than two views, masks, the thin-prism branch of the tool, non-central cameras.
 */
#ifndef CBA_STEREO_H_
#define CBA_STEREO_H_
#include "cba.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
  int32_t context_radius;                  /* r >= 1, W >= 2 r + 1, H >= 2 r + 1 */
  int32_t iterations;                      /* of cba_stereo_match, >= 0 */
  float min_depth, max_depth;              /* 0 < min_depth < max_depth */
  float max_normal_2d_length;
  float cost_threshold, angle_threshold, lr_consistency_factor_threshold;      /* the filter's */
  uint64_t seed;
} cba_stereo_options;

enum { CBA_STEREO_INIT = 0, CBA_STEREO_MUTATION = 1, CBA_STEREO_PROPAGATION = 2, CBA_STEREO_REFINEMENT = 3 };

/* Every call: CBA_ERR_ARG before any device call for a NULL pointer, r < 1, W < 2 r + 1 or H < 2 r + 1, iterations < 0,
 * min_depth <= 0 or min_depth >= max_depth (NaN included), max_normal_2d_length outside (0, 1] (beyond 1 an int8 could not hold
 * 127 n), non-finite grid parameters, sizes < 1, an unknown stage, pass < 0.
 * Launches go to the null stream of the handle's device; cba_stereo_run_stage and cba_stereo_match return without waiting. */
typedef struct cba_stereo cba_stereo;
int cba_stereo_create(int32_t width, int32_t height, int32_t stereo_width, int32_t stereo_height, const float* unprojection,
                      float fx, float fy, float cx, float cy, int32_t grid_width, int32_t grid_height, const float* projection,
                      const float* stereo_tr_reference, int32_t device, cba_stereo** out);
void cba_stereo_destroy(cba_stereo* s);
int cba_stereo_set_images(cba_stereo* s, const uint8_t* reference_image, const uint8_t* stereo_image);
int cba_stereo_set_pose(cba_stereo* s, const float* stereo_tr_reference);
int cba_stereo_match(cba_stereo* s, const cba_stereo_options* o);
/* the whole arrays (W H, 2 W H, W H); a new handle's state is all zero */
int cba_stereo_get_state(cba_stereo* s, float* inv_depth, int8_t* normal, float* cost);
int cba_stereo_set_state(cba_stereo* s, const float* inv_depth, const int8_t* normal, const float* cost);
/* exactly one stage; pass is the generator's pass word, and for the mutation also the iteration of its step range */
int cba_stereo_run_stage(cba_stereo* s, const cba_stereo_options* o, int32_t stage, int32_t pass);
/* cost (W H, 0 outside the inner region) of a given state; the handle's state is not touched */
int cba_stereo_cost(cba_stereo* s, const cba_stereo_options* o, const float* inv_depth, const int8_t* normal, float* cost);
/* other_inv_depth: stereo_width x stereo_height floats, or NULL for no left-right check; out: W H floats */
int cba_stereo_filter(cba_stereo* s, const cba_stereo_options* o, const float* other_inv_depth, float* out);

#ifdef __cplusplus
}
#endif
#endif /* CBA_STEREO_H_ */
