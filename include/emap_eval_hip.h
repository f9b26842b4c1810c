/* emap_eval_hip.h - the evaluation entry points of libemap_hip.so that came after ABI 12 of emap_hip.h: a second header with its own
 * version, bound by its own table (emap_amd/_lib.py: EVAL_SYMBOLS, eval_lib(), eval_api()).  emap_hip.h, its symbol set and
 * EMAP_ABI_VERSION are unchanged by anything declared here.
 *
 * Conventions are emap_hip.h's: C linkage, return value 0 = ok or a negative EMAP_E_* with the text in emap_last_error() (one
 * thread-local text for both headers), device pointers unless a parameter is named *_host, `stream` is a hipStream_t (NULL: the
 * default stream), every call is asynchronous on it, no entry point allocates and none needs a workspace.
 */
#ifndef EMAP_EVAL_HIP_H
#define EMAP_EVAL_HIP_H

#include <stdint.h>
#include "emap_hip.h" /* EMAP_OK, EMAP_E_INVALID, EMAP_E_LAUNCH; emap_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

#define EMAP_EVAL_ABI_VERSION 1
int emap_eval_abi_version(void);

/* dtype codes of emap_point_visibility */
#define EMAP_EVAL_POINTS_F64 0
#define EMAP_EVAL_POINTS_F32 1 /* widened to double exactly */
#define EMAP_EVAL_MAPS_U8 0    /* strength = g / 255.0 in double; with invert 1.0 - g / 255.0 */
#define EMAP_EVAL_MAPS_F32 1   /* strength = the value widened to double; invert is not applied */
#define EMAP_EVAL_MAPS_F64 2   /* strength = the value; invert is not applied */

/* Multi-view visibility of a point cloud (the per-point body of compute_visibility, scripts/get_gt_points_DTU.py:94-128 of the
 * reference): for each of n points the number of the F frames in which the point projects onto an edge pixel.
 *
 *   points   (n, 3) row-major, fp64 or fp32 by points_dtype
 *   K, R, T  (F, 3, 3), (F, 3, 3), (F, 3) doubles: intrinsics and the WORLD-TO-CAMERA rotation and translation of every frame
 *   maps     (F, h, w) row-major, uint8 / float32 / float64 by maps_dtype
 *   count    (n) int32 out: frames that count;  mask (n) uint8 out, or NULL: 1 where count > min_frames, else 0
 *
 * Per point X and frame, all in fp64 with no FMA contraction and every 3-term sum taken left to right:
 *   c = R X + T,  p = K c,  u = rint(p0 / p2),  v = rint(p1 / p2)      (half to even, as numpy's round)
 * The frame counts when 0 <= u < w and 0 <= v < h - tested on the doubles, so a NaN or infinite coordinate (p2 == 0 among them) is
 * outside - and strength[v, u] > threshold.  There is no depth test: a point behind the camera that lands in the image counts.
 * The result is a pure function of the inputs: one thread per point keeps its count in a register, there are no atomics and no
 * (n, F) intermediate, and neither n, the launch shape nor the previous contents of count / mask change a bit of it.
 *
 * EMAP_E_INVALID before any launch, with "point_visibility:" leading emap_last_error(): n < 0, F <= 0, h <= 0 or w <= 0, an
 * unknown dtype code, or with n > 0 a NULL points / K / R / T / maps / count.  n == 0 returns 0 and launches nothing. */
int emap_point_visibility(const void* points, int points_dtype, int64_t n, const double* K, const double* R, const double* T,
                          const void* maps, int maps_dtype, int F, int h, int w, int invert, double threshold, int min_frames,
                          int32_t* count, uint8_t* mask, void* stream);

#ifdef __cplusplus
}
#endif
#endif
