/* emap_score_hip.h - edge maps scored against edge maps in image space: the exact Euclidean distance transform of a stack of maps and
 * the per-frame and per-edge statistics read from it (pixel precision / recall / chamfer).  A fifth header of libemap_hip.so with its
 * own version, bound by its own table (emap_amd/_lib.py: SCORE_SYMBOLS, score_lib(), score_api()).  emap_hip.h, emap_eval_hip.h,
 * emap_fit_hip.h and emap_raster_hip.h, their symbol sets and their versions are unchanged by anything declared here.
 *
 * Conventions are emap_hip.h's: C linkage, return value 0 = ok or a negative EMAP_E_* with the text in emap_last_error() (one
 * thread-local text for all headers), device pointers unless a parameter is named *_host, `stream` is a hipStream_t (NULL: the
 * default stream), every call is asynchronous on it, no entry point allocates or synchronises.
 *
 * Distances are exact integers: no floating point enters d2.  The statistics count in integers; the one floating-point output
 * (sums) is a sum of IEEE fp64 square roots taken in an order the implementation fixes, with no FMA contraction and no
 * floating-point atomic.  Every output is a pure function of the inputs, bit-identical from run to run and independent of what the
 * output buffers and the workspace held before.  The numpy restatement is tests/edge_score_ref.py.
 */
#ifndef EMAP_SCORE_HIP_H
#define EMAP_SCORE_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "emap_hip.h" /* EMAP_OK, EMAP_E_INVALID, EMAP_E_LAUNCH; emap_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

#define EMAP_SCORE_ABI_VERSION 1
int emap_score_abi_version(void);

#define EMAP_SCORE_MAX_DIM 32768         /* h and w: (h - 1)^2 + (w - 1)^2 < 2^31 - 1, a squared distance is an exact int32 */
#define EMAP_SCORE_MAX_FRAMES 65535      /* F */
#define EMAP_SCORE_MAX_THRESHOLDS 8      /* K */
#define EMAP_SCORE_NONE 2147483647       /* d2 of a pixel whose frame has no SET pixel */
#define EMAP_SCORE_MAPS_U8 0             /* maps_dtype: (F, h, w) uint8 */
#define EMAP_SCORE_MAPS_F32 1            /* maps_dtype: (F, h, w) float */
#define EMAP_SCORE_WORKSPACE_PIXEL_BYTES 2 /* workspace bytes per pixel */

/* The mask of a map.  A pixel has the value v: for EMAP_SCORE_MAPS_F32 the float widened to double; for EMAP_SCORE_MAPS_U8 the byte b
 * gives  v = (double)(float)((double)b / 255.0)  - the table value of emap_amd.edge_raster.to_dataset_edges, so a byte map and its
 * float image have the same mask for every threshold.  The pixel is SET iff  v > threshold : the comparison is strict, a NaN is not
 * SET.  `threshold` is a finite double. */

/* Bytes of the workspace of emap_score_distance_maps:  F * h * w * EMAP_SCORE_WORKSPACE_PIXEL_BYTES  - one uint16 per pixel, the
 * column pass's result (below).  EMAP_E_INVALID ("score_workspace_bytes:" leads the text): F outside [1, EMAP_SCORE_MAX_FRAMES], h or w
 * outside [1, EMAP_SCORE_MAX_DIM], a NULL bytes_host. */
int emap_score_workspace_bytes(int F, int h, int w, size_t* bytes_host);

/* The exact squared Euclidean distance transform of every frame:
 *
 *     d2[f, y, x] = min over the SET pixels (y', x') of frame f of  (x - x')^2 + (y - y')^2      in integers,
 *
 * 0 on a SET pixel, and EMAP_SCORE_NONE everywhere in a frame without a SET pixel.  Frames are independent: a SET pixel of frame f
 * never influences another frame.
 *
 *   maps       (F, h, w) of maps_dtype;  d2 (F, h, w) int32 out
 *   workspace  workspace_bytes >= what emap_score_workspace_bytes reports, 16-byte aligned
 *
 * Two launches.  The column pass, one thread per (frame, x), sweeps y downwards and then upwards and leaves in the workspace
 * g[f, y, x] = min over SET (y', x) of |y - y'| as a uint16, 65535 for a column without a SET pixel; it reads the mask from `maps`.
 * The row pass, one workgroup per (frame, y), forms  min over x' of (x - x')^2 + g[f, y, x']^2  for every x.
 *
 * EMAP_E_INVALID before any launch ("score_distance_maps:" leads the text): what emap_score_workspace_bytes rejects; a maps_dtype that
 * is neither code; a threshold that is not finite; a NULL maps or d2; a workspace that is NULL, misaligned or too small. */
int emap_score_distance_maps(const void* maps, int maps_dtype, double threshold, int F, int h, int w, int32_t* d2, void* workspace,
                             size_t workspace_bytes, void* stream);

/* Statistics of the SET pixels of the maps A, read against the distance map d2_b of another set B (emap_score_distance_maps of B's
 * maps).  For every frame f, over the SET pixels p of maps_a[f] with d = d2_b[f, p]:
 *
 *   counts (F, 1 + K) int64 out:  column 0 the number of SET pixels; column 1 + k how many of them have  d != EMAP_SCORE_NONE  and
 *                                 (double)d <= t_k * t_k,  t_k = thresholds_host[k]  (one fp64 multiplication)
 *   sums   (F) double out:        the sum of sqrt((double)d), a pixel with d == EMAP_SCORE_NONE contributing +inf; 0 for a frame
 *                                 without a SET pixel.  The order of the summation is fixed: pixel i = y w + x of the frame belongs to
 *                                 thread i mod 1024, which adds its pixels in ascending i; the 1024 partial sums are then added in a
 *                                 binary tree, partial t + s into partial t for s = 512, 256, ..., 1
 *   ids (F, h, w) int32 and edge_counts (n_ids, 1 + K) int64 out: both NULL or both given.  ids is what emap_raster_edges writes;
 *                                 edge_counts holds the same two kinds of count per id, pooled over the frames.  A SET pixel whose
 *                                 id is outside [0, n_ids) is counted for its frame and for no edge.  n_ids is ignored without ids
 *
 * Every element of counts, sums and edge_counts is written.  All counting is in integers (integer atomics for edge_counts, which a
 * first launch sets to 0); one workgroup per frame.
 *
 * EMAP_E_INVALID before any launch ("score_stats:" leads the text): F, h or w out of range; an a_dtype that is neither code; an
 * a_threshold that is not finite; K outside [1, EMAP_SCORE_MAX_THRESHOLDS]; a NULL thresholds_host; a t_k that is negative or not
 * finite; a NULL maps_a, d2_b, counts or sums; ids without edge_counts or edge_counts without ids; n_ids < 1 with ids. */
int emap_score_stats(const void* maps_a, int a_dtype, double a_threshold, const int32_t* d2_b, const int32_t* ids, int n_ids,
                     const double* thresholds_host, int K, int F, int h, int w, int64_t* counts, double* sums, int64_t* edge_counts,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif
