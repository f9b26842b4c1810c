/* emap_field_hip.h - the exact distance field of an edge set: line segments and cubic Beziers expanded into one segment table, the
 * distance of every point to the nearest segment with that segment and the foot parameter, and the statistics of such distances
 * (threshold counts, per-edge counts, the sum and the maximum).  A sixth header of libemap_hip.so with its own version, bound by its
 * own table (emap_amd/_lib.py: FIELD_SYMBOLS, field_lib(), field_api()).  emap_hip.h, emap_eval_hip.h, emap_fit_hip.h,
 * emap_raster_hip.h and emap_score_hip.h, their symbol sets and their versions are unchanged by anything declared here.
 *
 * Conventions are emap_hip.h's: C linkage, return value 0 = ok or a negative EMAP_E_* with the text in emap_last_error() (one
 * thread-local text for all headers), device pointers unless a parameter is named *_host, `stream` is a hipStream_t (NULL: the
 * default stream), every call is asynchronous on it, no entry point allocates or synchronises.
 *
 * All arithmetic is IEEE fp64, one rounding per operation in the grouping written below, with no FMA contraction and no
 * floating-point atomic.  Every output is a pure function of the inputs, bit-identical from run to run and independent of what the
 * output buffers and the workspace held before.  The numpy restatement is tests/edge_field_ref.py.
 *
 * A SEGMENT TABLE is  segs (n_seg, 2, 3) doubles - the end points a, b of every segment -  and  seg_edge (n_seg) int32 - the edge
 * a segment belongs to.  The chord polyline of a curve IS the curve for everything declared here: distances are exact to the
 * table, not to the cubic.
 */
#ifndef EMAP_FIELD_HIP_H
#define EMAP_FIELD_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "emap_hip.h" /* EMAP_OK, EMAP_E_INVALID, EMAP_E_LAUNCH; emap_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

#define EMAP_FIELD_ABI_VERSION 1
int emap_field_abi_version(void);

#define EMAP_FIELD_MAX_CURVE_SEGMENTS 256 /* chords per curve */
#define EMAP_FIELD_MAX_SEGMENTS 1048576   /* n_seg: 1 << 20 */
#define EMAP_FIELD_MAX_POINTS 2147483647  /* n of a call */
#define EMAP_FIELD_MAX_THRESHOLDS 8       /* K */
#define EMAP_FIELD_POINTS_F64 0           /* points_dtype: (n, 3) double */
#define EMAP_FIELD_POINTS_F32 1           /* points_dtype: (n, 3) float, widened exactly */

/* The segment table of n_lines segments  lines (n_lines, 2, 3)  and n_curves cubic Beziers  curves (n_curves, 4, 3), doubles:
 *   segs (n_seg, 2, 3) double out,  seg_edge (n_seg) int32 out,   n_seg = n_lines + n_curves * curve_segments.
 * A line is one segment.  Curve j is curve_segments = n chords, chord k from B(t_k) to B(t_k+1), t_k = (double)k / (double)n, and with
 * u = 1 - t
 *     b0 = (u u) u,  b1 = (3 (u u)) t,  b2 = (3 u) (t t),  b3 = (t t) t,     B(t) = (b0 P0 + b1 P1) + (b2 P2 + b3 P3)   per coordinate
 * - the formula and the grouping of emap_raster_hip.h, so that B(0) = P0 and B(1) = P3 exactly and the table is the rasteriser's.
 * Segments are numbered lines first, then curve by curve, k ascending; edge e < n_lines is line e, edge n_lines + j is curve j.
 * One launch, one thread per segment.
 *
 * EMAP_E_INVALID before any launch ("field_expand_edges:" leads the text): n_lines < 0 or n_curves < 0; curve_segments outside
 * [1, EMAP_FIELD_MAX_CURVE_SEGMENTS]; n_seg outside [1, EMAP_FIELD_MAX_SEGMENTS]; a NULL lines with n_lines > 0, a NULL curves with
 * n_curves > 0, a NULL segs or seg_edge. */
int emap_field_expand_edges(const double* lines, int n_lines, const double* curves, int n_curves, int curve_segments, double* segs,
                            int32_t* seg_edge, void* stream);

/* Bytes of the workspace of emap_field_point_distances(n points, n_seg segments, split): 0 when the segments are taken in ONE part, else
 * parts * n * 20 rounded up to a multiple of 256 - per part and point the squared distance, the foot parameter and the segment index.
 * The number of parts is `split` (0: chosen for the current device), at most the number of segment tiles, no part empty.
 * EMAP_E_INVALID ("field_workspace_bytes:" leads the text): n outside [0, EMAP_FIELD_MAX_POINTS]; n_seg outside
 * [1, EMAP_FIELD_MAX_SEGMENTS]; split < 0; a NULL bytes_host. */
int emap_field_workspace_bytes(int64_t n, int n_seg, int split, size_t* bytes_host);

/* For every point p of  points (n, 3)  of points_dtype the nearest segment of  segs (n_seg, 2, 3).  For p and a segment a -> b, per
 * coordinate and in this grouping:
 *
 *     u  = b - a
 *     uu = (ux ux + uy uy) + uz uz
 *     r  = uu == 0 ? 0 : 1.0 / uu                        one IEEE division per SEGMENT, not per pair
 *     q  = ((px - ax) ux + (py - ay) uy) + (pz - az) uz
 *     tt = fmin(fmax(q r, 0), 1)                          fmax(x, 0) = x > 0 ? x : +0  and  fmin(x, 1) = x < 1 ? x : 1: a NaN gives +0
 *     e  = p - (a + tt u)
 *     d2 = (ex ex + ey ey) + ez ez
 *
 *   d2 (n) double out, seg (n) int32 out, t (n) double out: the lexicographic minimum of (d2, segment index) over all segments and that
 *   segment's tt.  A candidate wins only by d2 < best, or by equal d2 with a lower index, and the first candidate whose d2 is not a NaN
 *   wins against nothing: a NaN never wins, +inf can.  A point for which no segment wins - a NaN coordinate in the point, or in every
 *   segment - gets seg = -1, t = 0, d2 = NaN.
 *
 *   split      0 (automatic) or the forced number of parts the segments are divided into across workgroups; it never changes a bit of
 *              the result
 *   workspace  workspace_bytes >= what emap_field_workspace_bytes(n, n_seg, split) reports, 16-byte aligned; may be NULL when that is 0
 *
 * One launch with one part; with several, one launch that leaves every part's winner in the workspace and one that takes their
 * lexicographic minimum.  n = 0 is valid and launches nothing.
 *
 * EMAP_E_INVALID before any launch ("field_point_distances:" leads the text): what emap_field_workspace_bytes rejects; a points_dtype
 * that is neither code; with n > 0 a NULL points, segs, d2, seg or t, or a workspace that is NULL, misaligned or too small when one is
 * needed. */
int emap_field_point_distances(const void* points, int points_dtype, int64_t n, const double* segs, int n_seg, int split, double* d2,
                               int32_t* seg, double* t, void* workspace, size_t workspace_bytes, void* stream);

/* Statistics of n squared distances  d2 (n)  double, with  t_k = thresholds_host[k]:
 *
 *   counts (1 + K) int64 out:  column 0 is n; column 1 + k how many elements have  d2 < t_k * t_k  - strict, one fp64 multiplication; a
 *                              NaN is never counted
 *   sums (2) double out:       sums[0] the sum of sqrt(d2) in a fixed order: element i belongs to thread i mod 1024, which adds its
 *                              elements in ascending i starting from 0.0; the 1024 partial sums are then added in a binary tree, partial
 *                              t + s into partial t for s = 512, 256, ..., 1.  A NaN element makes it NaN.  sums[1] the maximum of the
 *                              elements that are not NaN, 0 when there is none
 *   edge_counts (n_ids, 1 + K) int64 out, or NULL;  ids (n) int32, required with edge_counts when n > 0 and NULL without it: per id the
 *                              number of elements with that id (column 0) and how many of them are within each threshold.  An element
 *                              whose id is outside [0, n_ids) counts only globally.  n_ids is ignored without edge_counts
 *
 * Every element of counts, sums and edge_counts is written.  All counting is in integers (integer atomics; an edge_counts too large for
 * the workgroup's LDS is set to 0 by a first launch and updated in place); one workgroup.  n = 0 is valid: zeros.
 *
 * EMAP_E_INVALID before any launch ("field_stats:" leads the text): n outside [0, EMAP_FIELD_MAX_POINTS]; K outside
 * [1, EMAP_FIELD_MAX_THRESHOLDS]; a NULL thresholds_host; a t_k that is negative or not finite; a NULL counts or sums; a NULL d2 with
 * n > 0; ids without edge_counts, or edge_counts without ids when n > 0; n_ids < 1 with edge_counts. */
int emap_field_stats(const double* d2, const int32_t* ids, int n_ids, const double* thresholds_host, int K, int64_t n, int64_t* counts,
                     double* sums, int64_t* edge_counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif
