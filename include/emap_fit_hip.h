/* emap_fit_hip.h - the edge-fitting entry points of libemap_hip.so: a third header with its own version, bound by its own table
 * (emap_amd/_lib.py: FIT_SYMBOLS, fit_lib(), fit_api()).  emap_hip.h and emap_eval_hip.h, their symbol sets and their versions are
 * unchanged by anything declared here.
 *
 * Conventions are emap_hip.h's: C linkage, return value 0 = ok or a negative EMAP_E_* with the text in emap_last_error() (one
 * thread-local text for all headers), device pointers unless a parameter is named *_host, `stream` is a hipStream_t (NULL: the
 * default stream), every call is asynchronous on it, no entry point allocates.
 *
 * All device arithmetic is fp64 with no FMA contraction; every 3-term sum is (x + y) + z; no result is formed by an atomic.  Every
 * output is a pure function of the inputs, bit-identical from run to run.  The numpy restatement of every entry point, in the same
 * scalar order, is tests/edge_fitting_ref.py.
 */
#ifndef EMAP_FIT_HIP_H
#define EMAP_FIT_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "emap_hip.h" /* EMAP_OK, EMAP_E_INVALID, EMAP_E_LAUNCH; emap_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

#define EMAP_FIT_ABI_VERSION 1
int emap_fit_abi_version(void);

#define EMAP_FIT_MAX_POLYLINE_POINTS 1024 /* points of one polyline of emap_fit_lines (they sit in LDS) */
#define EMAP_FIT_MAX_LINES 16             /* max_lines of emap_fit_lines */
#define EMAP_FIT_LINK_LDS_POINTS 1048576  /* emap_fit_link keeps its visited bits in LDS (128 KiB) up to this n, in vis_ws above it */

/* The greedy linking of connect_points (src/edge_extraction/edge_fitting/main.py:93-228 of the reference) in ONE launch of one workgroup.
 *
 *   points      (n, 6) doubles: position and unit line direction of every point
 *   cell_xyz    (n, 3) int32: the cell of every point in a uniform grid of gx x gy x gz cells whose edge is >= thr, every
 *               coordinate in [0, g) - any monotone map of the coordinates will do, the result does not depend on the grid
 *   cell_start  (gx gy gz + 1) int32, order (n) int32: the points sorted by cell index (cx gy + cy) gz + cz; cell c holds
 *               order[cell_start[c] .. cell_start[c + 1])
 *   chain       (3 n) int32 out, offsets (n + 1) int32 out: polyline k is chain[offsets[k] .. offsets[k + 1]), offsets[0] = 0
 *   count       (4) int32 out: [0] the number of polylines, [1] 0, or 1 if chain was too short (cannot happen: every appended point
 *               is marked visited or ends a direction of its walk) - the walk stops there, [2] the steps taken (the last, failing
 *               step of every direction included), [3] the seeds (kept and dropped polylines)
 *   vis_ws      ceil(n / 32) uint32 of workspace, needed when n > EMAP_FIT_LINK_LDS_POINTS or vis_global != 0; its contents on
 *               entry do not matter.  vis_global != 0 keeps the visited bits there at any n (the same result; for tests)
 *
 * Until no point is unvisited: the seed is the LOWEST unvisited index; it is marked visited and starts a polyline.  Forward steps from
 * the anchor s (the seed at first): the candidates are the unvisited points with dist < thr, dist = sqrt((dx dx + dy dy) + dz dz);
 * dir = (p - p_s) / (dist + 1e-6) per component, dot = (dir.x d_s.x + dir.y d_s.y) + dir.z d_s.z.  The winner has the largest dot,
 * the lowest index among equals; stop when there is none or dot_w <= 1 - angle.  The winner is appended; every candidate with
 * dist <= dist_w && dot < dot_w && dot >= nms dot_w is marked visited; if (d_w . dir_w) <= 0.5 the direction ends and the winner stays
 * UNvisited (it can be linked or seed again, as in the reference), otherwise it is marked visited and becomes the anchor.  Backward
 * steps start again from the seed: the winner has the smallest dot; stop when |dot_w| <= 1 - angle or dot_w >= 0; the marks are
 * dist <= dist_w && dot > dot_w && dot <= nms dot_w; the test is (-d_w . dir_w) <= 0.5; the winner is PREpended.  A polyline is kept
 * when it has more than 1 point (keep_short != 0) or more than 3; visited marks persist either way.  A candidate whose dot is NaN is
 * never a winner.  A step looks at the 27 cells around the anchor: its cost does not grow with n.  Every loop is bounded: at most n
 * steps per direction, at most n seeds.
 *
 * EMAP_E_INVALID before any launch ("fit_link:"): n outside 0..2^29, a grid dimension < 1 or gx gy gz > 2^30, thr not finite or <= 0, angle or
 * nms not finite, with n > 0 a NULL points / cell_xyz / cell_start / order / chain, a NULL offsets / count, a NULL vis_ws when it
 * is needed. */
int emap_fit_link(const double* points, int n, const int32_t* cell_xyz, const int32_t* cell_start, const int32_t* order, int gx, int gy,
                  int gz, double thr, double angle, double nms, int keep_short, int vis_global, int32_t* chain, int32_t* offsets,
                  int32_t* count, uint32_t* vis_ws, void* stream);

/* Exhaustive consensus line fit (fit_line_ransac_3d of edge_fitting/line_fit.py:52-161 as max_iterations -> infinity): one workgroup
 * per polyline, its points in LDS.
 *
 *   pts      (offsets[P], 3) doubles, offsets (P + 1) int32: polyline k is rows offsets[k] .. offsets[k + 1], at most
 *            EMAP_FIT_MAX_POLYLINE_POINTS of them (a longer one gets n_lines = -1 and labels -1: the caller checks before the call)
 *   segs     (P, max_lines, 6) doubles out: start and end point of every fitted line; unused rows are 0
 *   n_lines  (P) int32 out;  labels (offsets[P]) int32 out: the line of every point, -1 for a point that remains
 *
 * Per round, at most max_lines rounds while at least min_inliers points remain: over every pair i < j of the remaining points (in
 * their order) with |p_j - p_i| >= 1e-6, dir = (p_j - p_i) / |p_j - p_i|, count the remaining points with |cross(p - p_i, dir)| <
 * inlier_thr.  The largest count wins, the lexicographically lowest (i, j) among equals.  Stop if it is < min_inliers or
 * count / n_original < 1.0 / max_lines.  Otherwise: mean and 3 x 3 scatter matrix of the inliers (sums in their order), u = its
 * principal direction (cyclic Jacobi), oriented so that u . (last inlier - first inlier) >= 0; start = p_i + min(proj) u, end =
 * p_i + max(proj) u with proj = (p - p_i) . u over the inliers; the inliers get the round's line number and leave.
 *
 * EMAP_E_INVALID ("fit_lines:"): P < 0, inlier_thr not finite or <= 0, min_inliers < 2, max_lines outside 1..EMAP_FIT_MAX_LINES,
 * with P > 0 a NULL pointer. */
int emap_fit_lines(const double* pts, const int32_t* offsets, int P, double inlier_thr, int min_inliers, int max_lines, double* segs,
                   int32_t* n_lines, int32_t* labels, void* stream);

/* Batched cubic Bezier least squares (bezier_fit of edge_fitting/bezier_fit.py with the parameters t = linspace(0, 1, n) it fixes): one
 * wave per candidate.
 *
 *   pts   (offsets[Q], 3) doubles, offsets (Q + 1) int32: candidate k is rows offsets[k] .. offsets[k + 1], n >= 4 of them (fewer:
 *         ctrl and rmse are NaN)
 *   ctrl  (Q, 12) doubles out: the 4 control points minimising sum |B(t_k) - p_k|^2 in the Bernstein basis, by the normal equations
 *         (4 x 4, Cholesky); t_k = k (1 / (n - 1)), t_(n-1) = 1
 *   rmse  (Q) doubles out: sqrt(mean_k(sum_c residual^2))
 *
 * EMAP_E_INVALID ("fit_beziers:"): Q < 0, with Q > 0 a NULL pointer. */
int emap_fit_beziers(const double* pts, const int32_t* offsets, int Q, double* ctrl, double* rmse, void* stream);

/* merge_line_segments of the reference (merging/main.py:120-156).  Lines i < j are adjacent when d <= dist_thr && cos >= similarity:
 * d = the smaller clamped distance of the two end points of line j to SEGMENT i (one-sided, as the reference), cos = the signed cosine
 * of the direction vectors end - start, each divided by its norm (a zero norm by 1).  Connected components by label propagation to the
 * fixed point (at most L rounds).
 *
 *   lines    (L, 6) doubles;  raw (raw_off[L], 3) doubles, raw_off (L + 1) int32: the raw points line k was fitted to
 *   labels   (L) int32 out: the smallest index of the line's component
 *   merged   (L, 6) doubles out: row k with labels[k] == k is its component's line - line k itself when it is alone, otherwise the
 *            refit of the members' raw points (members ascending): center + u min(proj), center + u max(proj) with the mean, the
 *            principal direction u (sign: u . (last point - first point) >= 0) and proj = (p - center) . u; any other row is line k
 *   workspace  at least 4 L ceil(L / 32) bytes (the adjacency bits); contents on entry do not matter
 *
 * EMAP_E_INVALID ("fit_merge_lines:"): L outside 0..65536, dist_thr or similarity NaN, with L > 0 a NULL pointer or a workspace too small. */
int emap_fit_merge_lines(const double* lines, int L, const double* raw, const int32_t* raw_off, double dist_thr, double similarity,
                         int32_t* labels, double* merged, void* workspace, size_t workspace_bytes, void* stream);

/* merge_endpoints of the reference (merging/main.py:222-268) on E points (the caller lists the 2 L line end points, then the 2 C curve
 * end points): two are adjacent when dist <= dist_thr; every member of a component of more than one is replaced by the component's mean
 * (sum over the members ascending, divided by their number).
 *
 *   endpoints (E, 3) doubles;  labels (E) int32 out: smallest index of the component;  merged (E, 3) doubles out
 *   workspace at least 4 E ceil(E / 32) bytes
 *
 * EMAP_E_INVALID ("fit_merge_endpoints:"): E outside 0..65536, dist_thr NaN, with E > 0 a NULL pointer or a workspace too small. */
int emap_fit_merge_endpoints(const double* endpoints, int E, double dist_thr, int32_t* labels, double* merged, void* workspace,
                             size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
