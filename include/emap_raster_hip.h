/* emap_raster_hip.h - the edge rasteriser of libemap_hip.so: 3D line segments and cubic Beziers drawn into the edge maps of a camera
 * list.  A fourth header with its own version, bound by its own table (emap_amd/_lib.py: RASTER_SYMBOLS, raster_lib(), raster_api()).
 * emap_hip.h, emap_eval_hip.h and emap_fit_hip.h, their symbol sets and their versions are unchanged by anything declared here.
 *
 * Conventions are emap_hip.h's: C linkage, return value 0 = ok or a negative EMAP_E_* with the text in emap_last_error() (one
 * thread-local text for all headers), device pointers unless a parameter is named *_host, `stream` is a hipStream_t (NULL: the
 * default stream), every call is asynchronous on it, no entry point allocates.
 *
 * All arithmetic is fp64 with no FMA contraction, every sum is taken left to right as written below, division and square root are the
 * IEEE ones, and no result is formed by an atomic.  Every output is a pure function of the inputs, bit-identical from run to run and
 * independent of what the output buffers and the workspace held before.  The numpy restatement, in the same scalar order, is
 * tests/edge_raster_ref.py.
 */
#ifndef EMAP_RASTER_HIP_H
#define EMAP_RASTER_HIP_H

#include <stddef.h>
#include <stdint.h>
#include "emap_hip.h" /* EMAP_OK, EMAP_E_INVALID, EMAP_E_LAUNCH; emap_last_error() */

#ifdef __cplusplus
extern "C" {
#endif

#define EMAP_RASTER_ABI_VERSION 1
int emap_raster_abi_version(void);

#define EMAP_RASTER_MAX_CURVE_SEGMENTS 256   /* curve_segments */
#define EMAP_RASTER_MAX_SEGMENTS 1048576     /* n_lines + n_curves * curve_segments of one call */
#define EMAP_RASTER_MAX_HALF_WIDTH 64.0      /* half_width, in pixels */
#define EMAP_RASTER_MAX_FRAMES 65535         /* F */
#define EMAP_RASTER_MAX_DIM 65536            /* h and w */
#define EMAP_RASTER_MAX_COORD 1099511627776.0 /* 2^40: a segment with a projected coordinate of this magnitude or more is not drawn */
#define EMAP_RASTER_ROW_BYTES 64             /* workspace bytes per (frame, segment) */

/* Bytes of the workspace of emap_raster_edges:  F * (n_lines + n_curves * curve_segments) * EMAP_RASTER_ROW_BYTES  - one row per
 * frame and segment; 0 when there is no segment.  EMAP_E_INVALID ("raster_workspace_bytes:" leads the text): a negative count,
 * curve_segments outside [1, EMAP_RASTER_MAX_CURVE_SEGMENTS], more than EMAP_RASTER_MAX_SEGMENTS segments, F outside
 * [1, EMAP_RASTER_MAX_FRAMES], a NULL bytes_host. */
int emap_raster_workspace_bytes(int n_lines, int n_curves, int curve_segments, int F, size_t* bytes_host);

/* Draw n_lines segments and n_curves cubic Beziers into F views of h x w pixels.
 *
 *   lines      (n_lines, 2, 3) doubles: the end points;  curves (n_curves, 4, 3) doubles: the control points P0..P3
 *   weights    (n_lines + n_curves) doubles in [0, 1], or NULL: every weight 1.  EDGE e < n_lines is line e, edge n_lines + j curve j
 *   intr       (F, 4) doubles: fx, fy, cx, cy of every frame (intrinsics without skew whose last row is 0 0 1)
 *   R, T       (F, 3, 3), (F, 3) doubles: the WORLD-TO-CAMERA rotation and translation of every frame
 *   bytes      (F, h, w) uint8 out;  ids (F, h, w) int32 out, or NULL
 *   workspace  workspace_bytes >= what emap_raster_workspace_bytes reports, 16-byte aligned; may be NULL when that is 0
 *
 * Segments.  A line is one segment.  Curve j is curve_segments = n segments, segment k from B(t_k) to B(t_k+1), t_k = (double)k / (double)n,
 * and with u = 1 - t
 *     b0 = (u u) u,  b1 = (3 (u u)) t,  b2 = (3 u) (t t),  b3 = (t t) t,     B(t) = (b0 P0 + b1 P1) + (b2 P2 + b3 P3)   per coordinate,
 * so that B(0) = P0 and B(1) = P3 exactly.  Segments are numbered lines first, then curve by curve, k ascending.
 *
 * Camera.  An end point X = (x, y, z) has camera coordinates  c_i = ((R_i0 x + R_i1 y) + R_i2 z) + T_i.  With end points a, b in camera
 * coordinates: the segment is dropped when a_2 < z_near and b_2 < z_near; when exactly one of the two holds, with
 * t = (z_near - a_2) / (b_2 - a_2) that end becomes  a_i + t (b_i - a_i), i = 0, 1, 2  (the other end stays).  Then each end projects to
 *     px = (fx c_0) / c_2 + cx,   py = (fy c_1) / c_2 + cy,
 * and the segment is dropped unless all four of |x0|, |y0|, |x1|, |y1| are < EMAP_RASTER_MAX_COORD (a NaN fails).
 *
 * Box.  A segment that is not dropped has the pixel box  [max(0, floor(min(x0, x1) - half_width) - 1), min(w - 1, ceil(max(x0, x1) +
 * half_width) + 1)]  in x and the same with y and h; it may be empty.  Below the coordinate bound every pixel outside the box has
 * v = 0: restricting a segment to its box changes no output.
 *
 * Pixel.  For the pixel (x, y) - integers as doubles - inside the box of the segment (x0, y0) - (x1, y1) of edge e, ux = x1 - x0, uy = y1 - y0:
 *     t  = min(max(((x - x0) ux + (y - y0) uy) / ((ux ux + uy uy) + 1e-9), 0), 1)
 *     ex = x - (x0 + t ux),  ey = y - (y0 + t uy),  d = sqrt(ex ex + ey ey)
 *     v  = min(max(half_width - d, 0), 1) * weight[e]
 * The pixel's value is the maximum of v over all segments, 0 without one; its byte is rint(255 v), half to even.  ids, when given, holds
 * the lowest edge index among the segments that attain the maximum, and -1 where the maximum is 0.
 *
 * Two launches: one builds the (frame, segment) table in the workspace - projected end points, box, weight, edge -, one with a workgroup
 * per frame and tile of pixels gathers from it and stores every byte (and id) exactly once.
 *
 * EMAP_E_INVALID before any launch ("raster_edges:" leads the text): what emap_raster_workspace_bytes rejects; h or w outside
 * [1, EMAP_RASTER_MAX_DIM]; half_width not in (0, EMAP_RASTER_MAX_HALF_WIDTH]; a z_near that is not finite and > 0; a NULL intr / R / T /
 * bytes; a NULL lines with n_lines > 0 or curves with n_curves > 0; a workspace that is NULL, misaligned or too small when rows are
 * needed. */
int emap_raster_edges(const double* lines, int n_lines, const double* curves, int n_curves, int curve_segments, const double* weights,
                      const double* intr, const double* R, const double* T, int F, int h, int w, double half_width, double z_near,
                      uint8_t* bytes, int32_t* ids, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
