/* sid_fg.h - C ABI of the first-guess evaluation on MI355X (gfx950): SURVEY.md section 8, row f4.
 *
 * Replaces, in the reference's prelude of pattern matching (sea_ice_drift v0.7.1):
 *
 *   sid_fg_interp_linear   the evaluation half of lib.interpolation_near (lib.py:179-201):
 *                              griddata(src, x2, dst, method='linear'), griddata(src, y2, dst, method='linear')
 *                          i.e. point location in the Delaunay triangulation of the key points + barycentric
 *                          interpolation of both components at the N grid points, NaN outside the convex hull.
 *                          The triangulation itself stays SciPy's (Qhull) on the host - the simplices are an input -
 *                          so the triangles, and with them the interpolant, are the reference's.
 *   sid_fg_nearest_dist    pmlib.get_distance_to_nearest_keypoint (pmlib.py:61-77) sampled at the grid points
 *                          (pmlib.py:300-305): distance from each (row, col) to the nearest key-point pixel - the
 *                          exact Euclidean distance the full-image EDT holds there (sqrt of an exact integer).
 *
 * Arithmetic of the interpolation: per simplex the 2x2 system of the barycentric transform is solved by LU with
 * partial pivoting, c = Tinv (x - r), c2 = 1 - c0 - c1, value = c0 v0 + c1 v1 + c2 v2 accumulated in vertex order
 * (scipy.spatial.Delaunay.transform / LinearNDInterpolator); a point belongs to the first simplex (lowest index)
 * with all c >= -eps, eps = 100 * DBL_EPSILON.  SciPy reaches a simplex by a directed walk, so for a query ON an edge,
 * a vertex or the hull it may pick another simplex (or none); and its BLAS may round the 2x2 solve differently in the
 * last bit.  Neither may change what the reference computes next (np.round of the first guess, pmlib.py:285-288), so
 * every query for which that cannot be excluded is FLAGGED in doubt[] and the caller evaluates those with SciPy itself
 * (sea_ice_drift_amd/lib.py interpolation_near).  A query whose smallest barycentric coordinate in some simplex lies
 * within 1e-9 of zero (on an edge, a vertex, the hull) is looked at against every simplex: it stays flagged unless hull
 * membership is clear (no smallest coordinate within 4e-15 of SciPy's threshold -2.2e-14), all containing simplices round to the same
 * integers and no value lies within 1e-6 of a half-integer; every other query lies strictly inside exactly one simplex
 * (flagged only when its value is that close to a half-integer).
 * Limitation: degenerate (flat) simplices are skipped here, whereas SciPy gives them a NaN transform and then accepts
 * queries in their neighbours with a wider tolerance (sqrt(eps)) towards them - a case the flags do not model.  The
 * caller must not use this entry point for a triangulation that holds such a simplex: sea_ice_drift_amd/lib.py checks
 * (condition number of every simplex) and evaluates with SciPy alone then.
 * Host buffers in / host buffers out; 0 on success, a negative SID_PM_ERR_* code otherwise (sid_pm.h).
 */
#ifndef SID_FG_H
#define SID_FG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* pts [n_pts][2], simplices [n_simp][3] (indices into pts), values [n_pts][2], q [n_q][2] -> out [n_q][2];
 * optional (may be NULL): simplex [n_q] = index of the simplex a query was located in (-1: none), doubt [n_q] (above) */
int sid_fg_interp_linear(int device, const double *pts, int64_t n_pts, const int32_t *simplices, int64_t n_simp,
                         const double *values, const double *q, int64_t n_q, double *out, int32_t *simplex, int32_t *doubt);

/* seeds [n_seeds][2], q [n_q][2] -> dist [n_q] = min over seeds of the Euclidean distance */
int sid_fg_nearest_dist(int device, const double *seeds, int64_t n_seeds, const double *q, int64_t n_q, double *dist);

/* get_distance_to_nearest_keypoint (pmlib.py:61-77) at full resolution: dist [rows][cols] = distance of every pixel (row, column)
 * to the nearest of seeds [n_seeds][2] = (row, column) - the reference's distance_transform_edt image, evaluated per pixel through
 * the same buckets (sqrt of the exact integer squared distance in float64: the same numbers). */
int sid_fg_distance_image(int device, const double *seeds, int64_t n_seeds, int64_t rows, int64_t cols, double *dist);

/* A first guess that needs no triangulation (NOT the reference's method): out [n_q][2] = the
 * component-wise median of values [n_seeds][2] over the k nearest seeds [n_seeds][2] of every query q [n_q][2].  Every
 * operation below is one IEEE double rounding in the order written (tests/fg_knn_spec.py restates it in NumPy).
 *   usable seed     both coordinates and both values finite; no other seed takes part.
 *   distance        dx = q0 - s0; dy = q1 - s1; d2 = dx*dx + dy*dy.
 *   admissible      d2 <= m2, m2 = max_dist * max_dist (max_dist = +inf: no limit).
 *   neighbours      the first m = min(k, number of admissible usable seeds) seeds in ascending (d2, seed index) order -
 *                   lexicographic, so ties and duplicated seeds resolve by index.
 *   result          per component the median of the neighbours' values: m odd - the middle value of the sorted values s;
 *                   m even - (s[m/2-1] + s[m/2]) / 2.0.  m = 0, or a query that is not finite: NaN, NaN.
 *   count  [n_q]    (may be NULL) m.       index [n_q][k]   (may be NULL) the neighbours in that order, padded with -1.
 * n_q = 0 returns at once; n_seeds = 0 is valid (every result empty).  SID_PM_ERR_ARG: seeds NULL with n_seeds > 0, values, q
 * or out NULL, a negative size, k outside 1..16, max_dist NaN or <= 0; SID_PM_ERR_UNSUPPORTED: n_seeds >= 2^31; all before any
 * device call.  device = -1 runs the host instance: the same source (csrc/fg_knn.h) in a loop over every (query, seed) pair.
 * On a device the queries walk the buckets of sid_fg_nearest_dist (fewer than 256 usable seeds, a bounding box without area
 * or SID_FG_NO_GRID=1: every pair); the result is the host instance's bit for bit either way. */
int sid_fg_knn(int device, const double *seeds, int64_t n_seeds, const double *values, const double *q, int64_t n_q,
               int k, double max_dist, double *out, int32_t *count, int32_t *index);

/* Queries that are not finite (a NaN or an infinite coordinate; a projection does not keep grid points finite outside its
 * footprint).  sid_fg_interp_linear: such a query is in no simplex and near none - out = NaN, simplex = -1, doubt = 0 - on the
 * bucket route and on the brute-force route alike.  sid_fg_nearest_dist: its distance is +inf on both routes (every comparison
 * with a distance that is not a number is false, and no finite seed is nearer than +inf).  No cell arithmetic is undefined
 * for them: a coordinate that is not a number falls into cell 0 of the buckets, an infinite one into a border cell. */

/* Test support (host values only, no device call; the ABI version does not count it): the route of the calling thread's last
 * sid_fg_interp_linear, sid_fg_nearest_dist, sid_fg_distance_image or sid_fg_knn (on a device) that succeeded.
 *   buckets    1: the queries walked the buckets; 0: every simplex / every seed
 *   entries    interpolation: the bucket entries counted (more than `capacity`: they did not fit, brute force; 0 where the
 *              buckets were not tried: SID_FG_NO_GRID, a box without area); seeds: the seeds binned (0: none)
 *   capacity   the room of the bucket lists: 8 n_simp + 128 * 128, or the number of (usable) seeds
 *   ychunks, chunk   brute-force point location: the simplex chunks of the launch and the simplices per chunk (else 0)
 * SID_PM_ERR_ARG: out NULL; SID_PM_ERR_STATE: no such call yet on this thread. */
typedef struct sid_fg_route {
    int64_t buckets, entries, capacity, ychunks, chunk;
} sid_fg_route;
int sid_fg_debug_route(struct sid_fg_route *out);

const char *sid_fg_last_error(void);
/* Free the grow-only device scratch block of the two entry points on `device` (every device: -1).  The blocks are kept between calls so that no call pays for
 * hipMalloc / hipFree; a long-lived process that is done with the GPU hands the memory back with this (the Python mirror's
 * pmlib.release_contexts() calls it).  Not to be called while a call on that device is in flight. */
int sid_fg_release(int device);

#ifdef __cplusplus
}
#endif
#endif
