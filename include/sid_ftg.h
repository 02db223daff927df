/* sid_ftg.h - C ABI of the guided feature matcher on MI355X (gfx950): Hamming k=2 within a search radius.
 *
 * sid_ft_knn2 (sid_ft.h) is the reference's brute-force matcher: every descriptor of image 1 against every descriptor of
 * image 2.  This unit searches the two nearest neighbours of a query only among the train descriptors that lie within
 * `radius` pixels of the position the georeference predicts for it.  The reference has no such call.
 *
 *   desc1 [n1][32] uint8 with qx, qy [n1] float64: the query descriptors and their PREDICTED positions in the pixel frame
 *                                                  of the train image
 *   desc2 [n2][32] uint8 with tx, ty [n2] float64: the train descriptors and their positions
 *   radius                                         finite, >= 0
 *
 * Train descriptor j is a candidate of query i iff  dx * dx + dy * dy <= radius * radius  with dx = tx[j] - qx[i],
 * dy = ty[j] - qy[i], every operation ONE IEEE float64 rounding (no fused multiply-add).  A query whose position is not
 * finite has no candidates; a train point whose position is not finite is nobody's candidate.
 *
 *   idx [n1][2], dist [n1][2] int32   the two candidates of smallest Hamming distance, nearest first; equal distances by the
 *                                     smaller train index; entries that do not exist are -1
 *   count [n1] int32                  the number of candidates (may be NULL)
 *
 * A radius that covers every pair gives the idx and dist of sid_ft_knn2 bit for bit.
 *
 * 0 on success, a negative SID_PM_ERR_* code otherwise (sid_pm.h); sid_ftg_last_error() returns the message of the calling
 * thread's last failure.  SID_PM_ERR_ARG, before any device call: a negative size, n1 > (2^31 - 1) / 4, n2 >= 2^22 (the index
 * bits of the ordering key), a radius that is negative or not finite, a null pointer where n1 > 0.  n1 == 0 returns 0.
 */
#ifndef SID_FTG_H
#define SID_FTG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SID_FTG_DESC_BYTES 32
#define SID_FTG_MARGIN_LOG2 20        /* cell side >= radius * (1 + 2^-20) */
#define SID_FTG_MAX_AXIS 1024         /* cells per axis at the most */

/* Host buffers in, host buffers out (upload, match, download on the given device). */
int sid_ftg_knn2(int device, const uint8_t *desc1, const double *qx, const double *qy, int64_t n1,
                 const uint8_t *desc2, const double *tx, const double *ty, int64_t n2, double radius,
                 int32_t *idx, int32_t *dist, int32_t *count);

/* Same on device-resident buffers (descriptors and workspace 16-byte aligned), asynchronous on `hip_stream` (a hipStream_t,
 * may be NULL): no host synchronisation and no read-back.  `d_workspace` must hold sid_ftg_workspace_bytes(n1, n2) bytes
 * (0 for sizes the entry does not accept). */
int sid_ftg_knn2_device(const uint8_t *d_desc1, const double *d_qx, const double *d_qy, int64_t n1,
                        const uint8_t *d_desc2, const double *d_tx, const double *d_ty, int64_t n2, double radius,
                        int32_t *d_idx, int32_t *d_dist, int32_t *d_count, void *d_workspace, void *hip_stream);
int64_t sid_ftg_workspace_bytes(int64_t n1, int64_t n2);

/* Test support (host arithmetic only, no device call): what csrc/ft_guided_plan.h computes for n1 queries, n2 train points
 * whose finite positions have the bounding box [x_lo, x_hi] x [y_lo, y_hi] (lo > hi: no finite train position), and `radius`.
 *   nx, ny          cells along x and y; the cell of p is floor((p - x0) / cell_x), clamped to 0 .. nx - 1
 *   axis_cap        the most cells an axis may have for this n2: ceil(sqrt(n2)) in 1 .. SID_FTG_MAX_AXIS
 *   max_items       the bound of the work list = workgroups of the match kernel
 *   workspace_bytes as sid_ftg_workspace_bytes                                                                        */
typedef struct sid_ftg_plan {
    double x0, y0, cell_x, cell_y;
    int64_t nx, ny, axis_cap, max_items, workspace_bytes;
} sid_ftg_plan;
int sid_ftg_debug_plan(int64_t n1, int64_t n2, double x_lo, double x_hi, double y_lo, double y_hi, double radius,
                       struct sid_ftg_plan *out);

const char *sid_ftg_last_error(void);
/* Free the grow-only device block of sid_ftg_knn2 on `device` (every device: -1).  Not while a call on it is in flight. */
int sid_ftg_release(int device);

#ifdef __cplusplus
}
#endif
#endif
