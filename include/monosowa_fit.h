/* monosowa_fit.h -- C ABI of the template-pose search (libmonosowa_fit.so, monosowa_amd/csrc/template_fit.hip): a car template
 * fitted to each object's aggregated point cloud by exhaustive search over a grid of placements, the step that writes the first
 * 3D pseudo-label (the reference's optimize_coarse -> optimize_fine, optimize_moving and optimize_loc_only with the losses
 * binary2way / binary1way, KITTI frame).  Python side: monosowa_amd/template_fit.py.
 *
 * THE RULE.  monosowa_amd.template_fit.fit_host and tests/fit_reference.py follow it operation for operation.
 *
 * Frame: KITTI camera, x right, y down, z forward.  Template tmpl [T, 3] float32, centred at the origin, width along x, height
 * along y, length along z.  Object o: scan points scan_o [N_o, 3] float32, a centre c_o (float64) and three float64 lists
 * dx [I], dz [J], theta [K].
 *
 * The host forms, in float64, tx_i = dx_i + c.x, ty = c.y, tz_j = dz_j + c.z, cos(theta_k), sin(theta_k) and rounds each to
 * float32.  The kernels see only those float32 numbers.  Below, every float32 operation is rounded on its own; nothing is
 * contracted to an FMA.
 *
 * Placement h = (i * J + j) * K + k is the template rotated about y by theta_k and moved to (tx_i, ty, tz_j); with
 * c = cos(theta_k), s = sin(theta_k), template point (x, y, z) lands at
 *     wx = (c * x + s * z) + tx        wy = y + ty        wz = (c * z - s * x) + tz
 *
 * a(h) = the number of template points for which SOME scan point p has  ((p.x - wx)^2 + (p.y - wy)^2) + (p.z - wz)^2 < r2.
 * b(h) = the number of scan points p for which SOME template point has  ((lx - x)^2 + (ly - y)^2) + (lz - z)^2 < r2, the scan
 *        point taken into the template's frame:  px = p.x - tx, py = p.y - ty, pz = p.z - tz,
 *        lx = c * px - s * pz,  ly = py,  lz = s * px + c * pz.
 * r2 = float32(r) * float32(r) in float32, r = loss_functions.binary_loss_threshold.
 * A NaN or infinite coordinate passes no comparison: such a point is nobody's neighbour, and still counts in T or N.
 *
 * Loss: the double L(h) = -((double)a / T + (double)b / N) (binary2way) or -(double)a / T (binary1way; b is still reported).
 * The best placement has the smallest L; ties go to the smallest h (the reference's strict `<` in its nested loop order).
 *
 * Fine stage (two-stage static objects): a second search with I = J = 1 at the coarse winner's (tx, tz) over the caller's
 * K = 360 angles; its winner (first minimum again) replaces theta.  It reads the coarse winner from the device record: `fix`.
 *
 * Empty: an object with N = 0, or T = 0, gets status MONO_FIT_EMPTY, h = 0, a = b = 0, L = 0.
 *
 * The search is exact: the two uniform grids (over the template, built by the host once per template; over each object's scan,
 * built by mono_fit_grid_f32) only cull pairs that cannot pass.  Their cells are at least 1.01 r wide, float32 slack included, a
 * query looks at the 27 cells around its own, clipped to the grid, and a query more than one cell outside the grid's bounds has
 * no neighbour.  No atomics anywhere; a kernel boundary is the only hand-off between workgroups; the bytes written do not
 * depend on where the buffers lie.
 *
 * Limits (beyond them MONO_FIT_TOO_LARGE, and the Python side runs fit_host): T <= MONO_FIT_MAX_T, N <= MONO_FIT_MAX_N per
 * object, H = I * J * K <= MONO_FIT_MAX_H, B <= MONO_FIT_MAX_B, the template's grid <= MONO_FIT_MAX_TCELLS cells.
 *
 * Device pointers unless said otherwise, asynchronous on `stream`, no host synchronisation.
 * Return value: 0, MONO_FIT_NULL, MONO_FIT_BAD_SIZE, MONO_FIT_TOO_LARGE or a hipError_t (> 0).
 */
#ifndef MONOSOWA_FIT_H
#define MONOSOWA_FIT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MONO_FIT_ABI_VERSION 1
#define MONO_FIT_NULL (-1)       /* a required pointer is NULL */
#define MONO_FIT_BAD_SIZE (-2)   /* an extent below its minimum, r without a positive finite float32 square, a malformed grid
                                    record, `sorted` not 16-byte aligned */
#define MONO_FIT_TOO_LARGE (-3)  /* beyond the limits below: use the host routine */

#define MONO_FIT_MAX_T 2048
#define MONO_FIT_MAX_N 65536
#define MONO_FIT_MAX_H (1 << 20)
#define MONO_FIT_MAX_B 4096
#define MONO_FIT_MAX_DIM 32                /* cells per axis of either grid */
#define MONO_FIT_MAX_TCELLS 4096           /* the template's grid lives in LDS */
#define MONO_FIT_MAX_CELLS (32 * 32 * 32)  /* a scan's grid */

#define MONO_FIT_OK 0     /* status of an object */
#define MONO_FIT_EMPTY 1  /* N = 0 or T = 0 */

#define MONO_FIT_RESULT_INTS 6 /* per object: h, a, b, status, i, j */

/* A uniform grid: cell (cx, cy, cz) has id (cz * dim[1] + cy) * dim[0] + cx; along axis a, a point at v lies in cell
 * floor((v - origin[a]) * inv[a]), clamped into the grid; inv[a] < 0: one cell on that axis and no culling (extent not finite).
 * Points with a coordinate that is not finite have the id `ncell` and are never visited. */
typedef struct mono_fit_grid {
  float origin[3];
  float inv[3];
  int32_t dim[3];
  int32_t ncell;
} mono_fit_grid_t;

int mono_fit_abi_version(void);

/* Each object's scan index.  scan [B, Nmax, 3] float32 (object o uses its first count[o] points, clamped to [0, Nmax]), r the
 * threshold -> grid [B] mono_fit_grid_t, sorted [B, Nmax, 4] float32 (16-byte aligned; the points ordered by cell id, then by
 * index; .w = 0),
 * start [B, MONO_FIT_MAX_CELLS + 1] int32 (start[c] = number of points with id < c, written for c <= ncell).
 * Workspace: cell [B, Nmax] int32, scell [B, Nmax] int32.  Rows at and beyond count[o] are not written. */
int mono_fit_grid_f32(const float *scan, const int32_t *count, int B, int Nmax, float r, mono_fit_grid_t *grid, float *sorted,
                      int32_t *start, int32_t *cell, int32_t *scell, void *stream);

/* Evaluates placements.  tmpl [T, 3] float32 ORDERED BY CELL of `tgrid` (a HOST pointer), tstart [tgrid->ncell + 1] int32;
 * grid / sorted / start as mono_fit_grid_f32 wrote them; tx [B, I], ty [B], tz [B, J], cs [B, K, 2] (cos, sin) float32.
 * fix == NULL: H = I * J * K placements per object.  fix != NULL, int32 [B, MONO_FIT_RESULT_INTS] as mono_fit_reduce_f64 wrote
 * it: H = K placements at (tx[fix[o][4]], tz[fix[o][5]]) (indices clamped into the lists).
 * -> ab [B, H, 2] int32: a(h), b(h). */
int mono_fit_search_f32(const float *tmpl, const int32_t *tstart, const mono_fit_grid_t *tgrid, int T, const mono_fit_grid_t *grid,
                        const float *sorted, const int32_t *start, const int32_t *count, int B, int Nmax, const float *tx,
                        const float *ty, const float *tz, const float *cs, int I, int J, int K, const int32_t *fix, float r,
                        int32_t *ab, void *stream);

/* The fixed-order minimum.  ab [B, H, 2], count [B]; H = I * J * K (fix == NULL) or K (fix != NULL: i, j are copied from it);
 * one_way: binary1way -> result [B, MONO_FIT_RESULT_INTS] int32 (h, a, b, status, i, j), loss [B] float64. */
int mono_fit_reduce_f64(const int32_t *ab, const int32_t *count, int B, int Nmax, int T, int I, int J, int K, const int32_t *fix,
                        int one_way, int32_t *result, double *loss, void *stream);

#ifdef __cplusplus
}
#endif
#endif
