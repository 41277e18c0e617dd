/* monosowa_lift.h -- C ABI of the object-cloud stage (libmonosowa_lift.so, monosowa_amd/csrc/object_lift.hip): a metric depth map
 * and instance masks go in, each object's point cloud, centre and range come out, and the views of a track are gathered into the
 * padded clouds that the template search (monosowa_fit.h) takes.  It stands for the reference's decode_img (back-projection),
 * get_car_locations_from_img and standing_concatenate_lidar_clever / moving_lidar_keep_ref.  Python side: monosowa_amd/lift.py.
 *
 * THE RULE.  monosowa_amd.lift.lift_host and tests/lift_reference.py follow it operation for operation.  Each operation is rounded
 * on its own; nothing is contracted to an FMA; double is IEEE binary64.
 *
 * Inputs per frame f: depth [H, W] float32, intrinsics (fx, fy, cx, cy) float64, masks [M, H, W] bytes (non-zero = set),
 * mask_count, pose [3, 4] float64 (rows r0 r1 r2 t: current frame to reference frame).  Scalars: thr (int, >= 1), d, max (double).
 *
 * 1. Points.  Pixel (v, u) with depth z is a point iff z is finite and z > 0.  In double, x = ((u - cx) / fx) * z,
 *    y = ((v - cy) / fy) * z; x, y and z are each rounded once to float32, and all later arithmetic reads those float32 values,
 *    widened.  Point order is row-major pixel order everywhere.
 * 2. Shrink.  A = number of set pixels; s = 2 + isqrt(A) / 10 in integers.  E_r = the pixels for which every in-image pixel within
 *    L1 distance <= r is set (pixels outside the image count as set).  Equivalently, with D(p) the L1 distance from p to the
 *    nearest in-image pixel that is not set: p is in E_r iff D(p) > r.
 * 3. Selection.  S = the points in E_s; if |S| < thr, the points in E_1; if still < thr, the points in the mask; if still < thr:
 *    status FEW.  `shrink` = s, 1 or -1 says which was taken (-1 also for FEW here and for ABSENT).
 * 4. Centre.  m = the per-axis median of S in double ((lo + hi) * 0.5 for an even count).  S' = the points of S with
 *    dx * dx + dz * dz < d * d (double; dx = x - m.x, dz = z - m.z).  If S' is not empty, m = the median of S'.
 *    If use_range and (m.x * m.x + m.y * m.y) + m.z * m.z > max * max: status FAR.
 *    c = R m + t, row by row as ((r0 * m.x + r1 * m.y) + r2 * m.z) + t.  If not c.z > 0 (a NaN included): status BEHIND.
 * 5. Cloud.  The points of the unshrunk mask, their median m2, the same circle test about m2; each survivor transformed like c and
 *    rounded to float32.  total = the number of survivors; total < thr: status FEW.  Otherwise status OK, the first
 *    min(total, Nmax) survivors are written in pixel order, counts = min(total, Nmax), and the CLIPPED bit is set when
 *    total > Nmax.  centres = c; range = sqrt(m.x * m.x + m.z * m.z), the correctly rounded double square root (on the device:
 *    __dsqrt_rn, the round-to-nearest routine of the device library).
 *    truncated = the mask has a set pixel in its first or last 10 rows (rows < 10 or rows >= H - 10).
 * 6. Slots.  A mask at or beyond mask_count[f] (clamped to [0, M]) has status ABSENT.  Every slot's scalars are written:
 *    status, shrink, truncated (0 for ABSENT), and -- zero unless the status is OK (CLIPPED or not) -- counts, total, centres,
 *    range.  Rows of `points` at and beyond counts are not written; no row of a slot that is not OK is written.
 * 7. Gather.  Track b lists views (frame, mask); a view outside [0, F) x [0, M) or whose status is not OK is skipped.  Static
 *    track: the views ordered by key = range + (truncated ? 5.0 : 0.0), ascending, ties to the earlier entry (a stable sort); the
 *    first max_views are kept and their clouds (counts rows each) concatenated in that order.  Moving track: only its first OK view
 *    with frame == ref_frame, or nothing.  n = the sum of the kept counts, K = the output's rows: if n > K, point j is kept iff
 *    ((j + 1) * K) / n > (j * K) / n in 64-bit integers (exactly K points; point j lands in row (j * K) / n).  The track's centre
 *    is the per-axis median, in double, of the kept views' c (NaN if any of them is NaN on that axis); zeros and count 0 for a
 *    track that keeps nothing.  Rows at and beyond the track's count are not written.
 *
 * The device side has no float atomics and no global atomics; integer counters in LDS serve the selection.  A kernel boundary is the
 * only hand-off between workgroups; the bytes written do not depend on where the buffers lie or on launch order.  After the one pass
 * that finds a mask's area and bounding box, all work is confined to that box.  The erosion is a separable L1 distance transform
 * clipped at s + 1: a pass down and up each column, then a pass along each row.  The medians are exact radix selections on
 * order-preserving 32-bit keys of the float32 coordinates.
 *
 * Limits (beyond them MONO_LIFT_TOO_LARGE, and the Python side runs lift_host): H, W <= MONO_LIFT_MAX_SIDE,
 * H * W <= MONO_LIFT_MAX_PIXELS (the clipped distances are bytes: s + 1 <= 255 for every mask the image can hold),
 * M <= MONO_LIFT_MAX_M, F <= MONO_LIFT_MAX_F, Nmax <= MONO_LIFT_MAX_POINTS; gather: B <= MONO_LIFT_MAX_TRACKS,
 * V <= MONO_LIFT_MAX_VIEWS, K <= MONO_LIFT_MAX_POINTS.
 *
 * Device pointers, asynchronous on `stream`, no host synchronisation.
 * Return value: 0, MONO_LIFT_NULL, MONO_LIFT_BAD_SIZE, MONO_LIFT_TOO_LARGE or a hipError_t (> 0).
 */
#ifndef MONOSOWA_LIFT_H
#define MONOSOWA_LIFT_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MONO_LIFT_ABI_VERSION 1
#define MONO_LIFT_NULL (-1)      /* a required pointer is NULL */
#define MONO_LIFT_BAD_SIZE (-2)  /* an extent below its minimum, thr < 1, d or max not a finite number >= 0, stages outside 1..15 */
#define MONO_LIFT_TOO_LARGE (-3) /* beyond the limits below: use the host routine */

#define MONO_LIFT_MAX_SIDE 4096
#define MONO_LIFT_MAX_PIXELS (2530 * 2530 - 1) /* isqrt(A) <= 2529, so s = 2 + isqrt(A) / 10 <= 254 */
#define MONO_LIFT_MAX_M 256
#define MONO_LIFT_MAX_F 4096
#define MONO_LIFT_MAX_POINTS (1 << 20)
#define MONO_LIFT_MAX_TRACKS 65536
#define MONO_LIFT_MAX_VIEWS 256

#define MONO_LIFT_OK 0 /* status of a slot: one of these five, OK possibly with the CLIPPED bit */
#define MONO_LIFT_FEW 1
#define MONO_LIFT_FAR 2
#define MONO_LIFT_BEHIND 3
#define MONO_LIFT_ABSENT 4
#define MONO_LIFT_CLIPPED 8

#define MONO_LIFT_RECORD_INTS 16 /* workspace per slot: A, row0, row1, col0, col1, s, truncated, |E_s|, |E_1|, |mask| points, .. */

/* stages of mono_lift_objects_f32, one launch each; MONO_LIFT_ALL runs the four in order (a later stage reads what the earlier
 * ones left in the workspace) */
#define MONO_LIFT_STAGE_BOX 1     /* area, bounding box, truncated, s */
#define MONO_LIFT_STAGE_COLUMNS 2 /* the distance transform's column pass */
#define MONO_LIFT_STAGE_ROWS 4    /* its row pass, the three point sets and their sizes */
#define MONO_LIFT_STAGE_CLOUD 8   /* medians, tests, transform, compaction */
#define MONO_LIFT_ALL 15

int mono_lift_abi_version(void);

/* depth [F, H, W] float32, intrinsics [F, 4] float64, masks [F, M, H, W] uint8, mask_count [F] int32, poses [F, 3, 4] float64
 * (NULL: the identity).  Workspace: dist and sets, [F, M, H, W] bytes each, record [F, M, MONO_LIFT_RECORD_INTS] int32.
 * -> points [F, M, Nmax, 3] float32, counts / total / status / shrink [F, M] int32, centres [F, M, 3] float64, range [F, M] float64,
 * truncated [F, M] uint8. */
int mono_lift_objects_f32(const float *depth, const double *intrinsics, const uint8_t *masks, const int32_t *mask_count,
                          const double *poses, int F, int M, int H, int W, int Nmax, int thr, double d, int use_range, double max,
                          int stages, uint8_t *dist, uint8_t *sets, int32_t *record, float *points, int32_t *counts, int32_t *total,
                          double *centres, double *range, uint8_t *truncated, int32_t *status, int32_t *shrink, void *stream);

/* Rule 7.  points / counts / status / range / truncated / centres as mono_lift_objects_f32 wrote them; tracks [B, V, 2] int32
 * (frame, mask; a negative frame ends nothing, it is only skipped), moving [B] uint8 (NULL: none).
 * -> out_points [B, K, 3] float32, out_counts [B] int32, out_centres [B, 3] float64. */
int mono_lift_gather_f32(const float *points, const int32_t *counts, const int32_t *status, const double *range,
                         const uint8_t *truncated, const double *centres, int F, int M, int Nmax, const int32_t *tracks,
                         const uint8_t *moving, int B, int V, int ref_frame, int max_views, int K, float *out_points,
                         int32_t *out_counts, double *out_centres, void *stream);

#ifdef __cplusplus
}
#endif
#endif
