/* monosowa_track.h -- C ABI of the object-track stage (libmonosowa_track.so, monosowa_amd/csrc/object_track.hip): the centres and
 * statuses that the object-cloud stage (monosowa_lift.h) wrote go in; tracks, the moving / standing decision, the heading of a moving
 * track and the keep flag come out, in the form mono_lift_gather_f32 and the template search (monosowa_fit.h) take.  It stands for the
 * reference's perform_3D_tracking_kitti ("3D simple tracking", frames_creation.tracker_for_merging: 3D), decide_if_standing_or_moving_both5,
 * filter_moving_and_not_visible, choose_proper_mask, the pseudo-lidar branch of filter_hidden_standing_cars_tracked and
 * estimate_angle_from_movement_tracked.  Python side: monosowa_amd/track.py.
 *
 * THE RULE.  monosowa_amd.track.track_host follows it operation for operation; tests/track_reference.py restates it in the reference's
 * own shape.  All arithmetic is IEEE binary64; each operation is rounded on its own; nothing is contracted to an FMA.
 *
 * Inputs: S windows, each centres [F, M, 3] float64 and status [F, M] int32 as mono_lift_objects_f32 wrote them.  Scalars: ref_frame
 * (any int; outside [0, F) no track is visible), d_track, d_move, d_angle, z0 (finite, >= 0; the reference hard-codes z0 =
 * MONO_TRACK_Z0), use_pseudo_lidar, Tmax.
 *
 * 1. Detections.  The detections of frame f are its slots m in ascending order with (status & 7) == MONO_LIFT_OK and three finite
 *    centre coordinates.  A non-finite centre is not a detection (a deviation: numpy's argmin would pick the NaN).
 * 2. Tracks.  Every detection of frame 0 opens a track, in slot order.  Frames 1 .. F-1 are visited in order; a frame without a
 *    detection is skipped whole (no prediction advances).  A track with n views L[0 .. n-1] in append order predicts L[n-1] when
 *    n == 1; otherwise, with k = min(n - 1, 4) and e_j = L[n-j] - L[n-j-1], it predicts p = ((((e_1 + e_2) + e_3) + e_4) / k) + L[n-1]
 *    per axis, only the first k terms summed, the divisor k as a double.  Frame gaps are ignored, as the reference ignores them.
 *    q(z, t) = ((dx * dx + dy * dy) + dz * dz) with d = detection z - prediction t.  a(z) = the t that minimises q(z, t),
 *    b(t) = the z that minimises it: the scan starts at index 0 and moves on only when q < the best so far, so ties go to the lowest
 *    index.  Detection z is appended to track a(z) iff b(a(z)) == z and q(z, a(z)) < d_track * d_track; otherwise it opens a new track.
 *    New tracks follow the existing ones in detection order; all predictions of a frame are formed before any append.  Tracks never
 *    end (the reference's termination branch is dead code, `and False`).  Squares are compared where the reference compares the
 *    square roots of cdist and norm (a deviation).  A detection that would open track number Tmax or beyond is dropped and counted
 *    in dropped[s].
 * 3. Per track.  length = its views.  visible = it has a view at ref_frame; ref_mask = that view's slot, else -1.
 *    Moving.  N = length - 1 differences D_k = L[k+1] - L[k].  N <= 1: not moving.  Otherwise per axis mean = (the sum of D_k in k
 *    order, from 0.0) / N and var = (the sum of (D_k - mean) * (D_k - mean) in k order) / N; mm = (mean.x * mean.x + mean.y * mean.y) +
 *    mean.z * mean.z; vv = (var.x + var.y) + var.z; net2 = the same three-term square sum of L[length-1] - L[0].  Moving iff
 *    mm > ((z0 * z0) * 0.5) * vv and net2 > d_move * d_move.  This is the reference's norm(mean) / (norm(std) / sqrt 2) > z0 without the
 *    division: zero variance with a non-zero mean is moving, all-zero differences are not (the reference's 0 / 0 fails its comparison
 *    too), a NaN fails.
 *    Heading.  theta is NaN unless the track is moving, visible and length >= 3.  With r = the position of the reference view in the
 *    track, walk i = r-1, r-2, .. until 5 are accepted or the track ends: i is accepted when dx * dx + dz * dz > d_angle * d_angle with
 *    dx = L[r].x - L[i].x, dz = L[r].z - L[i].z, and its angle is atan2(dz, dx).  Then walk i = r+1, .. the same way with
 *    dx = L[i].x - L[r].x.  The angles are listed backward walk first, each in walk order.  Fewer than 3: NaN.  An even count repeats
 *    the last angle.  theta = (-median) + MONO_TRACK_HALF_PI, the median being the middle element of the sorted (odd) list.  The
 *    reference's `> pi` branch cannot fire on a result of atan2, which lies in [-pi, pi]; it is left out.  atan2 is the platform's
 *    (the device library's on the device, libm's on the host): the one operation that is not bit-reproducible between the two.
 *    keep = visible || (!use_pseudo_lidar && !moving), for a track with a view: filter_moving_and_not_visible followed by the
 *    pseudo-lidar branch of filter_hidden_standing_cars_tracked.  The real-LiDAR proximity test of that function's other branch is
 *    not built: without use_pseudo_lidar every standing track is kept.
 * 4. Outputs.  Every element of every output is written for every track below Tmax.  tracks [S, Tmax, F, 2] int32: position f holds
 *    (f, m) when the track has a view in frame f, else (-1, -1) -- the table mono_lift_gather_f32 takes with V = F (it skips negative
 *    frames; ascending frame order is its tie order).  length, ref_mask [S, Tmax] int32; moving, visible, keep [S, Tmax] uint8;
 *    theta [S, Tmax] float64; count (the number of tracks), dropped [S] int32.  Rows at and beyond count: tracks and ref_mask -1,
 *    length and the three flags 0, theta NaN.
 *
 * The device side: one workgroup per window walks the frames in order (association); one lane per track then reads that track's row
 * of the table (summary).  No global atomics, no float atomics; the bytes written do not depend on where the buffers lie.
 *
 * Limits (beyond them MONO_TRACK_TOO_LARGE, and the Python side runs track_host): F <= MONO_LIFT_MAX_VIEWS (the table's V),
 * M <= MONO_LIFT_MAX_M (one lane per slot of a frame), S <= MONO_TRACK_MAX_WINDOWS, Tmax <= MONO_TRACK_MAX_TRACKS.  The last is the
 * LDS budget of the association workgroup: per track its last five centres (120 bytes), its prediction (24), length, b(t) and the
 * frame's view (12), 156 bytes in all; per slot of a frame 40 bytes; 896 * 156 + 256 * 40 + 32 = 150,048 of the 163,840 bytes a
 * workgroup may hold on gfx950.
 *
 * Device pointers, asynchronous on `stream`, no host synchronisation.
 * Return value: 0, MONO_TRACK_NULL, MONO_TRACK_BAD_SIZE, MONO_TRACK_TOO_LARGE or a hipError_t (> 0).
 */
#ifndef MONOSOWA_TRACK_H
#define MONOSOWA_TRACK_H
#include <stdint.h>

#include "monosowa_lift.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MONO_TRACK_ABI_VERSION 1
#define MONO_TRACK_NULL (-1)      /* a required pointer is NULL */
#define MONO_TRACK_BAD_SIZE (-2)  /* S, F, M or Tmax below 1, a scalar that is not a finite number >= 0, stages outside 1..3 */
#define MONO_TRACK_TOO_LARGE (-3) /* beyond the limits below: use the host routine */

#define MONO_TRACK_MAX_TRACKS 896
#define MONO_TRACK_MAX_WINDOWS 65536

#define MONO_TRACK_Z0 0.2                     /* the z-score the reference hard-codes */
#define MONO_TRACK_HALF_PI 1.5707963267948966 /* the double M_PI / 2 */

/* stages of mono_track_objects_f64, one launch each; MONO_TRACK_ALL runs both in order (the summary reads the table that the
 * association wrote) */
#define MONO_TRACK_STAGE_ASSOCIATE 1 /* tracks, count, dropped */
#define MONO_TRACK_STAGE_SUMMARY 2   /* length, ref_mask, moving, visible, keep, theta */
#define MONO_TRACK_ALL 3

int mono_track_abi_version(void);

/* centres [S, F, M, 3] float64, status [S, F, M] int32
 * -> tracks [S, Tmax, F, 2] int32, length / ref_mask [S, Tmax] int32, moving / visible / keep [S, Tmax] uint8, theta [S, Tmax] float64,
 * count / dropped [S] int32.  No workspace: the association's state lives in LDS. */
int mono_track_objects_f64(const double *centres, const int32_t *status, int S, int F, int M, int ref_frame, double d_track,
                           double d_move, double d_angle, double z0, int use_pseudo_lidar, int Tmax, int stages, int32_t *tracks,
                           int32_t *length, int32_t *ref_mask, uint8_t *moving, uint8_t *visible, uint8_t *keep, double *theta,
                           int32_t *count, int32_t *dropped, void *stream);

#ifdef __cplusplus
}
#endif
#endif
