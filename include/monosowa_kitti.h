/* monosowa_kitti.h -- C ABI of the inference / evaluation side: the rotated-box overlap kernels of the KITTI evaluation
 *  and the detection extraction of the inference loop (row f3).
 *
 * Replaces lib/datasets/kitti/kitti_eval_python/rotate_iou.py:263-330 (`rotate_iou_gpu_eval`, a numba-CUDA kernel) and
 * the CPU loop of eval.py:197-230 (`d3_box_overlap`).  Device pointers, asynchronous on `stream`.
 * criterion: -1 IoU, 0 intersection / area of the first operand, 1 intersection / area of the second, 2 intersection.
 * The intersection is the reference's quantity but not its method: the reference collects corners by >= tests on absolute
 * coordinates and divides edge crossings by a determinant that vanishes for parallel edges, which scores identical boxes 0 or 1/3
 * and collinear or one-ulp-apart boxes anything up to NaN.  Here one rectangle is clipped in the other's frame (float32), so that
 * identical and edge-sharing boxes score their exact overlap, and a box with a side that is not > 0 intersects nothing.
 * Return value: 0, -1 (NULL pointer), -2 (bad size / criterion) or a hipError_t.
 */
#ifndef MONOSOWA_KITTI_H
#define MONOSOWA_KITTI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* boxes [N, 5], query [K, 5] = (cx, cy, w, h, angle; clockwise positive) -> out [N, K].
 * As in the reference, criterion 0 divides by the QUERY box's area and 1 by the box's (rotate_iou.py:249-260, :289). */
int mono_rotate_iou_f32(const float *boxes, const float *query, float *out, long long N, long long K, int criterion, void *stream);

/* Camera-frame 3D boxes [*, 7] = (x, y, z, d3, d4, d5, ry): BEV rectangle (x, z, d3, d5, ry), bottom at y, height d4;
 * out [N, K] = 3D overlap (criterion 0: / volume of the box, 1: / volume of the query box, as eval.py:210-221). */
int mono_box3d_overlap_f32(const float *boxes, const float *query, float *out, long long N, long long K, int criterion, void *stream);

/* Inference post-process: lib/helpers/decode_helper.py:58-111 `extract_dets_from_outputs` as one kernel.
 * logits [B, Q, C], boxes [B, Q, 6] (cx, cy, l, r, t, b), angle [B, Q, 24], size3d [B, Q, 3], depth [B, Q, 2] ->
 * out [B, K, 37] = [cls, score, x2d, y2d, w2d, h2d, depth, heading(24), size3d(3), x3d, y3d, sigma], the K best
 * sigmoid(logit) scores of each image in descending order (exact ties: smaller flat index first).  Q * C <= 8192. */
int mono_extract_dets_f32(const float *logits, const float *boxes, const float *angle, const float *size3d, const float *depth,
                          float *out, int B, int Q, int C, int K, void *stream);

/* KITTI rows of the detections (the public Detector's decode): lib/helpers/decode_helper.py:8-55 `decode_detections` as one
 * kernel in double, numpy's promotions kept (float32 detections widened; the threshold compared in float32; the final score a
 * float32 product, widened; `//` for the padding; arg-max ties to the lowest index).
 * dets [B, K, 37] (mono_extract_dets_f32's rows), geom f64 [B, 10] = (img_w, img_h, height_crop, canonical_scale, cu, cv, fu,
 * fv, tx, ty), cls_mean_size f64 [C, 3] -> rows f64 [B, K, 14] = (cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score):
 * the rows with ~(score < threshold) compacted in rank order, the rest zero; count int32 [B].  K <= 4096. */
int mono_decode_dets_f64(const float *dets, const double *geom, const double *cls_mean_size, double threshold, double *rows,
                         int *count, int B, int K, int C, void *stream);

/* Duplicate suppression by rotated BEV overlap and fusion of the mirrored view (tester.nms_iou / flip_tta / fuse), one kernel on
 * mono_decode_dets_f64's rows.  rows f64 [V*B, K, 14] and count [V*B]: view v of image b at index v*B + b, view 1 decoded from the
 * mirrored frame with the image's own geometry row; geom f64 [B, 10].  Candidates: id j for view 0, K + j for view 1 brought back
 * into the frame (x1' = W - x2, x2' = W - x1, alpha' = wrap(pi - alpha), x' = ((W - 2 cu) z) / fu - x + 2 tx,
 * ry' = wrap(alpha' + atan2((x1' + x2') / 2 - cu, fu)); double, unfused).  Order: score descending, exact ties by lower id, NaN
 * last.  A candidate joins the first seed of its class whose BEV rectangle (x, z, l, w, ry; float32, the evaluation's
 * intersection routine, criterion -1; two rectangles equal in all five float32 numbers, finite, overlap by 1; a
 * rectangle with a side that is not > 0 overlaps nothing) it overlaps by IoU >= iou (float32 compare; NaN never matches), else it
 * becomes a seed.
 * out_rows f64 [B, V*K, 14]: one row per seed in seed order, zeros behind; out_count int32 [B]; out_support int32 [B, V*K]: members
 * per cluster.  mode 0: the seed's row, byte for byte.  mode 1: columns x1..z = sum(w v) / sum(w) over the members in order with
 * w = score, ry = atan2(sum w sin ry, sum w cos ry), alpha = wrap(ry - atan2((x1 + x2) / 2 - cu, fu)), cls the seed's,
 * score = (best member score of view 0 + of view 1, 0 without a member) / V.  V in {1, 2}, V*K <= 256, iou in (0, 1];
 * otherwise -2. */
int mono_fuse_dets_f64(const double *rows, const int *count, const double *geom, double iou, int mode, double *out_rows,
                       int *out_count, int *out_support, int B, int K, int V, void *stream);

/* The inverse of mono_decode_dets_f64 for self-training: decoded (and fused) rows -> the padded target arrays the criterion reads,
 * in the frame of the student's own flip and crop; one kernel, one wavefront per image, one lane per slot.
 * rows f64 [B, R, 14], count int32 [B] (kept rows first), records f64 [B, 23] = (P2's 12 float32 values, img_w, img_h, flip,
 * the six numbers of the crop's affine `trans`, crop_scale, canonical_scale), cls_mean_size f64 [C, 3].
 * writelist_mask: bit c set when class c is trained on; depth_mode 0 'normal' (z * crop_scale), 1 'inverse' (z / crop_scale), 2 'none';
 * weight_mode 0: label_weight = the row's score (0 for a score that is negative or not finite), 1: = weight.
 * outputs: 17 device pointers (a host array), [B, max_objs, ...] each, in this order and with the dataset's dtypes: labels int8,
 * boxes f32 [4], boxes_3d f32 [6], depth f32 [1], size_2d f32 [2], size_3d f32 [3], src_size_3d f32 [3], heading_bin int64 [1],
 * heading_res f32 [1], mask_2d bool, calibs f32 [3, 4], indices int64, objects f32 [7], label_weight f32, ignore_boxes f32 [4],
 * ignore_mask bool, n_ignore int32 [B].  Every byte of every output is written.
 * Slot i < min(count, R, max_objs) is line i of the label file write_kitti_results(..., dontcare_below=min_score) would write from the
 * rows if it wrote every number exactly -- a row with !(score >= min_score), NaN included, as a DontCare line -- read by
 * KITTI_Dataset.__getitem__ on a training split with label_weights 'score' and ignore_regions on under the record's flip and crop
 * (aug_calib off): box2d and pos float32, truncation and occlusion 0, level UnKnown for !(y2 - y1 + 1 >= 25), the depth gate [2, 65]
 * on the unscaled float32 z, the centre-inside test, the negative l / r / t / b rule with clip_2d, z *= canonical_scale before
 * depth and objects, the heading recomputed in float32 from the flipped ry and box centre, every value rounded to its array's
 * dtype; label_weight 1 behind the lines.  The ignore boxes (DontCare lines and writelist lines that end as no target; empty ones
 * dropped) are packed at the front in line order, unused slots zero; n_ignore counts them.  rect_to_img's and affine_transform's
 * products run left to right in double, each operation rounded (numpy hands them to BLAS); the heading's float32 atan2 is the
 * double one rounded.  max_objs <= 64, C <= 31; otherwise -2. */
int mono_encode_targets_f64(const double *rows, const int *count, const double *records, const double *cls_mean_size,
                            int writelist_mask, int depth_mode, int clip_2d, double min_score, int weight_mode, double weight,
                            int res_w, int res_h, int B, int R, int C, int max_objs, void *const *outputs, void *stream);

/* The label memory of self-training (trainer.teacher_memory): one pass's rows of a frame merged into the rows remembered for it.
 * rows f64 [B, R, 14] and count int32 [B] as mono_fuse_dets_f64 / mono_decode_dets_f64 leave them (the raw frame's coordinates);
 * frame int32 [B]: the position of image b's frame in the bank, DISTINCT within a call (one workgroup owns one frame's block);
 * bank f64 [N, M, 16] and bank_count int32 [N], updated in place.  Frame f holds k = clamp(bank_count[f], 0, M) entries of 16
 * doubles: columns 0..13 a KITTI row in mono_decode_dets_f64's column order with column 13 the smoothed score, column 14 `hits`,
 * column 15 `misses` (consecutive passes without a match).  Image b brings n = clamp(count[b], 0, R) rows in their order.
 * w = 1.0 - momentum in double; everything in double, every operation rounded (no contraction).
 *  1. Eligible: a row takes part only when its score is finite; the others are counted as `skipped` and otherwise ignored.
 *  2. Flags: F[i][e] when row i and entry e have equal class (column 0 compared as double) and their BEV rectangles (x, z, l, w, ry;
 *     rounded to float32) overlap by IoU >= (float)iou -- mono_fuse_dets_f64's test: the evaluation's intersection routine on (row,
 *     entry) with criterion -1, compared in float32, a NaN never matches; two rectangles equal in all five float32 numbers, all five
 *     finite, overlap by 1 without the routine (the shortcut fires for nothing else: an infinite or NaN number goes to the routine,
 *     which finds no overlap); a rectangle with a side that is not > 0 matches nothing, an equal one included.
 *  3. Walk, in row order: eligible row i claims the lowest-index unclaimed entry e with F[i][e], else it is unmatched.
 *  4. Updates.  Claimed entry: columns 0..12 become the row's byte for byte; d = s_i - s; t = w * d; s' = s + t (three roundings);
 *     hits += 1, misses = 0.  Unclaimed entry: d = 0.0 - s; t = w * d; s' = s + t; columns 0..12 and hits stay, misses += 1.
 *     Unmatched eligible row: a candidate with columns 0..13 the row's byte for byte, hits = 1, misses = 0.
 *  5. Drop: a candidate, old entry or new row, with !(s' >= drop_below) -- a NaN included -- is dropped.
 *  6. Order: the survivors by s' descending; exact ties: old entries before new rows, old entries in slot order, new rows in row
 *     order (ranked by counting).  The first M stay, the rest are evicted.
 *  7. Writes: the frame's whole M x 16 block (survivors in order, zeros behind) and bank_count[f]; out_rows f64 [B, M, 14] = the
 *     survivors' columns 0..13 in the same order, zeros behind; out_count int32 [B]; stats int32 [B, 6] = (matched: entries
 *     claimed; created: unmatched eligible rows; missed: unclaimed entries; dropped; evicted; skipped), so that
 *     k + created - dropped - evicted = out_count.  Blocks of frames the call does not name are not touched.
 * A frame[b] outside [0, N): out_count 0, zero rows, zero stats, no bank access.
 * It follows (P1) that on an empty block n <= M rows with finite scores >= drop_below in non-increasing order come back as they
 * are, byte for byte, and (P3) that merging the same rows (sides > 0) again changes only `hits`: s - s is exactly 0 and every row's
 * lowest unclaimed match is itself.  momentum -> 0 does not make s' = s_i (s + (s_i - s) rounds); 0 is outside the interval.
 * Return: 0, -1 (NULL pointer), -2 (M not in 1..64, R not in 1..256, B or N negative, iou outside (0, 1], momentum outside (0, 1))
 * or a hipError_t. */
int mono_memory_merge_f64(const double *rows, const int *count, const int *frame, double *bank, int *bank_count, double momentum,
                          double iou, double drop_below, double *out_rows, int *out_count, int *stats, int B, int R, int N, int M,
                          void *stream);

/* KITTI AP accumulation, HOST functions: the official matching protocol as kitti_eval_python/eval.py:234-410
 * runs it (numba there), one call per (class, difficulty, min_overlap) over all images.  Host pointers.
 *   n_gt / n_dt / n_dc [n_images]: boxes per image;   overlaps: the images' [n_dt, n_gt] matrices (row = detection), concatenated;
 *   gt_data [sum n_gt, 5] = (x1, y1, x2, y2, alpha);   dt_data [sum n_dt, 6] = (x1, y1, x2, y2, alpha, score);
 *   ignored_gt / ignored_dt: 0 evaluate, 1 ignore, -1 other class (clean_data, eval.py:29-80);   dc_boxes [sum n_dc, 4].
 * mono_kitti_tp_scores_f64: scores of the true positives when every detection takes part (first pass, eval.py:563-577);
 *   scores_out has room for sum n_gt values.
 * mono_kitti_pr_f64: pr[t] += (tp, fp, fn, orientation similarity) at each score threshold (second pass, eval.py:363-410);
 *   metric 0 also forgives detections inside DontCare boxes.  Return 0, or -1 for a NULL pointer. */
int mono_kitti_tp_scores_f64(long long n_images, const int64_t *n_gt, const int64_t *n_dt, const int64_t *n_dc,
                             const double *overlaps, const double *gt_data, const double *dt_data, const int64_t *ignored_gt,
                             const int64_t *ignored_dt, const double *dc_boxes, int metric, double min_overlap,
                             double *scores_out, long long *n_scores);
int mono_kitti_pr_f64(long long n_images, const int64_t *n_gt, const int64_t *n_dt, const int64_t *n_dc, const double *overlaps,
                      const double *gt_data, const double *dt_data, const int64_t *ignored_gt, const int64_t *ignored_dt,
                      const double *dc_boxes, int metric, double min_overlap, const double *thresholds, long long n_thresholds,
                      int compute_aos, double *pr);

#ifdef __cplusplus
}
#endif
#endif
