// Rotated-box overlaps for the KITTI evaluation: BEV IoU of rotated rectangles and camera-frame 3D
// box IoU, N x K pairs per call.  Replaces the numba-CUDA kernel of
// lib/datasets/kitti/kitti_eval_python/rotate_iou.py:263-330 (+ the CPU loop eval.py:197-223 for the 3D case).
//
// Same quantity as the reference -- the area of the intersection of two rotated rectangles, combined by `criterion` -- but NOT its
// vertex collection (corners kept by >= tests on absolute coordinates, edge crossings divided by a determinant that vanishes for
// parallel edges, a sort by pseudo-angle): that scheme returns 0, 1/3, values far above 1 or NaN on identical, collinear, half-turned
// and one-ulp-apart boxes, and loses digits on absolute coordinates at KITTI distances.  Here box 2 is expressed in box 1's frame
// (centre difference, heading difference), its four corners are clipped against box 1's four axis-aligned sides
// (Sutherland-Hodgman, at most 8 vertices) and the polygon is summed as a fan about its first vertex.  Every inside / outside test is
// taken on a coordinate relative to box 1, every divisor is the distance between a point inside and a point outside, and coincident
// and edge-sharing boxes score their exact overlap.  One thread per (box, query) pair, the 64 x 64 tile's boxes staged in LDS; pure f32.
#include <hip/hip_runtime.h>

#include "../../include/monosowa_kitti.h"

namespace kitti {

struct P2 { float x, y; };

constexpr int kMaxVerts = 8;             // a quadrilateral gains at most one vertex per clipping side

// The part of the convex polygon in[0..n) with s * c <= lim, c its x (AXIS 0) or y (AXIS 1) coordinate and s = +-1.  A vertex on the
// side is inside.  A crossing lies between a vertex inside and one outside, so sp and sq differ in sign and sp - sq is at least as
// large as either; its clipped coordinate is the side's own, not an interpolation.
template <int AXIS>
__device__ __forceinline__ int clip_side(const P2 *in, int n, P2 *out, float s, float lim) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    const P2 p = in[i], q = in[i + 1 == n ? 0 : i + 1];
    const float sp = lim - s * (AXIS ? p.y : p.x), sq = lim - s * (AXIS ? q.y : q.x);
    const bool p_in = sp >= 0.f, q_in = sq >= 0.f;
    if (p_in && m < kMaxVerts) out[m++] = p;
    if (p_in != q_in && m < kMaxVerts) {
      const float t = sp / (sp - sq);
      P2 r;
      if (AXIS) {
        r.x = p.x + t * (q.x - p.x);
        r.y = s * lim;
      } else {
        r.x = s * lim;
        r.y = p.y + t * (q.y - p.y);
      }
      out[m++] = r;
    }
  }
  return m;
}

// b = (cx, cy, w, h, angle): corners (-w/2,-h/2), (-w/2,h/2), (w/2,h/2), (w/2,-h/2) rotated clockwise by angle, as the reference has
// them.  A box with a side that is not > 0 (zero, negative, NaN) has no area to share: 0.  A NaN or infinite centre or heading fails
// every >= test and leaves no vertex: 0 as well.
__device__ float intersection_area(const float *b1, const float *b2) {
  if (!(b1[2] > 0.f && b1[3] > 0.f && b2[2] > 0.f && b2[3] > 0.f)) return 0.f;
  const float ca = cosf(b1[4]), sa = sinf(b1[4]);
  const float d = b2[4] - b1[4];                           // equal headings: cos, sin = 1, 0 exactly
  const float cd = cosf(d), sd = sinf(d);
  const float dx = b2[0] - b1[0], dy = b2[1] - b1[1];
  const float ox = ca * dx - sa * dy, oy = sa * dx + ca * dy;      // box 2's centre in box 1's frame
  const float hx = b2[2] * 0.5f, hy = b2[3] * 0.5f;
  const float xs[4] = {-hx, -hx, hx, hx}, ys[4] = {-hy, hy, hy, -hy};
  P2 u[kMaxVerts], v[kMaxVerts];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    u[i].x = cd * xs[i] + sd * ys[i] + ox;
    u[i].y = -sd * xs[i] + cd * ys[i] + oy;
  }
  const float lx = b1[2] * 0.5f, ly = b1[3] * 0.5f;
  int n = clip_side<0>(u, 4, v, 1.f, lx);
  n = clip_side<0>(v, n, u, -1.f, lx);
  n = clip_side<1>(u, n, v, 1.f, ly);
  n = clip_side<1>(v, n, u, -1.f, ly);
  if (n < 3) return 0.f;
  float twice = 0.f;                                       // shoelace fan about vertex 0, on differences from it
  for (int i = 1; i + 1 < n; ++i)
    twice += (u[i].x - u[0].x) * (u[i + 1].y - u[0].y) - (u[i].y - u[0].y) * (u[i + 1].x - u[0].x);
  const float area = fabsf(twice) * 0.5f;
  return area < INFINITY ? area : 0.f;                     // (a NaN compares false)
}

__device__ __forceinline__ float ratio(float inter, float a1, float a2, int criterion) {
  if (criterion == -1) return inter / (a1 + a2 - inter);
  if (criterion == 0) return inter / a1;
  if (criterion == 1) return inter / a2;
  return inter;
}

// MODE 0: BEV boxes [*, 5] = (cx, cy, w, h, angle), out = overlap by `criterion` (areas: a1 = QUERY, a2 = box, the
// argument order of the reference's device function).  MODE 1: camera-frame 3D boxes [*, 7] = (x, y, z, d3, d4, d5, ry)
// with BEV rectangle (x, z, d3, d5, ry), bottom y and height d4 (eval.py:197-230).
template <int MODE>
__global__ __launch_bounds__(64) void overlap_kernel(const float *__restrict__ boxes, const float *__restrict__ query,
                                                     float *__restrict__ out, long long N, long long K, int criterion) {
  constexpr int W = MODE ? 7 : 5;
  __shared__ float sb[64 * W], sq[64 * W];
  const long long r0 = (long long)blockIdx.x * 64, c0 = (long long)blockIdx.y * 64;
  const int rows = (int)min(64LL, N - r0), cols = (int)min(64LL, K - c0);
  const int tx = threadIdx.x;
  if (tx < rows)
    for (int i = 0; i < W; ++i) sb[tx * W + i] = boxes[(r0 + tx) * W + i];
  if (tx < cols)
    for (int i = 0; i < W; ++i) sq[tx * W + i] = query[(c0 + tx) * W + i];
  __syncthreads();
  if (tx >= rows) return;
  const float *b = sb + tx * W;
  for (int j = 0; j < cols; ++j) {
    const float *q = sq + j * W;
    float res;
    if (MODE == 0) {
      res = ratio(intersection_area(q, b), q[2] * q[3], b[2] * b[3], criterion);
    } else {
      const float bb[5] = {b[0], b[2], b[3], b[5], b[6]}, qq[5] = {q[0], q[2], q[3], q[5], q[6]};
      const float bev = intersection_area(qq, bb);
      res = 0.f;
      if (bev > 0.f) {
        const float ih = fminf(b[1], q[1]) - fmaxf(b[1] - b[4], q[1] - q[4]);
        if (ih > 0.f) res = ratio(ih * bev, b[3] * b[4] * b[5], q[3] * q[4] * q[5], criterion);
      }
    }
    out[(r0 + tx) * K + c0 + j] = res;
  }
}

}  // namespace kitti

// ---- detections from network outputs: lib/helpers/decode_helper.py:58-111 (extract_dets_from_outputs) as ONE kernel ----
// prob = sigmoid(logits); top-K over the Q * C scores of an image; query = index / C, class = index % C; gather of the
// query's box / heading / depth / size; cxcylrtb -> xyxy -> cxcywh; sigma = exp(-log variance).  One workgroup per image.
// The rank of a score is counted directly (N = Q * C is 150 in inference): rank = #(larger scores) + #(equal scores with a
// smaller index) -- the order torch.topk produces on distinct scores, and a fixed, documented order on exact ties (where
// torch's is unspecified).  Row layout (37 floats): [cls, score, x2d, y2d, w2d, h2d, depth, heading(24), size3d(3), x3d,
// y3d, sigma].  Every arithmetic step is the reference's own expression, individually rounded (no fused multiply-add).
namespace dets {

constexpr int kThreads = 1024;
constexpr int kMaxScores = 8192;        // Q * C the kernel accepts (32 KB of LDS)

__device__ __forceinline__ float add_rn(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__global__ __launch_bounds__(kThreads) void extract_dets_kernel(
    const float *__restrict__ logits, const float *__restrict__ boxes, const float *__restrict__ angle,
    const float *__restrict__ size3d, const float *__restrict__ depth, float *__restrict__ out, int Q, int C, int K) {
  __shared__ float score[kMaxScores];
  const int b = blockIdx.x, N = Q * C;
  const float *lg = logits + (long long)b * N;
  for (int i = threadIdx.x; i < N; i += kThreads) score[i] = 1.0f / (1.0f + expf(-lg[i]));      // at::sigmoid
  __syncthreads();
  for (int i = threadIdx.x; i < N; i += kThreads) {
    const float s = score[i];
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      const float t = score[j];
      rank += (t > s) || (t == s && j < i);
    }
    if (rank >= K) continue;
    const int q = i / C, cls = i - q * C;
    const float *bx = boxes + ((long long)b * Q + q) * 6;
    const float cx = bx[0], cy = bx[1];
    const float x0 = sub_rn(cx, bx[2]), y0 = sub_rn(cy, bx[4]), x1 = add_rn(cx, bx[3]), y1 = add_rn(cy, bx[5]);   // box_cxcylrtb_to_xyxy
    float *o = out + ((long long)b * K + rank) * 37;
    o[0] = (float)cls;
    o[1] = s;
    o[2] = add_rn(x0, x1) / 2;                                                                                   // box_xyxy_to_cxcywh
    o[3] = add_rn(y0, y1) / 2;
    o[4] = sub_rn(x1, x0);
    o[5] = sub_rn(y1, y0);
    const float *dp = depth + ((long long)b * Q + q) * 2;
    o[6] = dp[0];
    const float *an = angle + ((long long)b * Q + q) * 24;
    for (int k = 0; k < 24; ++k) o[7 + k] = an[k];
    const float *sz = size3d + ((long long)b * Q + q) * 3;
    o[31] = sz[0]; o[32] = sz[1]; o[33] = sz[2];
    o[34] = cx;
    o[35] = cy;
    o[36] = expf(-dp[1]);
  }
}

// ---- KITTI rows from detections: lib/helpers/decode_helper.py:8-55 (decode_detections) as ONE kernel, in double ----
// dets f32 [B, K, 37] + per-image geometry f64 [B, 10] = (img_w, img_h, height_crop, canonical_scale, cu, cv, fu, fv, tx, ty)
// -> rows f64 [B, K, 14] = (cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score), the rows with ~(score < threshold)
// compacted in rank order, the rest zero; count [B].  Every step is numpy's own expression with numpy's promotions: float32
// detections widen into float64 arithmetic, each product and sum is rounded on its own (no fused multiply-add), the
// threshold is compared in float32, the final score is a float32 product widened, `//` is numpy's floor division, arg-max
// takes the lowest index of the largest value (the first NaN, as numpy does).  Only ry goes through a library function
// (atan2).  One workgroup per image; a detection per thread.
constexpr int kDecodeThreads = 256;
constexpr int kDecodeMaxK = 4096;        // detections per image the kernel accepts (a 4 KB flag array in LDS)
constexpr int kGeomDoubles = 10;
constexpr int kRowDoubles = 14;

__device__ __forceinline__ double floor_divide(double a, double b) {        // numpy's npy_floor_divide for doubles
#pragma clang fp contract(off)
  if (b == 0.0) return a / b;
  const double mod = fmod(a, b);
  double div = (a - mod) / b;
  if (mod != 0.0 && ((b < 0.0) != (mod < 0.0))) div -= 1.0;
  if (div != 0.0) {
    double fl = floor(div);
    if (div - fl > 0.5) fl += 1.0;
    return fl;
  }
  return copysign(0.0, a / b);
}

__global__ __launch_bounds__(kDecodeThreads) void decode_dets_kernel(
    const float *__restrict__ dets, const double *__restrict__ geom, const double *__restrict__ cls_mean_size, float threshold,
    double *__restrict__ rows, int *__restrict__ count, int K, int C) {
#pragma clang fp contract(off)
  __shared__ unsigned char kept[kDecodeMaxK];
  const int b = blockIdx.x;
  const float *db = dets + (long long)b * K * 37;
  for (int j = threadIdx.x; j < K; j += kDecodeThreads) kept[j] = !(db[j * 37 + 1] < threshold);
  __syncthreads();
  int total = 0;
  for (int j = 0; j < K; ++j) total += kept[j];
  if (threadIdx.x == 0) count[b] = total;
  const double *g = geom + (long long)b * kGeomDoubles;
  const double img_w = g[0], img_h = g[1], cu = g[4], cv = g[5], fu = g[6], fv = g[7], tx = g[8], ty = g[9];
  const double crop_h = img_h / g[2];
  const double padding = floor_divide(img_h - crop_h, 2.0);
  const double kPi = 3.141592653589793, kTwoPi = 2 * kPi, kBin = kTwoPi / 12.0;
  double *rb = rows + (long long)b * K * kRowDoubles;
  for (int j = threadIdx.x; j < K; j += kDecodeThreads) {
    if (j >= total) {                                        // the tail behind the kept rows
      double *z = rb + (long long)j * kRowDoubles;
      for (int c = 0; c < kRowDoubles; ++c) z[c] = 0.0;
    }
    if (!kept[j]) continue;
    int pos = 0;
    for (int i = 0; i < j; ++i) pos += kept[i];
    const float *d = db + j * 37;
    const int cls = (int)(long long)d[0];
    const int cm = cls < 0 ? 0 : (cls >= C ? C - 1 : cls);   // (numpy raises on a class outside the table; never read outside it)
    const double x = (double)d[2] * img_w;
    const double y = (double)d[3] * crop_h + padding;
    const double w = (double)d[4] * img_w;
    const double h = (double)d[5] * crop_h;
    const double depth = (double)d[6] / g[3];
    const double dim0 = (double)d[31] + cls_mean_size[cm * 3 + 0];
    const double dim1 = (double)d[32] + cls_mean_size[cm * 3 + 1];
    const double dim2 = (double)d[33] + cls_mean_size[cm * 3 + 2];
    const double x3d = (double)d[34] * img_w;
    const double y3d = (double)d[35] * crop_h + padding;
    const double loc_x = ((x3d - cu) * depth) / fu + tx;
    const double loc_y = ((y3d - cv) * depth) / fv + ty + dim0 / 2;
    int bin = 0;
    float best = d[7];
    if (!(best != best)) {
      for (int k = 1; k < 12; ++k) {
        const float v = d[7 + k];
        if (!(v <= best)) {
          best = v;
          bin = k;
          if (v != v) break;
        }
      }
    }
    double alpha = (double)bin * kBin + (double)d[19 + bin];
    alpha = alpha > kPi ? alpha - kTwoPi : alpha;
    double ry = alpha + atan2(x - cu, fu);
    ry = ry > kPi ? ry - kTwoPi : ry;
    ry = ry < -kPi ? ry + kTwoPi : ry;
    const float final_score = d[1] * d[36];
    double *o = rb + (long long)pos * kRowDoubles;
    o[0] = (double)cls;
    o[1] = alpha;
    o[2] = x - w / 2;
    o[3] = y - h / 2;
    o[4] = x + w / 2;
    o[5] = y + h / 2;
    o[6] = dim0;
    o[7] = dim1;
    o[8] = dim2;
    o[9] = loc_x;
    o[10] = loc_y;
    o[11] = depth;
    o[12] = ry;
    o[13] = (double)final_score;
  }
}

}  // namespace dets

extern "C" {

int mono_extract_dets_f32(const float *logits, const float *boxes, const float *angle, const float *size3d, const float *depth,
                          float *out, int B, int Q, int C, int K, void *stream_) {
  if (!logits || !boxes || !angle || !size3d || !depth || !out) return -1;
  if (B <= 0 || Q <= 0 || C <= 0 || K <= 0 || K > Q * C || (long long)Q * C > dets::kMaxScores) return -2;
  dets::extract_dets_kernel<<<B, dets::kThreads, 0, (hipStream_t)stream_>>>(logits, boxes, angle, size3d, depth, out, Q, C, K);
  return (int)hipGetLastError();
}

int mono_decode_dets_f64(const float *dets, const double *geom, const double *cls_mean_size, double threshold, double *rows,
                         int *count, int B, int K, int C, void *stream_) {
  if (!dets || !geom || !cls_mean_size || !rows || !count) return -1;
  if (B <= 0 || K <= 0 || C <= 0 || K > dets::kDecodeMaxK) return -2;
  dets::decode_dets_kernel<<<B, dets::kDecodeThreads, 0, (hipStream_t)stream_>>>(dets, geom, cls_mean_size, (float)threshold, rows,
                                                                                count, K, C);
  return (int)hipGetLastError();
}

int mono_rotate_iou_f32(const float *boxes, const float *query, float *out, long long N, long long K, int criterion, void *stream_) {
  if (!boxes || !query || !out) return -1;
  if (N <= 0 || K <= 0 || criterion < -1 || criterion > 2) return -2;
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((K + 63) / 64));
  kitti::overlap_kernel<0><<<grid, 64, 0, (hipStream_t)stream_>>>(boxes, query, out, N, K, criterion);
  return (int)hipGetLastError();
}

int mono_box3d_overlap_f32(const float *boxes, const float *query, float *out, long long N, long long K, int criterion, void *stream_) {
  if (!boxes || !query || !out) return -1;
  if (N <= 0 || K <= 0 || criterion < -1 || criterion > 2) return -2;
  const dim3 grid((unsigned)((N + 63) / 64), (unsigned)((K + 63) / 64));
  kitti::overlap_kernel<1><<<grid, 64, 0, (hipStream_t)stream_>>>(boxes, query, out, N, K, criterion);
  return (int)hipGetLastError();
}

}  // extern "C"

#include "fuse_dets.h"     // duplicate suppression / flip-view fusion of the decoded rows (mono_fuse_dets_f64)
#include "encode_targets.h" // decoded rows -> the dataset's padded training targets (mono_encode_targets_f64)
#include "memory_merge.h"  // a pass's rows merged into the frame's remembered rows (mono_memory_merge_f64)
#include "kitti_ap.h"     // host-side AP accumulation of the same library (mono_kitti_tp_scores_f64, mono_kitti_pr_f64)
