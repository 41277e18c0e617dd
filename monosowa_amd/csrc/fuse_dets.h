// ---- BEV duplicate suppression and flip-view fusion of decoded KITTI rows (included by rotate_iou.hip) ----
// rows f64 [V*B, K, 14] (mono_decode_dets_f64's output, view v of image b at v*B + b) + count [V*B] + geom f64 [B, 10]
// -> out_rows f64 [B, V*K, 14], out_count [B], out_support [B, V*K].  One workgroup per image:
//   1. the candidates of an image go to LDS: id = v * K + j for j < count; the rows of view 1 (the mirrored frame) are brought back
//      into the frame (u -> W - u with the calibration left alone, as kitti_dataset.py's training flip) in double, unfused;
//   2. rank by score descending (exact ties: lower id first; NaN last, in id order) with extract_dets_kernel's counting scheme;
//   3. BEV rectangles (x, z, l, w, ry) in float32, in rank order;
//   4. the overlaps of the same-class pairs i < j (rank positions) in parallel: a wavefront takes 64 consecutive i of one j, every
//      lane one kitti::intersection_area (the evaluation's own f32 routine, criterion -1), and a ballot packs the 64 flags
//      `IoU >= threshold` (float32 compare; a NaN overlap is no match) into one 64-bit word of LDS -- written by one lane, no atomics;
//   5. the greedy walk on wavefront 0: lane l keeps, per 64-block, whether rank 64 c + l is a seed; candidate r reads its flag
//      words, a ballot of (seed && flag) finds the first seed it matches -- seeds are made in rank order, so the lowest rank IS
//      the first seed in seed order -- or r becomes a seed.  n iterations of at most 4 ballots, wave-uniform control, bounded;
//   6. a thread per cluster writes its row: the seed's row byte for byte (mode 0) or the score-weighted mean of its members summed
//      in member (rank) order (mode 1); rows, support behind the clusters are zero.
// Two candidates whose five float32 numbers are equal (finite, non-zero area) overlap by 1 without asking the routine.  The routine
// no longer needs that: it clips one rectangle in the other's frame and scores coincident, collinear, half-turned and one-ulp-apart
// rectangles by their exact overlap (rotate_iou.hip; the reference's vertex collection, which it used to mirror, passed or failed
// corners on coincident edges by rounding).  The shortcut stays as the contract of include/monosowa_kitti.h states it.
// A rectangle with a side that is not > 0 (zero, negative, NaN) is not handed to the routine either, which would return 0 for it,
// and matches nothing; a NaN position or heading leaves the routine without a vertex, a zero ratio.  So a NaN or degenerate box
// ends as its own seed.
namespace fuse {

constexpr int kThreads = 512;
constexpr int kMaxCand = 256;            // V * K the kernel accepts
constexpr int kWords = kMaxCand / 64;    // 64-bit flag words per candidate
constexpr int kRow = 14;
constexpr int kGeom = 10;

__device__ __forceinline__ double wrap_pi(double a) {        // the decode's ry wrap
#pragma clang fp contract(off)
  const double kPi = 3.141592653589793, kTwoPi = 2 * kPi;
  a = a > kPi ? a - kTwoPi : a;
  a = a < -kPi ? a + kTwoPi : a;
  return a;
}

__global__ __launch_bounds__(kThreads) void fuse_dets_kernel(const double *__restrict__ rows, const int *__restrict__ count,
                                                            const double *__restrict__ geom, float threshold, int mode,
                                                            double *__restrict__ out_rows, int *__restrict__ out_count,
                                                            int *__restrict__ out_support, int B, int K, int V) {
#pragma clang fp contract(off)
  __shared__ double row[kMaxCand * kRow];                    // by id; view 1 un-mirrored
  __shared__ double cls_of[kMaxCand];                        // by rank
  __shared__ unsigned long long match[kMaxCand * kWords];    // by rank j: bit i of word c = candidate 64 c + i (< j) overlaps j
  __shared__ float box[kMaxCand * 5];                        // by rank
  __shared__ short order[kMaxCand], seed_of[kMaxCand], seed_rank[kMaxCand];
  __shared__ unsigned char valid[kMaxCand];
  __shared__ int n_seeds;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, N = V * K;
  const double *g = geom + (long long)b * kGeom;
  const double W = g[0], cu = g[4], fu = g[6], tx = g[8];
  const double kPi = 3.141592653589793;

  // 1. candidates
  int n = 0;
  for (int v = 0; v < V; ++v) {
    const int c = count[v * B + b];
    n += c < 0 ? 0 : (c > K ? K : c);
  }
  for (int id = tid; id < N; id += kThreads) {
    const int v = id / K, j = id - v * K;
    valid[id] = j < count[v * B + b];
  }
  for (int e = tid; e < N * kRow; e += kThreads) {
    const int id = e / kRow, v = id / K, j = id - v * K;
    row[e] = j < count[v * B + b] ? rows[((long long)(v * B + b) * K + j) * kRow + (e - id * kRow)] : 0.0;
  }
  __syncthreads();
  for (int id = K + tid; id < N; id += kThreads) {           // view 1: back into the frame
    if (!valid[id]) continue;
    double *m = row + id * kRow;
    const double x1 = W - m[4], x2 = W - m[2];
    const double alpha = wrap_pi(kPi - m[1]);
    m[2] = x1;
    m[4] = x2;
    m[1] = alpha;
    m[9] = ((W - 2 * cu) * m[11]) / fu - m[9] + 2 * tx;
    m[12] = wrap_pi(alpha + atan2((x1 + x2) / 2 - cu, fu));
  }
  __syncthreads();

  // 2. rank: #(candidates that come first)
  for (int i = tid; i < N; i += kThreads) {
    if (!valid[i]) continue;
    const double s = row[i * kRow + 13];
    const bool s_nan = s != s;
    int rank = 0;
    for (int j = 0; j < N; ++j) {
      if (!valid[j]) continue;
      const double t = row[j * kRow + 13];
      const bool t_nan = t != t;
      rank += s_nan ? (!t_nan || j < i) : (!t_nan && (t > s || (t == s && j < i)));
    }
    order[rank] = (short)i;
  }
  __syncthreads();

  // 3. BEV rectangles in rank order
  for (int r = tid; r < n; r += kThreads) {
    const double *m = row + order[r] * kRow;
    float *q = box + r * 5;
    q[0] = (float)m[9];
    q[1] = (float)m[11];
    q[2] = (float)m[8];
    q[3] = (float)m[7];
    q[4] = (float)m[12];
    cls_of[r] = m[0];
  }
  __syncthreads();

  // 4. flags of the same-class pairs i < j
  const int blocks = (n + 63) / 64;
  for (int item = tid >> 6; item < blocks * n; item += kThreads / 64) {
    const int c = item / n, j = item - c * n, i = c * 64 + lane;
    if (c * 64 >= j) continue;                               // wave-uniform: no i < j in this block (never read by the walk)
    bool hit = false;
    if (i < j && cls_of[i] == cls_of[j]) {
      const float *bi = box + i * 5, *bj = box + j * 5;
      if (bi[2] > 0.f && bi[3] > 0.f && bj[2] > 0.f && bj[3] > 0.f) {      // a rectangle without an area matches nothing
        bool same = true;                                    // coincident rectangles: IoU 1 (both: see the header of this file)
#pragma unroll
        for (int k = 0; k < 5; ++k) same = same && bi[k] == bj[k] && fabsf(bi[k]) < INFINITY;
        hit = same || kitti::ratio(kitti::intersection_area(bi, bj), bi[2] * bi[3], bj[2] * bj[3], -1) >= threshold;
      }
    }
    const unsigned long long word = __ballot(hit);
    if (lane == 0) match[j * kWords + c] = word;
  }
  __syncthreads();

  // 5. the greedy walk, wavefront 0
  if (tid < 64) {
    unsigned is_seed = 0;                                    // bit c: rank 64 c + lane is a seed
    int seeds = 0;
    for (int r = 0; r < n; ++r) {
      int first = -1;
#pragma unroll
      for (int c = 0; c < kWords; ++c) {
        if (first >= 0 || c * 64 >= r) continue;             // wave-uniform
        const unsigned long long word = match[r * kWords + c];
        const unsigned long long found = __ballot(((is_seed >> c) & 1u) && ((word >> lane) & 1ull));
        if (found) first = c * 64 + __ffsll((long long)found) - 1;
      }
      if (first < 0) {
        if (lane == (r & 63)) is_seed |= 1u << (r >> 6);
        if (lane == 0) seed_rank[seeds] = (short)r;
        ++seeds;
        first = r;
      }
      if (lane == 0) seed_of[r] = (short)first;
    }
    if (lane == 0) n_seeds = seeds;
  }
  __syncthreads();

  // 6. a row per cluster, zeros behind them
  const int seeds = n_seeds;
  if (tid == 0) out_count[b] = seeds;
  for (int s = tid; s < N; s += kThreads) {
    double *o = out_rows + ((long long)b * N + s) * kRow;
    if (s >= seeds) {
      for (int c = 0; c < kRow; ++c) o[c] = 0.0;
      out_support[(long long)b * N + s] = 0;
      continue;
    }
    const int q = seed_rank[s];
    const double *sr = row + order[q] * kRow;
    int members = 0;
    if (mode == 0) {
      for (int r = q; r < n; ++r) members += seed_of[r] == q;
      for (int c = 0; c < kRow; ++c) o[c] = sr[c];
    } else {
      double sw = 0.0, ss = 0.0, sc = 0.0, best0 = 0.0, best1 = 0.0, acc[10];
      bool have0 = false, have1 = false;
#pragma unroll
      for (int c = 0; c < 10; ++c) acc[c] = 0.0;
      for (int r = q; r < n; ++r) {
        if (seed_of[r] != q) continue;
        const int id = order[r];
        const double *m = row + id * kRow;
        const double w = m[13];
        ++members;
        sw += w;
#pragma unroll
        for (int c = 0; c < 10; ++c) acc[c] += w * m[2 + c];
        ss += w * sin(m[12]);
        sc += w * cos(m[12]);
        if (id < K) {                                        // members come in score order: the first of a view is its best
          if (!have0) { best0 = w; have0 = true; }
        } else if (!have1) {
          best1 = w;
          have1 = true;
        }
      }
#pragma unroll
      for (int c = 0; c < 10; ++c) acc[c] = acc[c] / sw;
      const double ry = atan2(ss, sc);
      o[0] = sr[0];
      o[1] = wrap_pi(ry - atan2((acc[0] + acc[2]) / 2 - cu, fu));
#pragma unroll
      for (int c = 0; c < 10; ++c) o[2 + c] = acc[c];
      o[12] = ry;
      o[13] = (best0 + best1) / (double)V;
    }
    out_support[(long long)b * N + s] = members;
  }
}

}  // namespace fuse

extern "C" int mono_fuse_dets_f64(const double *rows, const int *count, const double *geom, double iou, int mode, double *out_rows,
                                  int *out_count, int *out_support, int B, int K, int V, void *stream_) {
  if (!rows || !count || !geom || !out_rows || !out_count || !out_support) return -1;
  if (B <= 0 || K <= 0 || V < 1 || V > 2 || (long long)V * K > fuse::kMaxCand || mode < 0 || mode > 1 || !(iou > 0.0 && iou <= 1.0))
    return -2;
  fuse::fuse_dets_kernel<<<B, fuse::kThreads, 0, (hipStream_t)stream_>>>(rows, count, geom, (float)iou, mode, out_rows, out_count,
                                                                        out_support, B, K, V);
  return (int)hipGetLastError();
}
