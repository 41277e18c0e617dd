// Object tracks for gfx950 (include/monosowa_track.h states the rule): the centres and statuses of the object-cloud stage to tracks,
// the moving / standing decision, the heading of a moving track and the keep flag.  Exact and bit-reproducible but for atan2.
//
//   mono_track_objects_f64   two launches:
//     associate_kernel   one workgroup per window, sequential over its frames.  Per frame: an ordered compaction of the frame's
//                        detections (ballot and population count), one lane per track forms the prediction from the track's last
//                        five centres, one lane per detection scans the predictions for a(z) while one lane per track scans the
//                        detections for b(t), the mutual test, new-track indices by a second ballot prefix in detection order, and
//                        one lane per track writes the frame's entry of the table.  Six barriers per frame with a detection, three
//                        without.  The tracks' state (last five centres, prediction, length, b(t), the frame's view) lives in LDS:
//                        156 bytes per track, 40 per slot, 150,048 bytes at the limits.
//     summary_kernel     one lane per track over all S * Tmax rows of the table: length, visibility, the two-pass mean and variance
//                        of the differences, the heading's candidate angles in LDS (11 doubles per lane, sorted by insertion).
//
// No float atomics, no global atomics, no workspace.  A kernel boundary is the only hand-off between workgroups.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monosowa_track.h"

// the rule rounds every product and sum on its own
#pragma clang fp contract(off)

namespace track {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kMaxT = MONO_TRACK_MAX_TRACKS;
constexpr int kMaxM = MONO_LIFT_MAX_M;
constexpr int kRing = 5;     // the centres a prediction reads
constexpr int kAngles = 11;  // five a side, and the last one repeated when the count is even
static_assert(kMaxM <= kThreads, "one lane per slot of a frame");

__device__ __forceinline__ bool finite3(double x, double y, double z) {
  return fabs(x) <= DBL_MAX && fabs(y) <= DBL_MAX && fabs(z) <= DBL_MAX;
}

__device__ __forceinline__ double square3(double dx, double dy, double dz) { return (dx * dx + dy * dy) + dz * dz; }

// the number of set flags in the threads before this one, and in all of them; one barrier inside.  `sums` is not to be written
// again before the next barrier.
__device__ __forceinline__ int prefix(bool flag, int *sums, int &total) {
  const unsigned long long bal = __ballot(flag);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0) sums[wave] = __popcll(bal);
  __syncthreads();
  int before = __popcll(bal & ((1ull << lane) - 1ull));
  total = 0;
  for (int w = 0; w < kWaves; ++w) {
    const int c = sums[w];
    before += w < wave ? c : 0;
    total += c;
  }
  return before;
}

// ---------------------------------------------------------------------------------------------------------------- association
__global__ __launch_bounds__(kThreads) void associate_kernel(const double *__restrict__ centres, const int *__restrict__ status, int F,
                                                             int M, double dt2, int Tmax, int *__restrict__ tracks,
                                                             int *__restrict__ count, int *__restrict__ dropped) {
  __shared__ double ring[kMaxT][kRing][3];  // view n of a track lies in ring[n % 5]
  __shared__ double pred[kMaxT][3];
  __shared__ int len[kMaxT], bt[kMaxT], cur[kMaxT];
  __shared__ double dc[kMaxM][3], qa[kMaxM];
  __shared__ int dm[kMaxM], at[kMaxM];
  __shared__ int sums_d[kWaves], sums_n[kWaves];
  const int s = blockIdx.x, tid = threadIdx.x;
  centres += (size_t)s * F * M * 3;
  status += (size_t)s * F * M;
  tracks += (size_t)s * Tmax * F * 2;
  int T = 0, drop = 0;  // the same in every thread
  for (int f = 0; f < F; ++f) {
    // the frame's detections, in slot order
    bool ok = false;
    double cx = 0.0, cy = 0.0, cz = 0.0;
    if (tid < M && (status[f * M + tid] & 7) == MONO_LIFT_OK) {
      const double *c = centres + (size_t)(f * M + tid) * 3;
      cx = c[0], cy = c[1], cz = c[2];
      ok = finite3(cx, cy, cz);
    }
    int D;
    const int slot = prefix(ok, sums_d, D);
    if (ok) {
      dc[slot][0] = cx, dc[slot][1] = cy, dc[slot][2] = cz;
      dm[slot] = tid;
    }
    // every prediction of the frame, before any append
    for (int t = tid; t < Tmax; t += kThreads) {
      cur[t] = -1;
      if (t < T && D > 0) {
        const int n = len[t];
        const double *last = ring[t][(n - 1) % kRing];
        if (n == 1) {
          pred[t][0] = last[0], pred[t][1] = last[1], pred[t][2] = last[2];
        } else {
          const int k = n - 1 < 4 ? n - 1 : 4;
          for (int a = 0; a < 3; ++a) {
            double sum = last[a] - ring[t][(n - 2) % kRing][a];
            for (int j = 2; j <= k; ++j) sum = sum + (ring[t][(n - j) % kRing][a] - ring[t][(n - j - 1) % kRing][a]);
            pred[t][a] = sum / (double)k + last[a];
          }
        }
      }
    }
    __syncthreads();
    if (D > 0) {  // D and T are uniform: so is every barrier below
      if (T > 0) {
        if (tid < D) {  // a(z): the nearest prediction
          const double x = dc[tid][0], y = dc[tid][1], z = dc[tid][2];
          double best = square3(x - pred[0][0], y - pred[0][1], z - pred[0][2]);
          int a = 0;
          for (int t = 1; t < T; ++t) {
            const double q = square3(x - pred[t][0], y - pred[t][1], z - pred[t][2]);
            if (q < best) best = q, a = t;
          }
          at[tid] = a, qa[tid] = best;
        }
        for (int t = tid; t < T; t += kThreads) {  // b(t): the nearest detection
          const double x = pred[t][0], y = pred[t][1], z = pred[t][2];
          double best = square3(dc[0][0] - x, dc[0][1] - y, dc[0][2] - z);
          int b = 0;
          for (int d = 1; d < D; ++d) {
            const double q = square3(dc[d][0] - x, dc[d][1] - y, dc[d][2] - z);
            if (q < best) best = q, b = d;
          }
          bt[t] = b;
        }
      }
      __syncthreads();
      bool matched = false;
      int a = 0;
      if (tid < D && T > 0) {
        a = at[tid];
        matched = bt[a] == tid && qa[tid] < dt2;
      }
      int opened;
      const int rank = prefix(tid < D && !matched, sums_n, opened);
      if (tid < D) {
        const int t = matched ? a : T + rank;
        if (t < Tmax) {  // beyond: dropped
          const int n = matched ? len[t] : 0;
          double *to = ring[t][n % kRing];
          to[0] = dc[tid][0], to[1] = dc[tid][1], to[2] = dc[tid][2];
          len[t] = n + 1;
          cur[t] = dm[tid];
        }
      }
      const int room = Tmax - T;
      drop += opened > room ? opened - room : 0;
      T += opened > room ? room : opened;
      __syncthreads();
    }
    for (int t = tid; t < Tmax; t += kThreads) {  // the frame's entry of every row, written once
      const int m = cur[t];
      int *to = tracks + ((size_t)t * F + f) * 2;
      to[0] = m >= 0 ? f : -1;
      to[1] = m;
    }
    __syncthreads();
  }
  if (tid == 0) count[s] = T, dropped[s] = drop;
}

// ---------------------------------------------------------------------------------------------------------------- per track
__global__ __launch_bounds__(kThreads) void summary_kernel(const double *__restrict__ centres, const int *__restrict__ tracks, int rows,
                                                           int F, int M, int Tmax, int ref_frame, double dm2, double da2, double zz,
                                                           int use_pseudo_lidar, int *__restrict__ length, int *__restrict__ ref_mask,
                                                           uint8_t *__restrict__ moving, uint8_t *__restrict__ visible,
                                                           uint8_t *__restrict__ keep, double *__restrict__ theta) {
  __shared__ double ang[kAngles][kThreads];
  const int tid = threadIdx.x, g = blockIdx.x * kThreads + tid;
  if (g >= rows) return;  // no barrier below
  const int *row = tracks + (size_t)g * F * 2 + 1;  // the slot of frame f at row[2 f]
  const double *c = centres + (size_t)(g / Tmax) * F * M * 3;
  auto has = [&](int f) { return (unsigned)row[2 * f] < (unsigned)M; };  // a view in frame f
  auto at = [&](int f, int a) { return c[((size_t)f * M + row[2 * f]) * 3 + a]; };
  int n = 0, first = -1, last = -1;
  for (int f = 0; f < F; ++f)
    if (has(f)) {
      if (first < 0) first = f;
      last = f;
      ++n;
    }
  const int rm = ref_frame >= 0 && ref_frame < F && has(ref_frame) ? row[2 * ref_frame] : -1;
  const bool vis = rm >= 0;
  bool mov = false;
  if (n - 1 > 1) {
    const double N = (double)(n - 1);
    double mean[3], var[3], net[3];
    for (int a = 0; a < 3; ++a) {
      double sum = 0.0, prev = at(first, a);
      for (int f = first + 1; f <= last; ++f)
        if (has(f)) {
          const double v = at(f, a);
          sum = sum + (v - prev);
          prev = v;
        }
      mean[a] = sum / N;
      sum = 0.0, prev = at(first, a);
      for (int f = first + 1; f <= last; ++f)
        if (has(f)) {
          const double v = at(f, a), e = (v - prev) - mean[a];
          sum = sum + e * e;
          prev = v;
        }
      var[a] = sum / N;
      net[a] = at(last, a) - at(first, a);
    }
    const double mm = square3(mean[0], mean[1], mean[2]), vv = (var[0] + var[1]) + var[2];
    mov = mm > (zz * 0.5) * vv && square3(net[0], net[1], net[2]) > dm2;
  }
  double th = NAN;
  if (mov && vis && n >= 3) {
    const double rx = at(ref_frame, 0), rz = at(ref_frame, 2);
    int na = 0;
    for (int f = ref_frame - 1, taken = 0; f >= 0 && taken < 5; --f)
      if (has(f)) {
        const double dx = rx - at(f, 0), dz = rz - at(f, 2);
        if (dx * dx + dz * dz > da2) ang[na++][tid] = atan2(dz, dx), ++taken;
      }
    for (int f = ref_frame + 1, taken = 0; f < F && taken < 5; ++f)
      if (has(f)) {
        const double dx = at(f, 0) - rx, dz = at(f, 2) - rz;
        if (dx * dx + dz * dz > da2) ang[na++][tid] = atan2(dz, dx), ++taken;
      }
    if (na >= 3) {
      if (na % 2 == 0) ang[na][tid] = ang[na - 1][tid], ++na;
      for (int i = 1; i < na; ++i) {  // sorted by insertion
        const double v = ang[i][tid];
        int j = i;
        for (; j > 0 && ang[j - 1][tid] > v; --j) ang[j][tid] = ang[j - 1][tid];
        ang[j][tid] = v;
      }
      th = (-ang[na / 2][tid]) + MONO_TRACK_HALF_PI;
    }
  }
  length[g] = n;
  ref_mask[g] = rm;
  moving[g] = mov;
  visible[g] = vis;
  keep[g] = n > 0 && (vis || (!use_pseudo_lidar && !mov));  // a row beyond the count keeps nothing
  theta[g] = th;
}

}  // namespace track

extern "C" {

int mono_track_abi_version(void) { return MONO_TRACK_ABI_VERSION; }

int mono_track_objects_f64(const double *centres, const int32_t *status, int S, int F, int M, int ref_frame, double d_track,
                           double d_move, double d_angle, double z0, int use_pseudo_lidar, int Tmax, int stages, int32_t *tracks,
                           int32_t *length, int32_t *ref_mask, uint8_t *moving, uint8_t *visible, uint8_t *keep, double *theta,
                           int32_t *count, int32_t *dropped, void *stream) {
  if (!centres || !status || !tracks || !length || !ref_mask || !moving || !visible || !keep || !theta || !count || !dropped)
    return MONO_TRACK_NULL;
  if (S < 1 || F < 1 || M < 1 || Tmax < 1 || !(d_track >= 0.0 && d_track <= DBL_MAX) || !(d_move >= 0.0 && d_move <= DBL_MAX) ||
      !(d_angle >= 0.0 && d_angle <= DBL_MAX) || !(z0 >= 0.0 && z0 <= DBL_MAX) || stages < 1 || stages > MONO_TRACK_ALL)
    return MONO_TRACK_BAD_SIZE;
  if (S > MONO_TRACK_MAX_WINDOWS || F > MONO_LIFT_MAX_VIEWS || M > MONO_LIFT_MAX_M || Tmax > MONO_TRACK_MAX_TRACKS)
    return MONO_TRACK_TOO_LARGE;
  hipStream_t s = (hipStream_t)stream;
  const dim3 block(track::kThreads);
  if (stages & MONO_TRACK_STAGE_ASSOCIATE)
    track::associate_kernel<<<dim3(S), block, 0, s>>>(centres, status, F, M, d_track * d_track, Tmax, tracks, count, dropped);
  if (stages & MONO_TRACK_STAGE_SUMMARY) {
    const int rows = S * Tmax;
    track::summary_kernel<<<dim3((rows + track::kThreads - 1) / track::kThreads), block, 0, s>>>(
        centres, tracks, rows, F, M, Tmax, ref_frame, d_move * d_move, d_angle * d_angle, z0 * z0, use_pseudo_lidar, length, ref_mask,
        moving, visible, keep, theta);
  }
  return (int)hipGetLastError();
}
}
