// Object clouds for gfx950 (include/monosowa_lift.h states the rule): a depth map and instance masks to each object's point cloud,
// centre and range, and the views of a track to the padded clouds of the template search.  Exact and bit-reproducible.
//
//   mono_lift_objects_f32   four launches, one workgroup per (frame, mask) slot in each:
//     box_kernel       the one pass over the whole mask (16-byte loads): area, bounding box, truncated, s
//     columns_kernel   one thread per column of the box: a sweep down and a sweep up, the vertical distance to the nearest pixel
//                      that is not set, clipped at s + 1
//     rows_kernel      one thread per pixel of the box: min over |du| <= s of that distance + |du| (it leaves at |du| >= the minimum
//                      so far), the three point sets as bits of one byte, their sizes
//     cloud_kernel     medians by radix selection (four passes of 8 bits, the three axes and both middle ranks in one pass, integer
//                      counters in LDS), the circle, range and sign tests in double, an ordered compaction by ballot and population
//                      count, chunk after chunk
//   mono_lift_gather_f32    one workgroup per track: ranks by counting (a stable sort without a sort), offsets, medians of the
//                           centres, the even-spacing copy
//
// No float atomics, no global atomics.  A kernel boundary is the only hand-off between workgroups.
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "../../include/monosowa_lift.h"

// the rule rounds every product and sum on its own
#pragma clang fp contract(off)

namespace lift {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr int kRec = MONO_LIFT_RECORD_INTS;
// the record's fields
enum { rArea = 0, rRow0, rRow1, rCol0, rCol1, rS, rTrunc, rNs, rN1, rN0, rShrink, rBit };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// sum / min / max over the workgroup, the same value in every thread
template <int Op>
__device__ __forceinline__ int reduce(int v, int *scratch) {
  const int tid = threadIdx.x;
  __syncthreads();
  scratch[tid] = v;
  __syncthreads();
  for (int step = kThreads / 2; step > 0; step >>= 1) {
    if (tid < step) {
      const int a = scratch[tid], b = scratch[tid + step];
      scratch[tid] = Op == 0 ? a + b : (Op == 1 ? (a < b ? a : b) : (a > b ? a : b));
    }
    __syncthreads();
  }
  return scratch[0];
}

// ---------------------------------------------------------------------------------------------------------------- area and box
__global__ __launch_bounds__(kThreads) void box_kernel(const uint8_t *__restrict__ masks, const int *__restrict__ mask_count, int M,
                                                       int H, int W, int *__restrict__ record) {
  __shared__ int scratch[kThreads];
  const int slot = blockIdx.x, tid = threadIdx.x;
  const int f = slot / M, m = slot - f * M;
  int *rec = record + (size_t)slot * kRec;
  if (m >= clampi(mask_count[f], 0, M)) {
    if (tid == 0) rec[rArea] = -1;                     // ABSENT
    return;
  }
  const int n = H * W;
  const uint8_t *mk = masks + (size_t)slot * n;
  int area = 0, row0 = INT_MAX, row1 = -1, col0 = INT_MAX, col1 = -1;
  auto take = [&](int i) {
    const int v = i / W, u = i - v * W;
    ++area;
    row0 = v < row0 ? v : row0, row1 = v > row1 ? v : row1;
    col0 = u < col0 ? u : col0, col1 = u > col1 ? u : col1;
  };
  int head = (int)((16 - ((uintptr_t)mk & 15)) & 15);
  head = head < n ? head : n;
  const int nvec = (n - head) / 16;
  for (int i = tid; i < head; i += kThreads)
    if (mk[i]) take(i);
  const uint4 *body = (const uint4 *)(mk + head);
  for (int q = tid; q < nvec; q += kThreads) {
    const uint4 w = body[q];
    if ((w.x | w.y | w.z | w.w) == 0) continue;
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
    for (int k = 0; k < 4; ++k)
      for (int b = 0; b < 4; ++b)
        if ((word[k] >> (8 * b)) & 0xffu) take(head + q * 16 + k * 4 + b);
  }
  for (int i = head + nvec * 16 + tid; i < n; i += kThreads)
    if (mk[i]) take(i);
  area = reduce<0>(area, scratch);
  row0 = reduce<1>(row0, scratch), row1 = reduce<2>(row1, scratch);
  col0 = reduce<1>(col0, scratch), col1 = reduce<2>(col1, scratch);
  if (tid == 0) {
    int root = (int)sqrt((double)area);
    while (root > 0 && root * root > area) --root;
    while ((root + 1) * (root + 1) <= area) ++root;
    rec[rArea] = area;
    rec[rRow0] = area ? row0 : 0, rec[rRow1] = area ? row1 : -1;
    rec[rCol0] = area ? col0 : 0, rec[rCol1] = area ? col1 : -1;
    rec[rS] = 2 + root / 10;
    rec[rTrunc] = area && (row0 < 10 || row1 >= H - 10);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the column pass
__global__ __launch_bounds__(kThreads) void columns_kernel(const uint8_t *__restrict__ masks, int H, int W, const int *__restrict__ record,
                                                           uint8_t *__restrict__ dist) {
  const int slot = blockIdx.x;
  const int *rec = record + (size_t)slot * kRec;
  if (rec[rArea] <= 0) return;
  const int row0 = rec[rRow0], row1 = rec[rRow1], col0 = rec[rCol0], col1 = rec[rCol1];
  const int cap = rec[rS] + 1;                         // <= 255 by MONO_LIFT_MAX_PIXELS: it fits the byte
  const uint8_t *mk = masks + (size_t)slot * H * W;
  uint8_t *out = dist + (size_t)slot * H * W;
  for (int c = col0 + (int)threadIdx.x; c <= col1; c += kThreads) {
    int run = row0 == 0 ? cap : 0;                     // above the image counts as set; above the box nothing is set
    for (int r = row0; r <= row1; ++r) {
      run = mk[(size_t)r * W + c] ? (run + 1 < cap ? run + 1 : cap) : 0;
      out[(size_t)r * W + c] = (uint8_t)run;
    }
    run = row1 == H - 1 ? cap : 0;
    for (int r = row1; r >= row0; --r) {
      const int down = out[(size_t)r * W + c];
      run = down ? (run + 1 < cap ? run + 1 : cap) : 0;
      if (run < down) out[(size_t)r * W + c] = (uint8_t)run;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- the row pass
__device__ __forceinline__ bool is_point(float z) { return z > 0.0f && z <= FLT_MAX; }

__global__ __launch_bounds__(kThreads) void rows_kernel(const float *__restrict__ depth, int M, int H, int W, int thr, int *__restrict__ record,
                                                        const uint8_t *__restrict__ dist, uint8_t *__restrict__ sets) {
  __shared__ int scratch[kThreads];
  const int slot = blockIdx.x, tid = threadIdx.x;
  int *rec = record + (size_t)slot * kRec;
  const int area = rec[rArea];
  if (area < 0) return;
  const int row0 = rec[rRow0], col0 = rec[rCol0], col1 = rec[rCol1], s = rec[rS];
  const int bw = col1 - col0 + 1, npix = area ? bw * (rec[rRow1] - row0 + 1) : 0;
  const float *dp = depth + (size_t)(slot / M) * H * W;
  const uint8_t *g = dist + (size_t)slot * H * W;
  uint8_t *out = sets + (size_t)slot * H * W;
  int n0 = 0, n1 = 0, ns = 0;
  for (int idx = tid; idx < npix; idx += kThreads) {
    const int r = row0 + idx / bw, c = col0 + idx % bw;
    const size_t at = (size_t)r * W + c;
    int D = g[at];
    for (int du = 1; du <= s && du < D; ++du) {
      const int left = c - du, right = c + du;
      if (left >= 0) {                                 // left of the image: set; left of the box: not set
        const int cand = (left >= col0 ? (int)g[at - du] : 0) + du;
        D = cand < D ? cand : D;
      }
      if (right < W) {
        const int cand = (right <= col1 ? (int)g[at + du] : 0) + du;
        D = cand < D ? cand : D;
      }
    }
    int bits = 0;
    if (D > 0 && is_point(dp[at])) {
      bits = 1 | (D >= 2 ? 2 : 0) | (D >= s + 1 ? 4 : 0);
      n0 += 1, n1 += D >= 2, ns += D >= s + 1;
    }
    out[at] = (uint8_t)bits;
  }
  n0 = reduce<0>(n0, scratch), n1 = reduce<0>(n1, scratch), ns = reduce<0>(ns, scratch);
  if (tid == 0) {
    rec[rNs] = ns, rec[rN1] = n1, rec[rN0] = n0;
    rec[rBit] = ns >= thr ? 4 : (n1 >= thr ? 2 : (n0 >= thr ? 1 : 0));
    rec[rShrink] = ns >= thr ? s : (n1 >= thr ? 1 : -1);
  }
}

// ---------------------------------------------------------------------------------------------------------------- the cloud
struct Box {
  const float *depth;                                  // the frame's
  const uint8_t *sets;                                 // the slot's
  int W, row0, col0, bw, npix;
  double fx, fy, cx, cy;
};

// rule 1 at pixel idx of the box, for the points of the set `bit`
__device__ __forceinline__ bool point_at(const Box &b, int idx, int bit, float &x, float &y, float &z) {
  const int r = b.row0 + idx / b.bw, c = b.col0 + idx % b.bw;
  const size_t at = (size_t)r * b.W + c;
  if (!(b.sets[at] & bit)) return false;
  z = b.depth[at];
  x = (float)((((double)c - b.cx) / b.fx) * (double)z);
  y = (float)((((double)r - b.cy) / b.fy) * (double)z);
  return true;
}

__device__ __forceinline__ bool in_circle(float x, float z, double mx, double mz, double d2) {
  const double dx = (double)x - mx, dz = (double)z - mz;
  return dx * dx + dz * dz < d2;
}

__device__ __forceinline__ uint32_t to_key(float v) {
  const uint32_t b = __float_as_uint(v);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ double from_key(uint32_t k) {
  return (double)__uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

struct Select {
  unsigned hist[6][256];                               // selector 2 a + which: axis a, the lower / upper middle rank
  unsigned prefix[6];
  int rank[6];
  int n;
};

// the per-axis median of the points of `bit` (inside the circle about (mx, mz) when Circle) -> their number; med[] when it is > 0
template <bool Circle>
__device__ int median3(const Box &b, int bit, double mx, double mz, double d2, Select &sh, double med[3]) {
  const int tid = threadIdx.x;
  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    __syncthreads();
    for (int i = tid; i < 6 * 256; i += kThreads) (&sh.hist[0][0])[i] = 0;
    __syncthreads();
    for (int idx = tid; idx < b.npix; idx += kThreads) {
      float x, y, z;
      if (!point_at(b, idx, bit, x, y, z)) continue;
      if (Circle && !in_circle(x, z, mx, mz, d2)) continue;
      const uint32_t key[3] = {to_key(x), to_key(y), to_key(z)};
      for (int sel = 0; sel < 6; ++sel) {
        const uint32_t k = key[sel >> 1];
        if (pass == 0 || (k >> (shift + 8)) == sh.prefix[sel]) atomicAdd(&sh.hist[sel][(k >> shift) & 255u], 1u);
      }
    }
    __syncthreads();
    if (pass == 0) {
      if (tid == 0) {
        int n = 0;
        for (int i = 0; i < 256; ++i) n += (int)sh.hist[0][i];
        sh.n = n;
        for (int a = 0; a < 3; ++a) sh.rank[2 * a] = (n - 1) / 2, sh.rank[2 * a + 1] = n / 2, sh.prefix[2 * a] = sh.prefix[2 * a + 1] = 0;
      }
      __syncthreads();
      if (sh.n == 0) return 0;
    }
    if (tid < 6) {
      int acc = 0, bin = 255;
      const int want = sh.rank[tid];
      for (int i = 0; i < 256; ++i) {
        const int h = (int)sh.hist[tid][i];
        if (want < acc + h) {
          bin = i;
          break;
        }
        acc += h;
      }
      sh.rank[tid] = want - acc;
      sh.prefix[tid] = (sh.prefix[tid] << 8) | (unsigned)bin;
    }
  }
  __syncthreads();
  for (int a = 0; a < 3; ++a) med[a] = (from_key(sh.prefix[2 * a]) + from_key(sh.prefix[2 * a + 1])) * 0.5;
  return sh.n;
}

__global__ __launch_bounds__(kThreads) void cloud_kernel(const float *__restrict__ depth, const double *__restrict__ intrinsics,
                                                         const double *__restrict__ poses, int M, int H, int W, int Nmax, int thr, double d2,
                                                         int use_range, double max2, const int *__restrict__ record,
                                                         const uint8_t *__restrict__ sets, float *__restrict__ points, int *__restrict__ counts,
                                                         int *__restrict__ total, double *__restrict__ centres, double *__restrict__ range,
                                                         uint8_t *__restrict__ truncated, int *__restrict__ status, int *__restrict__ shrink) {
  __shared__ Select sh;
  __shared__ int scratch[kThreads];
  __shared__ int wave_count[kWaves];
  const int slot = blockIdx.x, tid = threadIdx.x, f = slot / M;
  const int *rec = record + (size_t)slot * kRec;
  const int area = rec[rArea], bit = area < 0 ? 0 : rec[rBit];
  // the scalars of a slot without a cloud
  auto leave = [&](int st, int shr) {
    if (tid == 0) {
      status[slot] = st, shrink[slot] = shr, truncated[slot] = (uint8_t)(area < 0 ? 0 : rec[rTrunc]);
      counts[slot] = 0, total[slot] = 0, range[slot] = 0.0;
      centres[(size_t)slot * 3] = 0.0, centres[(size_t)slot * 3 + 1] = 0.0, centres[(size_t)slot * 3 + 2] = 0.0;
    }
  };
  if (area < 0) return leave(MONO_LIFT_ABSENT, -1);
  if (bit == 0) return leave(MONO_LIFT_FEW, -1);
  const int used = rec[rShrink];
  Box b;
  b.depth = depth + (size_t)f * H * W, b.sets = sets + (size_t)slot * H * W;
  b.W = W, b.row0 = rec[rRow0], b.col0 = rec[rCol0], b.bw = rec[rCol1] - rec[rCol0] + 1;
  b.npix = b.bw * (rec[rRow1] - rec[rRow0] + 1);
  b.fx = intrinsics[f * 4], b.fy = intrinsics[f * 4 + 1], b.cx = intrinsics[f * 4 + 2], b.cy = intrinsics[f * 4 + 3];
  double T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
  if (poses)
    for (int i = 0; i < 12; ++i) T[i] = poses[(size_t)f * 12 + i];

  double m[3], again[3];
  median3<false>(b, bit, 0.0, 0.0, 0.0, sh, m);        // bit != 0: at least thr >= 1 points
  if (median3<true>(b, bit, m[0], m[2], d2, sh, again) > 0) m[0] = again[0], m[1] = again[1], m[2] = again[2];
  if (use_range && (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2] > max2) return leave(MONO_LIFT_FAR, used);
  double c[3];
  for (int a = 0; a < 3; ++a) c[a] = ((T[4 * a] * m[0] + T[4 * a + 1] * m[1]) + T[4 * a + 2] * m[2]) + T[4 * a + 3];
  if (!(c[2] > 0.0)) return leave(MONO_LIFT_BEHIND, used);

  double m2[3];
  median3<false>(b, 1, 0.0, 0.0, 0.0, sh, m2);
  int survivors = 0;
  for (int idx = tid; idx < b.npix; idx += kThreads) {
    float x, y, z;
    survivors += point_at(b, idx, 1, x, y, z) && in_circle(x, z, m2[0], m2[2], d2);
  }
  survivors = reduce<0>(survivors, scratch);
  if (survivors < thr) return leave(MONO_LIFT_FEW, used);

  float *out = points + (size_t)slot * Nmax * 3;
  const int lane = tid & (kWave - 1), wave = tid / kWave;
  int written = 0;                                     // survivors before this chunk
  for (int base = 0; base < b.npix && written < Nmax; base += kThreads) {
    const int idx = base + tid;
    float x = 0, y = 0, z = 0;
    const bool keep = idx < b.npix && point_at(b, idx, 1, x, y, z) && in_circle(x, z, m2[0], m2[2], d2);
    const unsigned long long votes = __ballot(keep);
    if (lane == 0) wave_count[wave] = __popcll(votes);
    __syncthreads();
    int pos = written + __popcll(votes & ((1ull << lane) - 1ull)), chunk = 0;
    for (int w = 0; w < kWaves; ++w) {
      pos += w < wave ? wave_count[w] : 0;
      chunk += wave_count[w];
    }
    if (keep && pos < Nmax) {
      const double X = x, Y = y, Z = z;
      for (int a = 0; a < 3; ++a) out[(size_t)pos * 3 + a] = (float)(((T[4 * a] * X + T[4 * a + 1] * Y) + T[4 * a + 2] * Z) + T[4 * a + 3]);
    }
    written += chunk;
    __syncthreads();
  }
  if (tid == 0) {
    status[slot] = MONO_LIFT_OK | (survivors > Nmax ? MONO_LIFT_CLIPPED : 0);
    shrink[slot] = used, truncated[slot] = (uint8_t)rec[rTrunc];
    counts[slot] = survivors < Nmax ? survivors : Nmax, total[slot] = survivors;
    range[slot] = __dsqrt_rn(m[0] * m[0] + m[2] * m[2]);
    for (int a = 0; a < 3; ++a) centres[(size_t)slot * 3 + a] = c[a];
  }
}

// ---------------------------------------------------------------------------------------------------------------- gather
__global__ __launch_bounds__(kThreads) void gather_kernel(const float *__restrict__ points, const int *__restrict__ counts,
                                                          const int *__restrict__ status, const double *__restrict__ range,
                                                          const uint8_t *__restrict__ truncated, const double *__restrict__ centres, int F,
                                                          int M, int Nmax, const int *__restrict__ tracks, const uint8_t *__restrict__ moving,
                                                          int V, int ref_frame, int max_views, int K, float *__restrict__ out_points,
                                                          int *__restrict__ out_counts, double *__restrict__ out_centres) {
  __shared__ double key[kThreads];
  __shared__ double cs[3][kThreads], sorted[3][kThreads];
  __shared__ int valid[kThreads], kept_slot[kThreads], offs[kThreads + 1];
  __shared__ int nkept, any_nan[3];
  const int b = blockIdx.x, v = threadIdx.x;
  const bool mov = moving && moving[b];
  int slot = -1;
  double k = 0.0;
  if (v < V) {
    const int f = tracks[((size_t)b * V + v) * 2], m = tracks[((size_t)b * V + v) * 2 + 1];
    if (f >= 0 && f < F && m >= 0 && m < M && (status[f * M + m] & 7) == MONO_LIFT_OK && (!mov || f == ref_frame)) {
      slot = f * M + m;
      k = mov ? (double)v : range[slot] + (truncated[slot] ? 5.0 : 0.0);
    }
  }
  key[v] = k, valid[v] = slot >= 0, kept_slot[v] = -1;
  if (v < 3) any_nan[v] = 0;
  __syncthreads();
  const int limit = mov ? 1 : max_views;
  if (slot >= 0) {
    int rank = 0;
    for (int w = 0; w < V; ++w) rank += valid[w] && (key[w] < k || (key[w] == k && w < v));
    if (rank < limit) kept_slot[rank] = slot;
  }
  __syncthreads();
  if (v == 0) {
    int n = 0;
    offs[0] = 0;
    while (n < V && n < limit && kept_slot[n] >= 0) {
      offs[n + 1] = offs[n] + clampi(counts[kept_slot[n]], 0, Nmax);
      ++n;
    }
    nkept = n;
  }
  __syncthreads();
  const int nk = nkept;
  if (v < nk)
    for (int a = 0; a < 3; ++a) {
      const double c = centres[(size_t)kept_slot[v] * 3 + a];
      if (c != c) any_nan[a] = 1;                      // every writer stores the same 1
      cs[a][v] = c != c ? INFINITY : c;
    }
  __syncthreads();
  if (v < nk)
    for (int a = 0; a < 3; ++a) {
      const double c = cs[a][v];
      int rank = 0;
      for (int w = 0; w < nk; ++w) rank += cs[a][w] < c || (cs[a][w] == c && w < v);
      sorted[a][rank] = c;
    }
  __syncthreads();
  if (v < 3) {
    double med = 0.0;
    if (nk > 0) med = any_nan[v] ? (double)NAN : (sorted[v][(nk - 1) / 2] + sorted[v][nk / 2]) * 0.5;
    out_centres[(size_t)b * 3 + v] = med;
  }
  const int n = offs[nk];
  if (v == 0) out_counts[b] = n < K ? n : K;
  float *out = out_points + (size_t)b * K * 3;
  for (int j = v; j < n; j += kThreads) {
    long long pos = j;
    if (n > K) {
      pos = ((long long)j * K) / n;
      if (!(((long long)(j + 1) * K) / n > pos)) continue;
    }
    int lo = 0, hi = nk - 1;                           // the view with offs[lo] <= j < offs[lo + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) / 2;
      if (offs[mid] <= j) lo = mid; else hi = mid - 1;
    }
    const float *src = points + ((size_t)kept_slot[lo] * Nmax + (j - offs[lo])) * 3;
    out[pos * 3] = src[0], out[pos * 3 + 1] = src[1], out[pos * 3 + 2] = src[2];
  }
}

}  // namespace lift

extern "C" {

int mono_lift_abi_version(void) { return MONO_LIFT_ABI_VERSION; }

int mono_lift_objects_f32(const float *depth, const double *intrinsics, const uint8_t *masks, const int32_t *mask_count,
                          const double *poses, int F, int M, int H, int W, int Nmax, int thr, double d, int use_range, double max,
                          int stages, uint8_t *dist, uint8_t *sets, int32_t *record, float *points, int32_t *counts, int32_t *total,
                          double *centres, double *range, uint8_t *truncated, int32_t *status, int32_t *shrink, void *stream) {
  if (!depth || !intrinsics || !masks || !mask_count || !dist || !sets || !record || !points || !counts || !total || !centres ||
      !range || !truncated || !status || !shrink)
    return MONO_LIFT_NULL;
  if (F < 0 || M < 0 || H < 1 || W < 1 || Nmax < 1 || thr < 1 || !(d >= 0.0 && d <= DBL_MAX) || !(max >= 0.0 && max <= DBL_MAX) ||
      stages < 1 || stages > MONO_LIFT_ALL)
    return MONO_LIFT_BAD_SIZE;
  if (F > MONO_LIFT_MAX_F || M > MONO_LIFT_MAX_M || H > MONO_LIFT_MAX_SIDE || W > MONO_LIFT_MAX_SIDE ||
      (long long)H * W > MONO_LIFT_MAX_PIXELS || Nmax > MONO_LIFT_MAX_POINTS)
    return MONO_LIFT_TOO_LARGE;
  if (F == 0 || M == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(F * M), block(lift::kThreads);
  if (stages & MONO_LIFT_STAGE_BOX) lift::box_kernel<<<grid, block, 0, s>>>(masks, mask_count, M, H, W, record);
  if (stages & MONO_LIFT_STAGE_COLUMNS) lift::columns_kernel<<<grid, block, 0, s>>>(masks, H, W, record, dist);
  if (stages & MONO_LIFT_STAGE_ROWS) lift::rows_kernel<<<grid, block, 0, s>>>(depth, M, H, W, thr, record, dist, sets);
  if (stages & MONO_LIFT_STAGE_CLOUD)
    lift::cloud_kernel<<<grid, block, 0, s>>>(depth, intrinsics, poses, M, H, W, Nmax, thr, d * d, use_range, max * max, record, sets,
                                              points, counts, total, centres, range, truncated, status, shrink);
  return (int)hipGetLastError();
}

int mono_lift_gather_f32(const float *points, const int32_t *counts, const int32_t *status, const double *range,
                         const uint8_t *truncated, const double *centres, int F, int M, int Nmax, const int32_t *tracks,
                         const uint8_t *moving, int B, int V, int ref_frame, int max_views, int K, float *out_points,
                         int32_t *out_counts, double *out_centres, void *stream) {
  if (!points || !counts || !status || !range || !truncated || !centres || !tracks || !out_points || !out_counts || !out_centres)
    return MONO_LIFT_NULL;
  if (F < 1 || M < 1 || Nmax < 1 || B < 0 || V < 1 || max_views < 1 || K < 1) return MONO_LIFT_BAD_SIZE;
  if (F > MONO_LIFT_MAX_F || M > MONO_LIFT_MAX_M || Nmax > MONO_LIFT_MAX_POINTS || B > MONO_LIFT_MAX_TRACKS || V > MONO_LIFT_MAX_VIEWS ||
      K > MONO_LIFT_MAX_POINTS)
    return MONO_LIFT_TOO_LARGE;
  if (B == 0) return 0;
  lift::gather_kernel<<<dim3(B), dim3(lift::kThreads), 0, (hipStream_t)stream>>>(points, counts, status, range, truncated, centres, F, M,
                                                                                Nmax, tracks, moving, V, ref_frame, max_views, K,
                                                                                out_points, out_counts, out_centres);
  return (int)hipGetLastError();
}
}
