// Template-pose search for gfx950 (include/monosowa_fit.h states the rule): a car template fitted to each object's point cloud by
// exhaustive search over a grid of placements, two integer counts per placement, exact and bit-reproducible.
//
//   mono_fit_grid_f32     three launches: bounds and cell ids (one workgroup per object), ranking by counting (the points ordered
//                         by cell, then index: a counting sort without a counter), cell starts by binary search
//   mono_fit_search_f32   one wavefront per placement, four consecutive placements (consecutive k: the same i, j) per workgroup; the
//                         template and its grid in LDS (sized by the launch), the scan's grid in global memory; lanes stride over points, look at the 27
//                         cells around each, leave at the first hit; counts by ballot and population count
//   mono_fit_reduce_f64   one workgroup per object: the losses in double, the minimum under the total order (L, h)
//
// No atomics.  A kernel boundary is the only hand-off between workgroups.
#include <float.h>
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "../../include/monosowa_fit.h"

// the rule rounds every float32 product and sum on its own
#pragma clang fp contract(off)

namespace fit {

constexpr int kThreads = 256;
constexpr int kWave = 64;
constexpr int kWaves = kThreads / kWave;
constexpr float kSlack = 1.01f;                      // cell width over r: covers the float32 rounding of the test and of the cell index

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= FLT_MAX; }

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// cell of an indexed point along one axis (the point is finite, v >= origin)
__device__ __forceinline__ int axis_cell(float v, float origin, float inv, int dim) {
  if (inv < 0.0f) return 0;
  const float u = (v - origin) * inv;
  if (!(u < (float)dim)) return dim - 1;             // the largest point: rounding may put it on the far edge
  return clampi((int)u, 0, dim - 1);
}

// the cells in which a query at v can have a neighbour: [lo, hi] inside the grid; false when v is not finite or lies more than a
// cell outside the bounds -- never a clamped cell
__device__ __forceinline__ bool axis_range(float v, float origin, float inv, int dim, int &lo, int &hi) {
  if (!finite(v)) return false;
  if (inv < 0.0f) {
    lo = hi = 0;
    return true;
  }
  const float u = (v - origin) * inv;
  if (!(u >= -1.0f && u < (float)(dim + 1))) return false;
  const int c = (int)floorf(u);                      // -1 .. dim
  lo = c - 1 < 0 ? 0 : c - 1;
  hi = c + 1 > dim - 1 ? dim - 1 : c + 1;
  return lo <= hi;
}

// the grid over `ext` = max - min along one axis: cells of hmin, or wider ones when kMaxDim of those do not reach
__device__ __forceinline__ void axis_grid(float lo, float hi, float hmin, float &inv, int &dim) {
  const float ext = hi - lo;
  if (!finite(ext)) {                                // overflow: one cell, no culling along this axis
    inv = -1.0f;
    dim = 1;
    return;
  }
  const float q = ext / hmin;
  float h = hmin;
  if (q >= (float)(MONO_FIT_MAX_DIM - 1)) {
    dim = MONO_FIT_MAX_DIM;
    h = fmaxf(hmin, ext / (float)MONO_FIT_MAX_DIM);
  } else {
    dim = (int)q + 1;
  }
  inv = 1.0f / h;
}

// ---------------------------------------------------------------------------------------------------------------- the scan's grid
__global__ __launch_bounds__(kThreads) void grid_cells_kernel(const float *__restrict__ scan, const int *__restrict__ count, int Nmax,
                                                              float hmin, mono_fit_grid_t *__restrict__ grid, int *__restrict__ cell) {
  __shared__ float red[6][kThreads];
  __shared__ mono_fit_grid_t g;
  const int o = blockIdx.x, tid = threadIdx.x;
  const int n = clampi(count[o], 0, Nmax);
  const float *pts = scan + (size_t)o * Nmax * 3;
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int p = tid; p < n; p += kThreads) {
    const float x = pts[p * 3], y = pts[p * 3 + 1], z = pts[p * 3 + 2];
    if (finite(x) && finite(y) && finite(z)) {
      lo[0] = fminf(lo[0], x), lo[1] = fminf(lo[1], y), lo[2] = fminf(lo[2], z);
      hi[0] = fmaxf(hi[0], x), hi[1] = fmaxf(hi[1], y), hi[2] = fmaxf(hi[2], z);
    }
  }
  for (int a = 0; a < 3; ++a) red[a][tid] = lo[a], red[3 + a][tid] = hi[a];
  __syncthreads();
  for (int step = kThreads / 2; step > 0; step >>= 1) {
    if (tid < step)
      for (int a = 0; a < 3; ++a) {
        red[a][tid] = fminf(red[a][tid], red[a][tid + step]);
        red[3 + a][tid] = fmaxf(red[3 + a][tid], red[3 + a][tid + step]);
      }
    __syncthreads();
  }
  if (tid == 0) {
    int cells = 1;
    for (int a = 0; a < 3; ++a) {
      float l = red[a][0], h = red[3 + a][0];
      if (l > h) l = h = 0.0f;                       // no finite point
      g.origin[a] = l;
      float inv;
      int dim;
      axis_grid(l, h, hmin, inv, dim);
      g.inv[a] = inv;
      g.dim[a] = dim;
      cells *= dim;
    }
    g.ncell = cells;
    grid[o] = g;
  }
  __syncthreads();
  int *out = cell + (size_t)o * Nmax;
  for (int p = tid; p < n; p += kThreads) {
    const float x = pts[p * 3], y = pts[p * 3 + 1], z = pts[p * 3 + 2];
    int id = g.ncell;
    if (finite(x) && finite(y) && finite(z)) {
      const int cx = axis_cell(x, g.origin[0], g.inv[0], g.dim[0]);
      const int cy = axis_cell(y, g.origin[1], g.inv[1], g.dim[1]);
      const int cz = axis_cell(z, g.origin[2], g.inv[2], g.dim[2]);
      id = (cz * g.dim[1] + cy) * g.dim[0] + cx;
    }
    out[p] = id;
  }
}

// rank of point p = the number of points before it in the order (cell id, index): every rank in [0, n) is taken exactly once
__global__ __launch_bounds__(kThreads) void grid_rank_kernel(const float *__restrict__ scan, const int *__restrict__ count, int Nmax,
                                                             const int *__restrict__ cell, float4 *__restrict__ sorted,
                                                             int *__restrict__ scell) {
  __shared__ int tile[kThreads];
  const int o = blockIdx.y, tid = threadIdx.x;
  const int n = clampi(count[o], 0, Nmax);
  if ((int)blockIdx.x * kThreads >= n) return;       // the whole workgroup
  const int *ids = cell + (size_t)o * Nmax;
  const int p = blockIdx.x * kThreads + tid;
  const int mine = p < n ? ids[p] : INT_MAX;
  int rank = 0;
  for (int q0 = 0; q0 < n; q0 += kThreads) {
    tile[tid] = q0 + tid < n ? ids[q0 + tid] : INT_MAX;
    __syncthreads();
    const int before = p - q0;                       // tile entries j < before lie before p
    for (int j = 0; j < kThreads; ++j) {
      const int c = tile[j];
      rank += (c < mine || (c == mine && j < before)) ? 1 : 0;
    }
    __syncthreads();
  }
  if (p < n) {
    const float *pt = scan + ((size_t)o * Nmax + p) * 3;
    sorted[(size_t)o * Nmax + rank] = make_float4(pt[0], pt[1], pt[2], 0.0f);
    scell[(size_t)o * Nmax + rank] = mine;
  }
}

// start[c] = the number of points with a cell id below c, for c = 0 .. ncell
__global__ __launch_bounds__(kThreads) void grid_starts_kernel(const int *__restrict__ count, int Nmax, const mono_fit_grid_t *__restrict__ grid,
                                                               const int *__restrict__ scell, int *__restrict__ start) {
  const int o = blockIdx.y;
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c > grid[o].ncell) return;
  const int n = clampi(count[o], 0, Nmax);
  const int *ids = scell + (size_t)o * Nmax;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  start[(size_t)o * (MONO_FIT_MAX_CELLS + 1) + c] = lo;
}

// ---------------------------------------------------------------------------------------------------------------- the search
__global__ __launch_bounds__(kThreads) void search_kernel(const float *__restrict__ tmpl, const int *__restrict__ tstart, mono_fit_grid_t tg,
                                                          int T, const mono_fit_grid_t *__restrict__ grid, const float4 *__restrict__ sorted,
                                                          const int *__restrict__ start, const int *__restrict__ count, int Nmax,
                                                          const float *__restrict__ txl, const float *__restrict__ tyl,
                                                          const float *__restrict__ tzl, const float *__restrict__ cs, int I, int J, int K,
                                                          const int *__restrict__ fix, int H, float r2, int *__restrict__ ab) {
  extern __shared__ float lds[];                      // the template's points, then its cell starts: (3 T + ncell + 1) words
  float *tp = lds;
  int *ts = reinterpret_cast<int *>(lds + T * 3);
  const int o = blockIdx.y, tid = threadIdx.x;
  for (int e = tid; e < T * 3; e += kThreads) tp[e] = tmpl[e];
  for (int e = tid; e <= tg.ncell; e += kThreads) ts[e] = tstart[e];
  __syncthreads();
  const int lane = tid & (kWave - 1);
  const int h = blockIdx.x * kWaves + (tid >> 6);
  if (h >= H) return;                                // the whole wavefront
  int i, j, k;
  if (fix) {
    i = clampi(fix[o * MONO_FIT_RESULT_INTS + 4], 0, I - 1);
    j = clampi(fix[o * MONO_FIT_RESULT_INTS + 5], 0, J - 1);
    k = h;
  } else {
    k = h % K;
    j = (h / K) % J;
    i = h / (K * J);
  }
  const float tx = txl[(size_t)o * I + i], ty = tyl[o], tz = tzl[(size_t)o * J + j];
  const float c = cs[((size_t)o * K + k) * 2], s = cs[((size_t)o * K + k) * 2 + 1];
  const int n = clampi(count[o], 0, Nmax);
  const mono_fit_grid_t sg = grid[o];
  const float4 *pts = sorted + (size_t)o * Nmax;
  const int *st = start + (size_t)o * (MONO_FIT_MAX_CELLS + 1);

  // a: template points with a scan point within r
  int a = 0;
  for (int t0 = 0; t0 < T; t0 += kWave) {
    const int t = t0 + lane;
    bool hit = false;
    if (t < T) {
      const float x = tp[t * 3], y = tp[t * 3 + 1], z = tp[t * 3 + 2];
      const float wx = (c * x + s * z) + tx;
      const float wy = y + ty;
      const float wz = (c * z - s * x) + tz;
      int x0, x1, y0, y1, z0, z1;
      if (axis_range(wx, sg.origin[0], sg.inv[0], sg.dim[0], x0, x1) && axis_range(wy, sg.origin[1], sg.inv[1], sg.dim[1], y0, y1) &&
          axis_range(wz, sg.origin[2], sg.inv[2], sg.dim[2], z0, z1)) {
        for (int cz = z0; cz <= z1 && !hit; ++cz)
          for (int cy = y0; cy <= y1 && !hit; ++cy) {
            const int row = (cz * sg.dim[1] + cy) * sg.dim[0];
            const int q1 = st[row + x1 + 1];
            for (int q = st[row + x0]; q < q1; ++q) {
              const float4 p = pts[q];
              const float ex = p.x - wx, ey = p.y - wy, ez = p.z - wz;
              const float d = (ex * ex + ey * ey) + ez * ez;
              if (d < r2) {
                hit = true;
                break;
              }
            }
          }
      }
    }
    a += __popcll(__ballot(hit));
  }

  // b: scan points with a template point within r, in the template's frame
  int b = 0;
  for (int p0 = 0; p0 < n; p0 += kWave) {
    const int q = p0 + lane;
    bool hit = false;
    if (q < n) {
      const float4 p = pts[q];
      const float px = p.x - tx, py = p.y - ty, pz = p.z - tz;
      const float lx = c * px - s * pz;
      const float ly = py;
      const float lz = s * px + c * pz;
      int x0, x1, y0, y1, z0, z1;
      if (axis_range(lx, tg.origin[0], tg.inv[0], tg.dim[0], x0, x1) && axis_range(ly, tg.origin[1], tg.inv[1], tg.dim[1], y0, y1) &&
          axis_range(lz, tg.origin[2], tg.inv[2], tg.dim[2], z0, z1)) {
        for (int cz = z0; cz <= z1 && !hit; ++cz)
          for (int cy = y0; cy <= y1 && !hit; ++cy) {
            const int row = (cz * tg.dim[1] + cy) * tg.dim[0];
            const int t1 = ts[row + x1 + 1];
            for (int t = ts[row + x0]; t < t1; ++t) {
              const float ex = lx - tp[t * 3], ey = ly - tp[t * 3 + 1], ez = lz - tp[t * 3 + 2];
              const float d = (ex * ex + ey * ey) + ez * ez;
              if (d < r2) {
                hit = true;
                break;
              }
            }
          }
      }
    }
    b += __popcll(__ballot(hit));
  }
  if (lane == 0) {
    int *out = ab + ((size_t)o * H + h) * 2;
    out[0] = a;
    out[1] = b;
  }
}

// ---------------------------------------------------------------------------------------------------------------- the minimum
__device__ __forceinline__ bool before(double l1, int h1, double l2, int h2) { return l1 < l2 || (l1 == l2 && h1 < h2); }

__global__ __launch_bounds__(kThreads) void reduce_kernel(const int *__restrict__ ab, const int *__restrict__ count, int Nmax, int T, int I,
                                                          int J, int K, const int *__restrict__ fix, int H, int one_way,
                                                          int *__restrict__ result, double *__restrict__ loss) {
  __shared__ double ls[kThreads];
  __shared__ int hs[kThreads];
  const int o = blockIdx.x, tid = threadIdx.x;
  const int n = clampi(count[o], 0, Nmax);
  int *res = result + o * MONO_FIT_RESULT_INTS;
  if (n == 0 || T == 0) {                            // the whole workgroup
    if (tid == 0) {
      res[0] = 0, res[1] = 0, res[2] = 0, res[3] = MONO_FIT_EMPTY;
      res[4] = fix ? fix[o * MONO_FIT_RESULT_INTS + 4] : 0;
      res[5] = fix ? fix[o * MONO_FIT_RESULT_INTS + 5] : 0;
      loss[o] = 0.0;
    }
    return;
  }
  const int *mine = ab + (size_t)o * H * 2;
  double best = INFINITY;
  int at = INT_MAX;
  for (int h = tid; h < H; h += kThreads) {
    const double la = (double)mine[h * 2] / (double)T;
    const double l = one_way ? -la : -(la + (double)mine[h * 2 + 1] / (double)n);
    if (before(l, h, best, at)) best = l, at = h;
  }
  ls[tid] = best, hs[tid] = at;
  __syncthreads();
  for (int step = kThreads / 2; step > 0; step >>= 1) {
    if (tid < step && before(ls[tid + step], hs[tid + step], ls[tid], hs[tid])) ls[tid] = ls[tid + step], hs[tid] = hs[tid + step];
    __syncthreads();
  }
  if (tid == 0) {
    const int h = hs[0];
    res[0] = h, res[1] = mine[h * 2], res[2] = mine[h * 2 + 1], res[3] = MONO_FIT_OK;
    res[4] = fix ? fix[o * MONO_FIT_RESULT_INTS + 4] : h / (K * J);
    res[5] = fix ? fix[o * MONO_FIT_RESULT_INTS + 5] : (h / K) % J;
    loss[o] = ls[0];
  }
}

static bool good_r(float r) { return r > 0.0f && r <= FLT_MAX && r * r > 0.0f && r * r * kSlack <= FLT_MAX; }

// I, J, K >= 1 -> their product when it is within the limit, else 0
static long long placements(int I, int J, int K) {
  const long long h = (long long)I * J * K;
  return (I > MONO_FIT_MAX_H || J > MONO_FIT_MAX_H || K > MONO_FIT_MAX_H || h > MONO_FIT_MAX_H) ? 0 : h;
}

}  // namespace fit

extern "C" {

int mono_fit_abi_version(void) { return MONO_FIT_ABI_VERSION; }

int mono_fit_grid_f32(const float *scan, const int32_t *count, int B, int Nmax, float r, mono_fit_grid_t *grid, float *sorted,
                      int32_t *start, int32_t *cell, int32_t *scell, void *stream_) {
  if (!scan || !count || !grid || !sorted || !start || !cell || !scell) return MONO_FIT_NULL;
  if (B < 0 || Nmax < 1 || !fit::good_r(r) || ((uintptr_t)sorted & 15)) return MONO_FIT_BAD_SIZE;
  if (B > MONO_FIT_MAX_B || Nmax > MONO_FIT_MAX_N) return MONO_FIT_TOO_LARGE;
  if (B == 0) return 0;
  hipStream_t stream = (hipStream_t)stream_;
  fit::grid_cells_kernel<<<B, fit::kThreads, 0, stream>>>(scan, count, Nmax, r * fit::kSlack, grid, cell);
  fit::grid_rank_kernel<<<dim3((Nmax + fit::kThreads - 1) / fit::kThreads, B), fit::kThreads, 0, stream>>>(scan, count, Nmax, cell,
                                                                                                        (float4 *)sorted, scell);
  fit::grid_starts_kernel<<<dim3((MONO_FIT_MAX_CELLS + 1 + fit::kThreads - 1) / fit::kThreads, B), fit::kThreads, 0, stream>>>(
      count, Nmax, grid, scell, start);
  return (int)hipGetLastError();
}

int mono_fit_search_f32(const float *tmpl, const int32_t *tstart, const mono_fit_grid_t *tgrid, int T, const mono_fit_grid_t *grid,
                        const float *sorted, const int32_t *start, const int32_t *count, int B, int Nmax, const float *tx,
                        const float *ty, const float *tz, const float *cs, int I, int J, int K, const int32_t *fix, float r,
                        int32_t *ab, void *stream_) {
  if (!tmpl || !tstart || !tgrid || !grid || !sorted || !start || !count || !tx || !ty || !tz || !cs || !ab) return MONO_FIT_NULL;
  if (B < 0 || Nmax < 1 || T < 0 || I < 1 || J < 1 || K < 1 || !fit::good_r(r) || ((uintptr_t)sorted & 15)) return MONO_FIT_BAD_SIZE;
  long long cells = 1;
  for (int a = 0; a < 3; ++a) {
    if (tgrid->dim[a] < 1 || tgrid->dim[a] > MONO_FIT_MAX_DIM) return MONO_FIT_BAD_SIZE;
    cells *= tgrid->dim[a];
  }
  if (tgrid->ncell != cells) return MONO_FIT_BAD_SIZE;
  const long long H = fix ? (K <= MONO_FIT_MAX_H ? K : 0) : fit::placements(I, J, K);
  if (B > MONO_FIT_MAX_B || Nmax > MONO_FIT_MAX_N || T > MONO_FIT_MAX_T || cells > MONO_FIT_MAX_TCELLS || H == 0 ||
      I > MONO_FIT_MAX_H || J > MONO_FIT_MAX_H)
    return MONO_FIT_TOO_LARGE;
  if (B == 0) return 0;
  const size_t lds = ((size_t)T * 3 + (size_t)cells + 1) * sizeof(float);      // at most 40,964 bytes
  fit::search_kernel<<<dim3(((int)H + fit::kWaves - 1) / fit::kWaves, B), fit::kThreads, lds, (hipStream_t)stream_>>>(
      tmpl, tstart, *tgrid, T, grid, (const float4 *)sorted, start, count, Nmax, tx, ty, tz, cs, I, J, K, fix, (int)H, r * r, ab);
  return (int)hipGetLastError();
}

int mono_fit_reduce_f64(const int32_t *ab, const int32_t *count, int B, int Nmax, int T, int I, int J, int K, const int32_t *fix,
                        int one_way, int32_t *result, double *loss, void *stream_) {
  if (!ab || !count || !result || !loss) return MONO_FIT_NULL;
  if (B < 0 || Nmax < 1 || T < 0 || I < 1 || J < 1 || K < 1) return MONO_FIT_BAD_SIZE;
  const long long H = fix ? (K <= MONO_FIT_MAX_H ? K : 0) : fit::placements(I, J, K);
  if (B > MONO_FIT_MAX_B || Nmax > MONO_FIT_MAX_N || T > MONO_FIT_MAX_T || H == 0) return MONO_FIT_TOO_LARGE;
  if (B == 0) return 0;
  fit::reduce_kernel<<<B, fit::kThreads, 0, (hipStream_t)stream_>>>(ab, count, Nmax, T, I, J, K, fix, (int)H, one_way != 0, result,
                                                                  loss);
  return (int)hipGetLastError();
}

}  // extern "C"
