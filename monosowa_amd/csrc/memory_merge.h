// ---- The self-training label memory: a pass's rows merged into a frame's remembered rows (included by rotate_iou.hip) ----
// rows f64 [B, R, 14] + count [B] + frame [B] + bank f64 [N, M, 16] + bank_count [N] -> the frame's bank block and bank_count in
// place, out_rows f64 [B, M, 14], out_count [B], stats int32 [B, 6].  include/monosowa_kitti.h states the rule; this is its layout.
// One workgroup per image, which owns the block of the frame it names (the caller names distinct frames):
//   1. the image's n rows (at most 256 x 14 doubles) and the frame's k entries (at most 64 x 16 doubles) go to LDS, their BEV
//      rectangles (x, z, l, w, ry) beside them in float32;
//   2. flags: a wavefront per row, a lane per entry -- there are at most 64 entries, so ONE ballot is the row's whole flag word
//      (equal class and fuse_dets.h's overlap test: the shortcut for five equal finite numbers, kitti::intersection_area and
//      kitti::ratio with criterion -1 otherwise, compared in float32).  One lane writes the word; no atomics.  A row whose score is
//      not finite gets the word 0;
//   3. the greedy walk on wavefront 0: lane l holds the flag words of rows 64 c + l in registers, the trip for row i reads its
//      word with a lane read (the index is wave-uniform), `word & ~claimed` and the lowest set bit.  The claimed mask is one
//      wave-uniform 64-bit value.  At most 256 trips without a memory access; lane l keeps row 64 c + l's entry, lane e keeps
//      entry e's row, and both are written once behind the loop;
//   4. a thread per candidate (k entries, then the n rows: at most 320 of 512 threads): the smoothed score -- three roundings,
//      contraction off -- and the drop test;
//   5. rank by counting among the survivors (score descending, ties by candidate index: entries before rows, each in their own
//      order), as fuse_dets.h step 2; wavefront 0 counts the tallies with ballots meanwhile;
//   6. a thread per double of the M x 16 block: the survivor of that rank or zero, to the bank and (columns 0..13) to out_rows.
// A frame outside [0, N) reads and writes no bank: zero rows, count and stats.
namespace memory {

constexpr int kThreads = 512;
constexpr int kMaxRows = 256;            // R the kernel accepts
constexpr int kMaxSlots = 64;            // M the kernel accepts: one lane per entry
constexpr int kMaxCand = kMaxSlots + kMaxRows;
constexpr int kRow = 14;
constexpr int kEntry = 16;
constexpr int kStats = 6;                // matched, created, missed, dropped, evicted, skipped

__device__ __forceinline__ bool finite(double v) { return fabs(v) < (double)INFINITY; }      // false for a NaN

__global__ __launch_bounds__(kThreads) void memory_merge_kernel(const double *__restrict__ rows, const int *__restrict__ count,
                                                               const int *__restrict__ frame, double *__restrict__ bank,
                                                               int *__restrict__ bank_count, double w, float threshold,
                                                               double drop_below, double *__restrict__ out_rows,
                                                               int *__restrict__ out_count, int *__restrict__ stats, int R, int N,
                                                               int M) {
#pragma clang fp contract(off)
  __shared__ double row[kMaxRows * kRow];
  __shared__ double ent[kMaxSlots * kEntry];
  __shared__ double score[kMaxCand];                         // by candidate: entry e at e, row i at k + i
  __shared__ unsigned long long flag[kMaxRows];              // bit e of flag[i]: row i may claim entry e
  __shared__ float rbox[kMaxRows * 5], ebox[kMaxSlots * 5];
  __shared__ short match_of[kMaxRows];                       // the entry row i claimed, -1 unmatched, -2 not eligible
  __shared__ short claimer[kMaxSlots];                       // the row that claimed entry e, -1 none
  __shared__ short dest[kMaxSlots];                          // by rank: the candidate
  __shared__ unsigned char state[kMaxCand];                  // 0 no candidate, 1 survivor, 2 dropped
  __shared__ int tally[kStats];
  __shared__ int n_out;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  const int f = frame[b];
  double *orow = out_rows + (long long)b * M * kRow;
  if (f < 0 || f >= N) {                                     // workgroup-uniform: no barrier is skipped by part of a workgroup
    for (int e = tid; e < M * kRow; e += kThreads) orow[e] = 0.0;
    if (tid < kStats) stats[b * kStats + tid] = 0;
    if (tid == 0) out_count[b] = 0;
    return;
  }
  double *block = bank + (long long)f * M * kEntry;
  const int cb = count[b], ck = bank_count[f];
  const int n = cb < 0 ? 0 : (cb > R ? R : cb), k = ck < 0 ? 0 : (ck > M ? M : ck);

  // 1. rows, entries, rectangles
  for (int e = tid; e < n * kRow; e += kThreads) row[e] = rows[(long long)b * R * kRow + e];
  for (int e = tid; e < k * kEntry; e += kThreads) ent[e] = block[e];
  __syncthreads();
  for (int i = tid; i < n + k; i += kThreads) {
    const double *m = i < n ? row + i * kRow : ent + (i - n) * kEntry;
    float *q = i < n ? rbox + i * 5 : ebox + (i - n) * 5;
    q[0] = (float)m[9];
    q[1] = (float)m[11];
    q[2] = (float)m[8];
    q[3] = (float)m[7];
    q[4] = (float)m[12];
  }
  __syncthreads();

  // 2. flags: a wavefront per row, a lane per entry
  for (int i = tid >> 6; i < n; i += kThreads / 64) {
    bool hit = false;
    if (lane < k && finite(row[i * kRow + 13]) && row[i * kRow] == ent[lane * kEntry]) {
      const float *bi = rbox + i * 5, *bj = ebox + lane * 5;
      if (bi[2] > 0.f && bi[3] > 0.f && bj[2] > 0.f && bj[3] > 0.f) {      // a rectangle without an area matches nothing
        bool same = true;                                    // five equal finite numbers: IoU 1 (fuse_dets.h)
#pragma unroll
        for (int c = 0; c < 5; ++c) same = same && bi[c] == bj[c] && fabsf(bi[c]) < INFINITY;
        hit = same || kitti::ratio(kitti::intersection_area(bi, bj), bi[2] * bi[3], bj[2] * bj[3], -1) >= threshold;
      }
    }
    const unsigned long long word = __ballot(hit);
    if (lane == 0) flag[i] = word;
  }
  __syncthreads();

  // 3. the greedy walk, wavefront 0
  if (tid < 64) {
    constexpr int kBlocks = kMaxRows / 64;
    int lo[kBlocks], hi[kBlocks], mine[kBlocks];
    unsigned long long eligible[kBlocks];
    int n_eligible = 0;
#pragma unroll
    for (int c = 0; c < kBlocks; ++c) {
      const int i = c * 64 + lane;
      const unsigned long long word = i < n ? flag[i] : 0ull;
      lo[c] = (int)(unsigned)word;
      hi[c] = (int)(unsigned)(word >> 32);
      eligible[c] = __ballot(i < n && finite(row[(i < n ? i : 0) * kRow + 13]));
      n_eligible += __popcll(eligible[c]);
      mine[c] = -2;
    }
    unsigned long long claimed = 0ull;
    int my_row = -1;
#pragma unroll
    for (int c = 0; c < kBlocks; ++c) {
      for (int l = 0; l < 64 && c * 64 + l < n; ++l) {
        if (!((eligible[c] >> l) & 1ull)) continue;          // wave-uniform
        const unsigned long long word = ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(hi[c], l) << 32) |
                                        (unsigned long long)(unsigned)__builtin_amdgcn_readlane(lo[c], l);
        const unsigned long long open = word & ~claimed;
        int e = -1;
        if (open) {
          e = __ffsll((long long)open) - 1;
          claimed |= 1ull << e;
          if (lane == e) my_row = c * 64 + l;
        }
        if (lane == l) mine[c] = e;
      }
    }
#pragma unroll
    for (int c = 0; c < kBlocks; ++c)
      if (c * 64 + lane < n) match_of[c * 64 + lane] = (short)mine[c];
    claimer[lane] = (short)my_row;
    if (lane == 0) {
      tally[0] = __popcll(claimed);
      tally[2] = k - __popcll(claimed);
      tally[5] = n - n_eligible;
    }
  }
  __syncthreads();

  // 4. a thread per candidate: the smoothed score and the drop test
  for (int c = tid; c < k + n; c += kThreads) {
    unsigned char st = 0;
    if (c < k) {
      const int i = claimer[c];
      const double old = ent[c * kEntry + 13];
      const double d = (i >= 0 ? row[i * kRow + 13] : 0.0) - old;
      const double t = w * d;
      const double s = old + t;
      score[c] = s;
      st = s >= drop_below ? 1 : 2;
    } else if (match_of[c - k] == -1) {
      const double s = row[(c - k) * kRow + 13];
      score[c] = s;
      st = s >= drop_below ? 1 : 2;
    }
    state[c] = st;
  }
  __syncthreads();

  // 5. rank by counting; wavefront 0 counts the tallies
  for (int c = tid; c < k + n; c += kThreads) {
    if (state[c] != 1) continue;
    const double s = score[c];
    int rank = 0;
    for (int j = 0; j < k + n; ++j) {
      const double t = score[j];
      rank += state[j] == 1 && (t > s || (t == s && j < c));
    }
    if (rank < M) dest[rank] = (short)c;
  }
  if (tid < 64) {
    int survivors = 0, dropped = 0, created = 0;
    for (int c0 = 0; c0 < k + n; c0 += 64) {                 // wave-uniform
      const int c = c0 + lane;
      const int st = c < k + n ? state[c] : 0;
      survivors += __popcll(__ballot(st == 1));
      dropped += __popcll(__ballot(st == 2));
      created += __popcll(__ballot(st != 0 && c >= k));
    }
    if (lane == 0) {
      const int kept = survivors < M ? survivors : M;
      n_out = kept;
      tally[1] = created;
      tally[3] = dropped;
      tally[4] = survivors - kept;
    }
  }
  __syncthreads();

  // 6. the frame's block, out_rows, the counts
  const int kept = n_out;
  for (int e = tid; e < M * kEntry; e += kThreads) {
    const int r = e / kEntry, col = e - r * kEntry;
    double v = 0.0;
    if (r < kept) {
      const int c = dest[r];
      if (c < k) {
        const int i = claimer[c];
        if (col < 13) v = i >= 0 ? row[i * kRow + col] : ent[c * kEntry + col];
        else if (col == 13) v = score[c];
        else if (col == 14) v = i >= 0 ? ent[c * kEntry + 14] + 1.0 : ent[c * kEntry + 14];
        else v = i >= 0 ? 0.0 : ent[c * kEntry + 15] + 1.0;
      } else {
        v = col < kRow ? row[(c - k) * kRow + col] : (col == 14 ? 1.0 : 0.0);
      }
    }
    block[e] = v;
    if (col < kRow) orow[r * kRow + col] = v;
  }
  if (tid < kStats) stats[b * kStats + tid] = tally[tid];
  if (tid == 0) {
    bank_count[f] = kept;
    out_count[b] = kept;
  }
}

}  // namespace memory

extern "C" int mono_memory_merge_f64(const double *rows, const int *count, const int *frame, double *bank, int *bank_count,
                                     double momentum, double iou, double drop_below, double *out_rows, int *out_count, int *stats,
                                     int B, int R, int N, int M, void *stream_) {
  if (!rows || !count || !frame || !bank || !bank_count || !out_rows || !out_count || !stats) return -1;
  if (M < 1 || M > memory::kMaxSlots || R < 1 || R > memory::kMaxRows || B < 0 || N < 0 || !(iou > 0.0 && iou <= 1.0) ||
      !(momentum > 0.0 && momentum < 1.0))
    return -2;
  if (B == 0) return 0;
  memory::memory_merge_kernel<<<B, memory::kThreads, 0, (hipStream_t)stream_>>>(rows, count, frame, bank, bank_count, 1.0 - momentum,
                                                                              (float)iou, drop_below, out_rows, out_count, stats, R,
                                                                              N, M);
  return (int)hipGetLastError();
}
