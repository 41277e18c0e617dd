// The matched-pair losses of MonoDETR's SetCriterion in two launches (forward, backward) for all decoder layers:
//   loss_center / loss_bbox  L1 on the 3D-centre projection and the l, r, t, b distances     (monodetr.py:1010-1030)
//   loss_giou                1 - GIoU of the (cx-l, cy-t, cx+r, cy+b) boxes                  (:1032-1044, box_ops)
//   loss_depth               Laplacian aleatoric uncertainty, 1.4142 exp(-s) |d - d*| + s      (:1046-1059)
//   loss_dim                 dimension-aware L1 |s - s*| / s* with the per-layer compensation weight (:1061-1078)
//   loss_angle               12-bin cross entropy + L1 of the target bin's residual           (:1080-1103)
// PyTorch evaluates them with ~60 small kernels forward and ~150 backward (gathers, elementwise ops, index_put
// scatters), enqueued right behind the matcher's host sync where the GPU queue is empty and every launch is exposed.
// One workgroup per decoder layer walks that layer's K matched (image, query, target) triples.
// Outputs are the per-layer SUMS (the caller divides by num_boxes); the backward scatters into zeroed gradients.
#pragma once
#include <hip/hip_runtime.h>

namespace mono {

struct MatchedArgs {
  const float *boxes, *depth, *dims, *angle;        // predictions [NL, B, Q, 6 | 2 | 3 | 24]
  const long long *idx;                             // [3, NL, K]: image, query, flat target index
  const float *t_box, *t_depth, *t_size, *t_res;    // targets [T, 6], [T], [T, 3], [T]
  const long long *t_bin;                           // [T]
  int NL, B, Q, K;
};

__device__ __forceinline__ float sgn(float d) { return (float)(d > 0.f) - (float)(d < 0.f); }

__device__ __forceinline__ float block_sum(float v, float *scratch) {      // 256 threads; result to all
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = v;
  __syncthreads();
  return (scratch[0] + scratch[1]) + (scratch[2] + scratch[3]);
}

// GIoU of a = (x1, y1, x2, y2) against the constant box b, and its gradient with respect to a.
__device__ __forceinline__ float giou_grad(const float a[4], const float b[4], float g[4]) {
  const float aw = a[2] - a[0], ah = a[3] - a[1];
  const float area_a = aw * ah, area_b = (b[2] - b[0]) * (b[3] - b[1]);
  const float iw = fminf(a[2], b[2]) - fmaxf(a[0], b[0]), ih = fminf(a[3], b[3]) - fmaxf(a[1], b[1]);
  const float iwc = fmaxf(iw, 0.f), ihc = fmaxf(ih, 0.f);
  const float inter = iwc * ihc, uni = area_a + area_b - inter;
  const float cw0 = fmaxf(a[2], b[2]) - fminf(a[0], b[0]), ch0 = fmaxf(a[3], b[3]) - fminf(a[1], b[1]);
  const float cw = fmaxf(cw0, 0.f), ch = fmaxf(ch0, 0.f), area_c = cw * ch;
  const float di[4] = {(iw > 0.f && a[0] > b[0]) ? -ihc : 0.f, (ih > 0.f && a[1] > b[1]) ? -iwc : 0.f,
                       (iw > 0.f && a[2] < b[2]) ? ihc : 0.f, (ih > 0.f && a[3] < b[3]) ? iwc : 0.f};
  const float da[4] = {-ah, -aw, ah, aw};
  const float dc[4] = {(cw0 > 0.f && a[0] < b[0]) ? -ch : 0.f, (ch0 > 0.f && a[1] < b[1]) ? -cw : 0.f,
                       (cw0 > 0.f && a[2] > b[2]) ? ch : 0.f, (ch0 > 0.f && a[3] > b[3]) ? cw : 0.f};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float du = da[k] - di[k];
    g[k] = (di[k] * uni - inter * du) / (uni * uni) + (du * area_c - uni * dc[k]) / (area_c * area_c);
  }
  return inter / uni - (area_c - uni) / area_c;
}

struct Pair {
  float box[6], tbox[6], dep[2], tdep, dim[3], tdim[3], ang[24], tres;
  int bin;
  long long row;      // (l * B + b) * Q + q
  long long t;        // flat target
};

__device__ __forceinline__ Pair load_pair(const MatchedArgs &a, int l, int k) {
  Pair p;
  const long long *ip = a.idx + (long long)l * a.K + k;
  const long long stride = (long long)a.NL * a.K;
  const long long b = ip[0], q = ip[stride], t = ip[2 * stride];
  p.row = ((long long)l * a.B + b) * a.Q + q;
  p.t = t;
#pragma unroll
  for (int i = 0; i < 6; ++i) { p.box[i] = a.boxes[p.row * 6 + i]; p.tbox[i] = a.t_box[t * 6 + i]; }
  p.dep[0] = a.depth[p.row * 2]; p.dep[1] = a.depth[p.row * 2 + 1]; p.tdep = a.t_depth[t];
#pragma unroll
  for (int i = 0; i < 3; ++i) { p.dim[i] = a.dims[p.row * 3 + i]; p.tdim[i] = a.t_size[t * 3 + i]; }
#pragma unroll
  for (int i = 0; i < 24; ++i) p.ang[i] = a.angle[p.row * 24 + i];
  p.bin = (int)a.t_bin[t];
  p.tres = a.t_res[t];
  return p;
}

__device__ __forceinline__ void to_xyxy(const float c[6], float o[4]) {
  o[0] = c[0] - c[2]; o[1] = c[1] - c[4]; o[2] = c[0] + c[3]; o[3] = c[1] + c[5];
}

// Per-label weights (W; tw [T], finite, >= 0; nullptr and never read without W): the pair of flat target t enters every sum as
// fma(w_t, term, sum) -- one rounding, so all weights 1 give the unweighted bytes and all weights 0.5 exactly half of them.
template <bool W>
__device__ __forceinline__ float wacc(float w, float term, float acc) {
  if constexpr (W) return __builtin_fmaf(w, term, acc);
  else return acc + term;
}

// out[l] = {center, bbox, giou, depth, dim, angle} sums; comp[l] = sum |s - s*| / sum |s - s*| / s*   (W: every term times w_t)
template <bool W>
__global__ __launch_bounds__(256) void matched_fwd_kernel(const MatchedArgs a, const float *__restrict__ tw, float *__restrict__ out,
                                                          float *__restrict__ comp) {
  __shared__ float scratch[4];
  const int l = blockIdx.x;
  float s_center = 0.f, s_bbox = 0.f, s_giou = 0.f, s_depth = 0.f, s_l1 = 0.f, s_dl = 0.f, s_angle = 0.f;
  for (int k = threadIdx.x; k < a.K; k += 256) {
    const Pair p = load_pair(a, l, k);
    float w = 1.f;
    if constexpr (W) w = tw[p.t];
    s_center = wacc<W>(w, fabsf(p.box[0] - p.tbox[0]) + fabsf(p.box[1] - p.tbox[1]), s_center);
    s_bbox = wacc<W>(w, (fabsf(p.box[2] - p.tbox[2]) + fabsf(p.box[3] - p.tbox[3])) + (fabsf(p.box[4] - p.tbox[4]) + fabsf(p.box[5] - p.tbox[5])),
                     s_bbox);
    float xa[4], xb[4], g[4];
    to_xyxy(p.box, xa);
    to_xyxy(p.tbox, xb);
    s_giou = wacc<W>(w, 1.f - giou_grad(xa, xb, g), s_giou);
    s_depth = wacc<W>(w, 1.4142f * expf(-p.dep[1]) * fabsf(p.dep[0] - p.tdep) + p.dep[1], s_depth);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const float d = fabsf(p.dim[i] - p.tdim[i]);
      s_l1 = wacc<W>(w, d, s_l1);
      s_dl = wacc<W>(w, d / p.tdim[i], s_dl);
    }
    float mx = p.ang[0];
#pragma unroll
    for (int i = 1; i < 12; ++i) mx = fmaxf(mx, p.ang[i]);
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) se += expf(p.ang[i] - mx);
    float logit_t = 0.f, res_p = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { if (i == p.bin) { logit_t = p.ang[i]; res_p = p.ang[12 + i]; } }
    s_angle = wacc<W>(w, (logf(se) + mx - logit_t) + fabsf(res_p - p.tres), s_angle);
  }
  const float c = block_sum(s_center, scratch), bb = block_sum(s_bbox, scratch), gi = block_sum(s_giou, scratch);
  const float dp = block_sum(s_depth, scratch), l1 = block_sum(s_l1, scratch), dl = block_sum(s_dl, scratch);
  const float an = block_sum(s_angle, scratch);
  if (threadIdx.x == 0) {
    const float cp = l1 / dl;                 // mean(l1) / mean(l1 / s*): same element count
    comp[l] = cp;
    out[l * 6 + 0] = c; out[l * 6 + 1] = bb; out[l * 6 + 2] = gi; out[l * 6 + 3] = dp; out[l * 6 + 4] = dl * cp; out[l * 6 + 5] = an;
  }
}

// gradients of sum_l sum_j go[l][j] * out[l][j] scattered to the matched rows (the buffers are zero elsewhere; a
// (layer, image, query) row is matched at most once, so plain stores).  W: the loop below stays the unweighted one, statement for
// statement, and every thread then multiplies the rows it has just stored by their pairs' w_t -- a weight of 1 leaves the sibling's
// bytes, 0.5 halves them, 0 leaves zeros.  (Folding w_t into the loop's expressions lets the compiler vectorise and contract them
// otherwise than in the unweighted instantiation: the last bits differ then.)
template <bool W>
__global__ __launch_bounds__(256) void matched_bwd_kernel(const MatchedArgs a, const float *__restrict__ tw, const float *__restrict__ comp,
                                                          const float *__restrict__ go,
                                                          float *__restrict__ g_boxes, float *__restrict__ g_depth,
                                                          float *__restrict__ g_dims, float *__restrict__ g_angle) {
  const int l = blockIdx.x;
  const float w_center = go[l * 6], w_bbox = go[l * 6 + 1], w_giou = go[l * 6 + 2], w_depth = go[l * 6 + 3];
  const float w_dim = go[l * 6 + 4] * comp[l], w_angle = go[l * 6 + 5];
  for (int k = threadIdx.x; k < a.K; k += 256) {
    const Pair p = load_pair(a, l, k);
    float gb[6];
    gb[0] = w_center * sgn(p.box[0] - p.tbox[0]);
    gb[1] = w_center * sgn(p.box[1] - p.tbox[1]);
#pragma unroll
    for (int i = 2; i < 6; ++i) gb[i] = w_bbox * sgn(p.box[i] - p.tbox[i]);
    float xa[4], xb[4], g[4];
    to_xyxy(p.box, xa);
    to_xyxy(p.tbox, xb);
    (void)giou_grad(xa, xb, g);
    const float s = -w_giou;                                  // loss = 1 - giou
    gb[0] += s * (g[0] + g[2]); gb[1] += s * (g[1] + g[3]);
    gb[2] -= s * g[0]; gb[3] += s * g[2]; gb[4] -= s * g[1]; gb[5] += s * g[3];
#pragma unroll
    for (int i = 0; i < 6; ++i) g_boxes[p.row * 6 + i] = gb[i];
    const float e = 1.4142f * expf(-p.dep[1]), d = p.dep[0] - p.tdep;
    g_depth[p.row * 2] = w_depth * e * sgn(d);
    g_depth[p.row * 2 + 1] = w_depth * (1.f - e * fabsf(d));
#pragma unroll
    for (int i = 0; i < 3; ++i) g_dims[p.row * 3 + i] = w_dim * sgn(p.dim[i] - p.tdim[i]) / p.tdim[i];
    float mx = p.ang[0];
#pragma unroll
    for (int i = 1; i < 12; ++i) mx = fmaxf(mx, p.ang[i]);
    float ex[12], se = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { ex[i] = expf(p.ang[i] - mx); se += ex[i]; }
    const float inv = 1.f / se;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      g_angle[p.row * 24 + i] = w_angle * (ex[i] * inv - (i == p.bin ? 1.f : 0.f));
      g_angle[p.row * 24 + 12 + i] = (i == p.bin) ? w_angle * sgn(p.ang[12 + i] - p.tres) : 0.f;
    }
  }
  if constexpr (W) {
    const long long stride = (long long)a.NL * a.K;
    for (int k = threadIdx.x; k < a.K; k += 256) {          // the same k as above: a thread rereads its own stores
      const long long *ip = a.idx + (long long)l * a.K + k;
      const long long row = ((long long)l * a.B + ip[0]) * a.Q + ip[stride];
      const float w = tw[ip[2 * stride]];
      for (int i = 0; i < 6; ++i) g_boxes[row * 6 + i] *= w;
      for (int i = 0; i < 2; ++i) g_depth[row * 2 + i] *= w;
      for (int i = 0; i < 3; ++i) g_dims[row * 3 + i] *= w;
      for (int i = 0; i < 24; ++i) g_angle[row * 24 + i] *= w;
    }
  }
}

// ---- label audit (monosowa_amd/label_audit.py): the terms above per LABEL instead of per layer -----------------------------------------
//   out[t] = means over the pairs of one layer that are matched to flat target t of
//            { |dcx| + |dcy|, l/r/t/b L1, 1 - GIoU, Laplacian depth term, |d - d*|, sum |s - s*|, heading CE + residual L1,
//              sigmoid(logit of the label's class) }, then the number of pairs -- nine doubles.
// Every term is matched_fwd_kernel's float32 expression on the same load_pair; it is widened to double, added in double and divided
// by the count in double.  One wavefront per label: its lanes stride over k (fixed order per lane), a fixed xor tree adds the lanes.
// No atomics, nothing depends on where out lies.  A label without a pair: nine zeros.  A pair whose image or query index lies
// outside [0, B) x [0, Q) is counted nowhere (nothing is read through it).
constexpr int kAuditCols = 9;
constexpr int kAuditLabelsPerBlock = 4;               // wavefronts of a 256-thread workgroup

struct AuditArgs {
  MatchedArgs m;
  const float *logits;                // [NL, B, Q, C]
  const long long *labels;            // [T] class of every target
  int C, T, layer;
};

__global__ __launch_bounds__(256) void label_audit_kernel(const AuditArgs a, double *__restrict__ out) {
  const int t = blockIdx.x * kAuditLabelsPerBlock + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (t >= a.T) return;                               // whole wavefronts leave: the shuffles below see all 64 lanes
  const int l = a.layer;
  const long long stride = (long long)a.m.NL * a.m.K;
  const long long *bi = a.m.idx + (long long)l * a.m.K, *qi = bi + stride, *ti = bi + 2 * stride;
  const long long cls = a.labels[t];
  double s[kAuditCols - 1] = {0., 0., 0., 0., 0., 0., 0., 0.}, n = 0.;
  for (int k = lane; k < a.m.K; k += 64) {
    if (ti[k] != (long long)t) continue;
    if ((unsigned long long)bi[k] >= (unsigned long long)a.m.B || (unsigned long long)qi[k] >= (unsigned long long)a.m.Q) continue;
    const Pair p = load_pair(a.m, l, k);
    s[0] += (double)(fabsf(p.box[0] - p.tbox[0]) + fabsf(p.box[1] - p.tbox[1]));
    s[1] += (double)((fabsf(p.box[2] - p.tbox[2]) + fabsf(p.box[3] - p.tbox[3])) + (fabsf(p.box[4] - p.tbox[4]) + fabsf(p.box[5] - p.tbox[5])));
    float xa[4], xb[4], g[4];
    to_xyxy(p.box, xa);
    to_xyxy(p.tbox, xb);
    s[2] += (double)(1.f - giou_grad(xa, xb, g));
    s[3] += (double)(1.4142f * expf(-p.dep[1]) * fabsf(p.dep[0] - p.tdep) + p.dep[1]);
    s[4] += (double)fabsf(p.dep[0] - p.tdep);
    float l1 = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) l1 += fabsf(p.dim[i] - p.tdim[i]);
    s[5] += (double)l1;
    float mx = p.ang[0];
#pragma unroll
    for (int i = 1; i < 12; ++i) mx = fmaxf(mx, p.ang[i]);
    float se = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) se += expf(p.ang[i] - mx);
    float logit_t = 0.f, res_p = 0.f;
#pragma unroll
    for (int i = 0; i < 12; ++i) { if (i == p.bin) { logit_t = p.ang[i]; res_p = p.ang[12 + i]; } }
    s[6] += (double)((logf(se) + mx - logit_t) + fabsf(res_p - p.tres));
    // a class outside [0, C) names no logit: NaN, nothing is read
    const float x = (cls >= 0 && cls < a.C) ? a.logits[p.row * a.C + cls] : __builtin_nanf("");
    s[7] += (double)(1.f / (1.f + expf(-x)));
    n += 1.;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
    for (int j = 0; j < kAuditCols - 1; ++j) s[j] += __shfl_xor(s[j], o);
    n += __shfl_xor(n, o);
  }
  if (lane == 0) {
    double *row = out + (long long)t * kAuditCols;
#pragma unroll
    for (int j = 0; j < kAuditCols - 1; ++j) row[j] = n > 0. ? s[j] / n : 0.;
    row[kAuditCols - 1] = n;
  }
}

// ---- classification side of the criterion for all decoder layers (monodetr.py:396-449, sigmoid_focal_loss :302-330) -------------
//   out[l] = { sum over (image, query, class) of the sigmoid focal loss against the matched one-hot targets,
//              class_error = 100 - top-1 accuracy of the matched queries in %,
//              cardinality_error = mean over images of | #(queries whose arg-max is not the last class) - #targets | }
// PyTorch: ~25 small kernels forward (one-hot scatter, sigmoid, BCE, p_t, modulation, alpha weighting, reductions, arg-max
// bookkeeping) and ~30 backward, in the stretch behind the matcher's synchronisation where every launch is exposed.  One
// workgroup per layer: the layer's matched (image, query) -> class map lives in LDS.
constexpr int kFocalThreads = 1024;
constexpr int kFocalMaxCells = 32768;                 // B * Q cells of the class map (bytes of LDS)
// with per-label weights a cell also keeps the pair that claimed it (16 bits; its weight is tw[flat target of that pair]): 3 bytes of
// LDS per cell, 48 KB at the reach below
constexpr int kFocalWeightedMaxCells = 16384;
constexpr unsigned short kFocalNoPair = 0xffff;

struct FocalArgs {
  const float *logits;                // [NL, B, Q, C]
  const long long *idx;               // [3, NL, K]: image, query, flat target
  const long long *labels;            // [T] class of every target
  const float *sizes;                 // [B] targets per image (cardinality)
  int NL, B, Q, C, K;
  float alpha, gamma;
};

template <bool W>
__device__ __forceinline__ void focal_class_map(const FocalArgs &a, int l, unsigned char *cls, unsigned short *pair) {
  const int cells = a.B * a.Q;
  for (int i = threadIdx.x; i < cells; i += kFocalThreads) {
    cls[i] = (unsigned char)a.C;          // C = "no object"
    if constexpr (W) pair[i] = kFocalNoPair;
  }
  __syncthreads();
  const long long *bi = a.idx + (long long)l * a.K, *qi = a.idx + ((long long)a.NL + l) * a.K, *ti = a.idx + ((long long)2 * a.NL + l) * a.K;
  for (int k = threadIdx.x; k < a.K; k += kFocalThreads) {
    cls[bi[k] * a.Q + qi[k]] = (unsigned char)a.labels[ti[k]];
    if constexpr (W) pair[bi[k] * a.Q + qi[k]] = (unsigned short)k;
  }
  __syncthreads();
}

// weight of a cell: its target's, 1 for a cell no pair claimed
__device__ __forceinline__ float focal_cell_weight(const FocalArgs &a, int l, const float *__restrict__ tw, unsigned short k) {
  return k == kFocalNoPair ? 1.f : tw[a.idx[((long long)2 * a.NL + l) * a.K + k]];
}

// focal term of one logit x against target t in {0, 1} and its derivative (alpha < 0: no alpha weighting)
__device__ __forceinline__ float focal_term(float x, bool t, float alpha, float gamma, float *dfdx) {
  // log p = -softplus(-x), log(1 - p) = -softplus(x); softplus(z) = max(z, 0) + log1p(exp(-|z|))
  const float lse = log1pf(expf(-fabsf(x)));
  const float log_p = -(fmaxf(-x, 0.f) + lse), log_1p = -(fmaxf(x, 0.f) + lse);
  const float p = 1.f / (1.f + expf(-x));
  const float q = t ? 1.f - p : p;                       // 1 - p_t
  const float ce = t ? -log_p : -log_1p;
  const float w = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  const float mod = gamma == 2.f ? q * q : powf(q, gamma);
  if (dfdx) {
    // d q / dx = -+ p (1 - p); d ce / dx = -(1 - p) (t = 1), p (t = 0)
    const float dq = t ? -p * (1.f - p) : p * (1.f - p);
    const float dce = t ? -(1.f - p) : p;
    const float dmod = gamma == 2.f ? 2.f * q : gamma * powf(q, gamma - 1.f);
    *dfdx = w * (dmod * dq * ce + mod * dce);
  }
  return w * mod * ce;
}

// W: all C terms of a matched cell times the weight of its target; the two logging entries stay unweighted.  The unweighted forward
// adds alpha_t * mod * ce as ONE fma((alpha_t * mod), ce, sum) (the compiler contracts the term's last product into the accumulation);
// the weighted one spells that fma out with the cell's weight folded into the first factor, so a weight of 1 gives the same bytes and
// a weight of 0 leaves the sum.  focal_factors: the two factors, focal_term's own expressions.
__device__ __forceinline__ void focal_factors(float x, bool t, float alpha, float gamma, float &wmod, float &ce) {
  const float lse = log1pf(expf(-fabsf(x)));
  const float log_p = -(fmaxf(-x, 0.f) + lse), log_1p = -(fmaxf(x, 0.f) + lse);
  const float p = 1.f / (1.f + expf(-x));
  const float q = t ? 1.f - p : p;
  ce = t ? -log_p : -log_1p;
  const float w = alpha >= 0.f ? (t ? alpha : 1.f - alpha) : 1.f;
  wmod = w * (gamma == 2.f ? q * q : powf(q, gamma));
}

// I (ignore regions): a cell that no pair claimed (LDS class C) and whose byte of ign [NL, B, Q] is set adds none of its C terms: the
// terms are evaluated like the sibling's, fma for fma, and the running sum is kept by a select, so a non-finite logit of such a cell
// never reaches it and every other cell adds the sibling's bits.  The two logging entries count every cell, as before.
template <bool W, bool I = false>
__global__ __launch_bounds__(kFocalThreads) void focal_fwd_kernel(const FocalArgs a, const float *__restrict__ tw, float *__restrict__ out,
                                                                  const unsigned char *__restrict__ ign = nullptr) {
  __shared__ unsigned char cls[W ? kFocalWeightedMaxCells : kFocalMaxCells];
  __shared__ unsigned short pair[W ? kFocalWeightedMaxCells : 1];
  __shared__ float red[kFocalThreads / 64];
  __shared__ int card[256], correct;
  const int l = blockIdx.x, cells = a.B * a.Q;
  if (threadIdx.x < 256) card[threadIdx.x] = 0;
  if (threadIdx.x == 0) correct = 0;
  focal_class_map<W>(a, l, cls, pair);
  const float *lg = a.logits + (long long)l * cells * a.C;
  float sum = 0.f;
  for (int i = threadIdx.x; i < cells; i += kFocalThreads) {
    const int t = cls[i];
    float w = 1.f;
    if constexpr (W) w = focal_cell_weight(a, l, tw, pair[i]);
    bool skip = false;
    if constexpr (I) skip = t == a.C && ign[(long long)l * cells + i] != 0;
    int best = 0;
    float bv = lg[(long long)i * a.C];
    for (int c = 0; c < a.C; ++c) {
      const float x = lg[(long long)i * a.C + c];
      if constexpr (I) {
        float wmod, ce;
        focal_factors(x, c == t, a.alpha, a.gamma, wmod, ce);
        const float with = __builtin_fmaf(wmod * w, ce, sum);
        sum = skip ? sum : with;
      } else if constexpr (W) {
        float wmod, ce;
        focal_factors(x, c == t, a.alpha, a.gamma, wmod, ce);
        sum = __builtin_fmaf(wmod * w, ce, sum);
      } else {
        sum += focal_term(x, c == t, a.alpha, a.gamma, nullptr);
      }
      if (x > bv) { bv = x; best = c; }                 // first maximum, like torch.argmax
    }
    if (best != a.C - 1) atomicAdd(&card[i / a.Q], 1);
    if (t < a.C && best == t) atomicAdd(&correct, 1);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int w = 0; w < kFocalThreads / 64; ++w) tot += red[w];
    float ce = 0.f;
    for (int b = 0; b < a.B; ++b) ce += fabsf((float)card[b] - a.sizes[b]);
    out[l * 3] = tot;
    // 100 * wrong / K, not 100 - 100 * correct / K: the subtraction cancels the leading digits of a small error
    out[l * 3 + 1] = a.K > 0 ? 100.f * (float)(a.K - correct) / (float)a.K : 100.f;
    out[l * 3 + 2] = ce / (float)a.B;
  }
}

// grad_logits[l, b, q, c] = grad_out[l] * d focal / d logit     (grad_out: gradient of the per-layer focal SUM)
// W: the unweighted loop, statement for statement, then the C gradients of every matched cell times the weight of its target (see
// matched_bwd_kernel); the workgroup meets in between, a cell's gradients come from other threads.
// I: the row of an ignored cell (see focal_fwd_kernel) is written as +0.0, whatever its logits hold -- stored over what the unweighted
// loop left there, in a pass of its own behind it, like the weights: a select inside the loop changed the compiler's contraction of the
// other rows' expressions, and those are the sibling's bytes.
template <bool W, bool I = false>
__global__ __launch_bounds__(kFocalThreads) void focal_bwd_kernel(const FocalArgs a, const float *__restrict__ tw,
                                                                  const float *__restrict__ grad_out, float *__restrict__ grad_logits,
                                                                  const unsigned char *__restrict__ ign = nullptr) {
  __shared__ unsigned char cls[kFocalMaxCells];
  const int l = blockIdx.x, cells = a.B * a.Q;
  focal_class_map<false>(a, l, cls, nullptr);
  const float *lg = a.logits + (long long)l * cells * a.C;
  float *gl = grad_logits + (long long)l * cells * a.C;
  const float g = grad_out[l];
  for (int i = threadIdx.x; i < cells * a.C; i += kFocalThreads) {
    const int cell = i / a.C, c = i - cell * a.C;
    float d;
    (void)focal_term(lg[i], c == cls[cell], a.alpha, a.gamma, &d);
    gl[i] = g * d;
  }
  if constexpr (W) {
    __syncthreads();
    const long long *bi = a.idx + (long long)l * a.K, *qi = a.idx + ((long long)a.NL + l) * a.K, *ti = a.idx + ((long long)2 * a.NL + l) * a.K;
    for (int k = threadIdx.x; k < a.K; k += kFocalThreads) {
      const float w = tw[ti[k]];
      float *row = gl + (bi[k] * a.Q + qi[k]) * a.C;
      for (int c = 0; c < a.C; ++c) row[c] *= w;
    }
  }
  if constexpr (I) {
    __syncthreads();
    for (int cell = threadIdx.x; cell < cells; cell += kFocalThreads) {
      if (cls[cell] != a.C || ign[(long long)l * cells + cell] == 0) continue;
      float *row = gl + (long long)cell * a.C;
      for (int c = 0; c < a.C; ++c) row[c] = 0.f;
    }
  }
}


// ---- the matcher's cost blocks (matcher.py:60-99 of this repo = the reference's matcher.py:53-88 restricted to each image's own
// targets) as one launch.  One thread per (layer, image, query, target slot).  Every operation is the PyTorch expression's own,
// rounded individually and in its order (no contraction: rn()), with the same elementary functions (expf / logf of the device
// library): the floats -- and with them the assignments -- are those of the ~70 elementwise launches it replaces.
// exp / log exactly as PyTorch's elementwise kernels evaluate them: the device library's functions by name.  (hipcc 7.2 expands a
// plain `logf` through the backend's own lowering, which differs from __ocml_log_f32 in the last bit for a third of the arguments
// in (0, 1): tools/ubench/log_variants.hip.)
extern "C" __device__ float __ocml_exp_f32(float);
extern "C" __device__ float __ocml_log_f32(float);

struct CostArgs {
  const float *logits, *boxes;         // [NL, B, Q, C], [NL, B, Q, 6]
  const long long *labels;             // [T]
  const float *tboxes;                 // [T, 6]
  const long long *cols;               // [B, N]: flat target of slot j of image b (padding slots repeat a valid target)
  int NL, B, Q, C, N;
  float w_class, w_3d, w_bbox, w_giou;
};

__device__ __forceinline__ float rn_mul(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float rn_add(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float rn_sub(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

__global__ __launch_bounds__(256) void match_cost_kernel(const CostArgs a, float *__restrict__ out) {
  const long long n = (long long)a.NL * a.B * a.Q * a.N;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int j = (int)(i % a.N);
  const long long cell = i / a.N;                          // (l, b, q)
  const int b = (int)((cell / a.Q) % a.B);
  const long long t = a.cols[(long long)b * a.N + j];
  const long long id = a.labels[t];
  // focal-style classification cost of the target's class
  const float x = a.logits[cell * a.C + id];
  const float p = 1.0f / rn_add(1.0f, __ocml_exp_f32(-x));                                           // sigmoid
  const float neg = rn_mul(rn_mul(0.75f, rn_mul(p, p)), -__ocml_log_f32(rn_add(rn_sub(1.0f, p), 1e-8f)));
  const float omp = rn_sub(1.0f, p);
  const float pos = rn_mul(rn_mul(0.25f, rn_mul(omp, omp)), -__ocml_log_f32(rn_add(p, 1e-8f)));
  const float cost_class = rn_sub(pos, neg);
  const float *pb = a.boxes + cell * 6, *tb = a.tboxes + t * 6;
  float pa[6], ta[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { pa[k] = pb[k]; ta[k] = tb[k]; }
  const float c3d = rn_add(fabsf(rn_sub(pa[0], ta[0])), fabsf(rn_sub(pa[1], ta[1])));
  float cbb = rn_add(fabsf(rn_sub(pa[2], ta[2])), fabsf(rn_sub(pa[3], ta[3])));
  cbb = rn_add(cbb, fabsf(rn_sub(pa[4], ta[4])));
  cbb = rn_add(cbb, fabsf(rn_sub(pa[5], ta[5])));
  // (cx, cy, l, r, t, b) -> (cx - l, cy - t, cx + r, cy + b)
  const float ax0 = rn_sub(pa[0], pa[2]), ay0 = rn_sub(pa[1], pa[4]), ax1 = rn_add(pa[0], pa[3]), ay1 = rn_add(pa[1], pa[5]);
  const float bx0 = rn_sub(ta[0], ta[2]), by0 = rn_sub(ta[1], ta[4]), bx1 = rn_add(ta[0], ta[3]), by1 = rn_add(ta[1], ta[5]);
  const float area1 = rn_mul(rn_sub(ax1, ax0), rn_sub(ay1, ay0)), area2 = rn_mul(rn_sub(bx1, bx0), rn_sub(by1, by0));
  // torch.min / torch.max / clamp(min=0) hand NaNs on (fminf / fmaxf would drop them)
  auto tmin = [](const float u, const float v) { return (u != u || u < v) ? u : v; };
  auto tmax = [](const float u, const float v) { return (u != u || u > v) ? u : v; };
  auto relu = [](const float u) { return u < 0.f ? 0.f : u; };
  const float w = relu(rn_sub(tmin(ax1, bx1), tmax(ax0, bx0))), h = relu(rn_sub(tmin(ay1, by1), tmax(ay0, by0)));
  const float inter = rn_mul(w, h);
  const float uni = rn_sub(rn_add(area1, area2), inter);
  const float iou = inter / uni;
  const float wc = relu(rn_sub(tmax(ax1, bx1), tmin(ax0, bx0))), hc = relu(rn_sub(tmax(ay1, by1), tmin(ay0, by0)));
  const float area = rn_mul(wc, hc);
  const float cost_giou = -rn_sub(iou, rn_sub(area, uni) / area);
  float c = rn_add(rn_mul(a.w_bbox, cbb), rn_mul(a.w_3d, c3d));
  c = rn_add(c, rn_mul(a.w_class, cost_class));
  c = rn_add(c, rn_mul(a.w_giou, cost_giou));
  out[i] = c;
}

// ---- ignore regions: which queries sit on an object that is known to exist and is no target -----------------------------------------
//   flags[l, b, q] = 1 when for some valid box g of image b, with p = (cx - l, cy - t, cx + r, cy + b) of the predicted box and
//   A = (p.x2 - p.x1)(p.y2 - p.y1):   A > 0,  iw = min(p.x2, g.x2) - max(p.x1, g.x1) > 0,  ih likewise > 0,  iw ih >= ioa A
// -- intersection over the QUERY's area.  float32, every operation rounded on its own (rn()), min / max handing NaNs on like
// torch.minimum / np.minimum, so a NaN anywhere fails the comparisons and a numpy float32 restatement gives the same bytes.  Whether the
// cell is matched is not known here: the focal kernels look at that.  One workgroup per layer, which also writes the layer's number
// of flagged cells (LDS tree, no atomics, nothing to zero first); the launch does not depend on the matching.
constexpr int kIgnoreThreads = 1024;

struct IgnoreArgs {
  const float *boxes;                  // [NL, B, Q, 6]
  const float *ign;                    // [B, M, 4] x1, y1, x2, y2
  const unsigned char *mask;           // [B, M]
  int NL, B, Q, M;
  float ioa;
};

__global__ __launch_bounds__(kIgnoreThreads) void ignore_flags_kernel(const IgnoreArgs a, unsigned char *__restrict__ flags,
                                                                      int *__restrict__ counts) {
  __shared__ int red[kIgnoreThreads / 64];
  const int l = blockIdx.x, cells = a.B * a.Q;
  auto tmin = [](const float u, const float v) { return (u != u || u < v) ? u : v; };
  auto tmax = [](const float u, const float v) { return (u != u || u > v) ? u : v; };
  int n = 0;
  for (int i = threadIdx.x; i < cells; i += kIgnoreThreads) {
    const int b = i / a.Q;
    const float *pb = a.boxes + ((long long)l * cells + i) * 6;
    const float x1 = rn_sub(pb[0], pb[2]), y1 = rn_sub(pb[1], pb[4]), x2 = rn_add(pb[0], pb[3]), y2 = rn_add(pb[1], pb[5]);
    const float area = rn_mul(rn_sub(x2, x1), rn_sub(y2, y1));
    const float need = rn_mul(a.ioa, area);
    bool hit = false;
    if (area > 0.f) {
      const float *g = a.ign + (long long)b * a.M * 4;
      const unsigned char *m = a.mask + (long long)b * a.M;
      // the mask bytes eight at a time: one byte load per slot behind a branch each is a chain of 50 load latencies per cell
      for (int j0 = 0; j0 < a.M; j0 += 8) {
        unsigned char mm[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) mm[u] = j0 + u < a.M ? m[j0 + u] : (unsigned char)0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          if (!mm[u]) continue;
          const int j = j0 + u;
          const float iw = rn_sub(tmin(x2, g[j * 4 + 2]), tmax(x1, g[j * 4 + 0]));
          const float ih = rn_sub(tmin(y2, g[j * 4 + 3]), tmax(y1, g[j * 4 + 1]));
          hit = hit || (iw > 0.f && ih > 0.f && rn_mul(iw, ih) >= need);
        }
      }
    }
    flags[(long long)l * cells + i] = hit ? 1 : 0;
    n += hit ? 1 : 0;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) n += __shfl_xor(n, o);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    int tot = 0;
    for (int w = 0; w < kIgnoreThreads / 64; ++w) tot += red[w];
    counts[l] = tot;
  }
}

}  // namespace mono
