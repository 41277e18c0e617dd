// ---- KITTI rows -> the padded training targets of the dataset (included by rotate_iou.hip): the inverse of decode_dets_kernel ----
// rows f64 [B, R, 14] (cls, alpha, x1, y1, x2, y2, h, w, l, x, y, z, ry, score; kept rows first) + count [B] + one camera /
// augmentation record per image, f64 [B, 23] = (P2's 12 float32 values, img_w, img_h, flip, the six numbers of the crop's affine
// `trans`, crop_scale, canonical_scale) -> every array of KITTI_Dataset.__getitem__'s target dict as [B, max_objs, ...] in the
// dataset's dtypes, plus label_weight, ignore_boxes / ignore_mask and n_ignore [B].
//
// Slot i < min(count, R, max_objs) is line i of the label file that holds row i with every number written exactly -- a row with
// !(score >= min_score) as the DontCare line of write_kitti_results -- read by kitti_dataset.py's __getitem__ on a training split
// with label_weights 'score' and ignore_regions on, under the record's flip and crop.  The sequence below is that method's, line
// by line, with numpy's promotions: box2d and pos are float32; the level is UnKnown for !(y2 - y1 + 1 >= 25) (truncation and
// occlusion are 0); the depth gate [2, 65] reads the unscaled float32 z; labels and size_2d are written before the l / r / t / b
// rule drops the line; pos z is multiplied by canonical_scale before depth and objects read it; the heading is float32 arithmetic
// on the flipped ry and the flipped box centre; every stored value is rounded to its array's dtype once.  Two stated differences
// from the class: the two small matrix products (rect_to_img's hom . P2^T, affine_transform's 2 x 3 product) are evaluated left to
// right in double, each operation rounded, where numpy hands them to BLAS; and the float32 atan2 of the heading is the double
// atan2 rounded once.  Nothing contracts to a fused multiply-add.
//
// One wavefront per image, one lane per slot (max_objs <= 64).  A lane writes its own slot of every array, zeros included, so no
// output needs clearing first; the ignore boxes are packed at the front in line order by one ballot and a prefix count through
// 1 KB of LDS.  No atomics, no scratch, plain per-element stores with no alignment assumed: the same bytes wherever the outputs lie.
namespace encode {

constexpr int kLanes = 64;
constexpr int kRow = 14;
constexpr int kRecord = 23;              // doubles per image record
constexpr int kOutputs = 17;

struct Outputs {                         // device pointers, [B, max_objs, ...] each; the order of include/monosowa_kitti.h
  signed char *labels;                   // int8
  float *boxes;                          // [.., 4]
  float *boxes_3d;                       // [.., 6]
  float *depth;                          // [.., 1]
  float *size_2d;                        // [.., 2]
  float *size_3d;                        // [.., 3]
  float *src_size_3d;                    // [.., 3]
  long long *heading_bin;                // int64 [.., 1]
  float *heading_res;                    // [.., 1]
  unsigned char *mask_2d;                // bool
  float *calibs;                         // [.., 3, 4]
  long long *indices;                    // int64
  float *objects;                        // [.., 7]
  float *label_weight;
  float *ignore_boxes;                   // [.., 4]
  unsigned char *ignore_mask;            // bool
  int *n_ignore;                         // [B]
};

struct Settings {
  int writelist_mask, depth_mode, clip_2d, weight_mode;
  double min_score, weight;
  int res_w, res_h, R, C, max_objs;
};

__device__ __forceinline__ float remainder_f32(float a, float b) {      // numpy's float32 `%` for b > 0
#pragma clang fp contract(off)
  float m = fmodf(a, b);
  if (m != 0.f) {
    if (m < 0.f) m += b;
  } else {
    m = 0.f;
  }
  return m;
}

__device__ __forceinline__ float wrap_f32(float a) {                     // a float32 angle against Python's pi: compared in float32
#pragma clang fp contract(off)
  const float kPi = 3.141592653589793f, kTwoPi = (float)(2 * 3.141592653589793);
  return a > kPi ? a - kTwoPi : (a < -kPi ? a + kTwoPi : a);
}

__device__ __forceinline__ double clip01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }
__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

__global__ __launch_bounds__(kLanes) void encode_targets_kernel(const double *__restrict__ rows, const int *__restrict__ count,
                                                               const double *__restrict__ records,
                                                               const double *__restrict__ cls_mean_size, Settings s, Outputs o) {
#pragma clang fp contract(off)
  __shared__ float packed[kLanes * 4];
  const int b = blockIdx.x, lane = threadIdx.x;
  const double *rec = records + (long long)b * kRecord;
  float P[12];
  for (int k = 0; k < 12; ++k) P[k] = (float)rec[k];
  const double img_w = rec[12];
  const bool flip = rec[14] != 0.0;
  const double t0 = rec[15], t1 = rec[16], t2 = rec[17], t3 = rec[18], t4 = rec[19], t5 = rec[20];
  const double crop_scale = rec[21], canonical_scale = rec[22];
  const double res_w = (double)s.res_w, res_h = (double)s.res_h;
  const double kPi = 3.141592653589793, kTwoPi = 2 * kPi, kBin = kTwoPi / 12.0;

  int n = count[b];
  n = n < 0 ? 0 : n;
  n = n > s.R ? s.R : n;
  n = n > s.max_objs ? s.max_objs : n;
  const bool slot = lane < s.max_objs, live = lane < n;

  // the slot's values: what the class leaves in a slot it never touches
  int label = 0, bin = 0;
  float box[4] = {0.f, 0.f, 0.f, 0.f}, box3d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, depth = 0.f, size2d[2] = {0.f, 0.f};
  float size3d[3] = {0.f, 0.f, 0.f}, src3d[3] = {0.f, 0.f, 0.f}, res = 0.f, obj[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float weight = 1.f, ig[4] = {0.f, 0.f, 0.f, 0.f};
  bool target = false, ignore = false;

  if (live) {
    const double *r = rows + ((long long)b * s.R + lane) * kRow;
    const double cls_d = r[0], score = r[13];
    const bool dontcare = !(score >= s.min_score);
    const bool named = cls_d > -1.0 && cls_d < (double)s.C;
    const int cls = named ? (int)cls_d : 0;
    const bool listed = !dontcare && named && ((s.writelist_mask >> cls) & 1);
    if (s.weight_mode == 0)
      weight = (score >= 0.0 && score <= 1.7976931348623157e308) ? (float)score : 0.f;   // the class refuses such a line
    else
      weight = (float)s.weight;
    // Object3d: float32 box and position; the flip of __getitem__
    float x1 = (float)r[2], x2 = (float)r[4];
    const float y1 = (float)r[3], y2 = (float)r[5];
    const double h = r[6], w = r[7], l = r[8];
    const float px = (float)r[9], py = (float)r[10], pz = (float)r[11];
    double ry = r[12];
    const bool unknown = !((double)y2 - (double)y1 + 1.0 >= 25.0);
    if (flip) {
      const float fx1 = (float)(img_w - (double)x2), fx2 = (float)(img_w - (double)x1);
      x1 = fx1;
      x2 = fx2;
      ry = kPi - ry;
      ry = ry > kPi ? ry - kTwoPi : (ry < -kPi ? ry + kTwoPi : ry);
    }
    ignore = dontcare || listed;              // a writelist line is taken off again when it ends as a target
    if (listed && !unknown && !(pz < 2.f || pz > 65.f)) {
      const float bx0 = (float)(t0 * (double)x1 + t1 * (double)y1 + t2), by0 = (float)(t3 * (double)x1 + t4 * (double)y1 + t5);
      const float bx1 = (float)(t0 * (double)x2 + t1 * (double)y2 + t2), by1 = (float)(t3 * (double)x2 + t4 * (double)y2 + t5);
      const float c2x = (bx0 + bx1) / 2.f, c2y = (by0 + by1) / 2.f;
      // the box centre (not the bottom centre) through P2, left to right in double
      const double X = (double)px, Y = (double)py + (-(h / 2)), Z = (double)pz;
      const double p0 = X * (double)P[0] + Y * (double)P[1] + Z * (double)P[2] + (double)P[3];
      const double p1 = X * (double)P[4] + Y * (double)P[5] + Z * (double)P[6] + (double)P[7];
      double u = p0 / Z;
      const double v = p1 / Z;
      if (flip) u = img_w - u;
      const float uf = (float)u, vf = (float)v;
      const double cx = t0 * (double)uf + t1 * (double)vf + t2, cy = t3 * (double)uf + t4 * (double)vf + t5;
      if (!(cx < 0.0 || cx >= res_w || cy < 0.0 || cy >= res_h)) {
        label = cls;
        size2d[0] = bx1 - bx0;
        size2d[1] = by1 - by0;
        const float k0 = (float)((double)bx0 / res_w), k1 = (float)((double)by0 / res_h);
        const float k2 = (float)((double)bx1 / res_w), k3 = (float)((double)by1 / res_h);
        const double c3x = cx / res_w, c3y = cy / res_h;
        double el = c3x - (double)k0, er = (double)k2 - c3x, et = c3y - (double)k1, eb = (double)k3 - c3y;
        bool keep = true;
        if (el < 0.0 || er < 0.0 || et < 0.0 || eb < 0.0) {
          keep = s.clip_2d != 0;
          el = clip01(el);
          er = clip01(er);
          et = clip01(et);
          eb = clip01(eb);
        }
        if (keep) {
          target = true;
          ignore = false;
          box[0] = (float)((double)c2x / res_w);
          box[1] = (float)((double)c2y / res_h);
          box[2] = (float)((double)size2d[0] / res_w);
          box[3] = (float)((double)size2d[1] / res_h);
          box3d[0] = (float)c3x;
          box3d[1] = (float)c3y;
          box3d[2] = (float)el;
          box3d[3] = (float)er;
          box3d[4] = (float)et;
          box3d[5] = (float)eb;
          const float z = (float)((double)pz * canonical_scale);           // Canonical Object Space
          depth = s.depth_mode == 0 ? (float)((double)z * crop_scale) : (s.depth_mode == 1 ? (float)((double)z / crop_scale) : z);
          // ry2alpha on float32 intrinsics, then angle2class: float32 throughout
          const float centre = (x1 + x2) / 2.f;
          const float at = (float)atan2((double)(centre - P[2]), (double)P[0]);
          float hd = wrap_f32(wrap_f32((float)ry - at));
          const float two_pi = (float)kTwoPi;
          hd = remainder_f32(hd, two_pi);
          const float shifted = remainder_f32(hd + (float)(kBin / 2), two_pi);
          const float q = shifted / (float)kBin;
          bin = q == q ? (int)q : 0;
          res = shifted - (float)((double)bin * kBin + kBin / 2);
          src3d[0] = (float)h;
          src3d[1] = (float)w;
          src3d[2] = (float)l;
          for (int k = 0; k < 3; ++k) size3d[k] = (float)((double)src3d[k] - cls_mean_size[cls * 3 + k]);
          obj[0] = src3d[0];
          obj[1] = src3d[1];
          obj[2] = src3d[2];
          obj[3] = px;
          obj[4] = py;
          obj[5] = z;
          obj[6] = (float)ry;
        }
      }
    }
    if (ignore) {                             // _ignore_boxes: the flipped box through the crop, normalised and clipped, float32
      const float fw = (float)s.res_w, fh = (float)s.res_h;
      ig[0] = clip01((float)(t0 * (double)x1 + t1 * (double)y1 + t2) / fw);
      ig[1] = clip01((float)(t3 * (double)x1 + t4 * (double)y1 + t5) / fh);
      ig[2] = clip01((float)(t0 * (double)x2 + t1 * (double)y2 + t2) / fw);
      ig[3] = clip01((float)(t3 * (double)x2 + t4 * (double)y2 + t5) / fh);
      if (ig[2] <= ig[0] || ig[3] <= ig[1]) ignore = false;      // empty after the clip
    }
  }

  // the ignore boxes packed at the front in line order
  const unsigned long long votes = __ballot(ignore);
  const int total = __popcll(votes), before = __popcll(votes & ((1ull << lane) - 1ull));
  if (ignore)
    for (int k = 0; k < 4; ++k) packed[before * 4 + k] = ig[k];
  __syncthreads();
  if (lane == 0) o.n_ignore[b] = total;
  if (!slot) return;

  const long long i = (long long)b * s.max_objs + lane;
  o.labels[i] = (signed char)label;
  for (int k = 0; k < 4; ++k) o.boxes[i * 4 + k] = box[k];
  for (int k = 0; k < 6; ++k) o.boxes_3d[i * 6 + k] = box3d[k];
  o.depth[i] = depth;
  o.size_2d[i * 2] = size2d[0];
  o.size_2d[i * 2 + 1] = size2d[1];
  for (int k = 0; k < 3; ++k) {
    o.size_3d[i * 3 + k] = size3d[k];
    o.src_size_3d[i * 3 + k] = src3d[k];
  }
  o.heading_bin[i] = (long long)bin;
  o.heading_res[i] = res;
  o.mask_2d[i] = target ? 1 : 0;
  for (int k = 0; k < 12; ++k) o.calibs[i * 12 + k] = target ? P[k] : 0.f;
  o.indices[i] = 0;
  for (int k = 0; k < 7; ++k) o.objects[i * 7 + k] = obj[k];
  o.label_weight[i] = weight;
  const bool mine = lane < total;
  for (int k = 0; k < 4; ++k) o.ignore_boxes[i * 4 + k] = mine ? packed[lane * 4 + k] : 0.f;
  o.ignore_mask[i] = mine ? 1 : 0;
}

}  // namespace encode

extern "C" int mono_encode_targets_f64(const double *rows, const int *count, const double *records, const double *cls_mean_size,
                                       int writelist_mask, int depth_mode, int clip_2d, double min_score, int weight_mode, double weight,
                                       int res_w, int res_h, int B, int R, int C, int max_objs, void *const *outputs, void *stream_) {
  if (!rows || !count || !records || !cls_mean_size || !outputs) return -1;
  for (int k = 0; k < encode::kOutputs; ++k)
    if (!outputs[k]) return -1;
  if (B <= 0 || R <= 0 || C <= 0 || C > 31 || max_objs <= 0 || max_objs > encode::kLanes || res_w <= 0 || res_h <= 0 || depth_mode < 0 ||
      depth_mode > 2 || weight_mode < 0 || weight_mode > 1)
    return -2;
  encode::Settings s;
  s.writelist_mask = writelist_mask;
  s.depth_mode = depth_mode;
  s.clip_2d = clip_2d;
  s.weight_mode = weight_mode;
  s.min_score = min_score;
  s.weight = weight;
  s.res_w = res_w;
  s.res_h = res_h;
  s.R = R;
  s.C = C;
  s.max_objs = max_objs;
  encode::Outputs o;
  o.labels = (signed char *)outputs[0];
  o.boxes = (float *)outputs[1];
  o.boxes_3d = (float *)outputs[2];
  o.depth = (float *)outputs[3];
  o.size_2d = (float *)outputs[4];
  o.size_3d = (float *)outputs[5];
  o.src_size_3d = (float *)outputs[6];
  o.heading_bin = (long long *)outputs[7];
  o.heading_res = (float *)outputs[8];
  o.mask_2d = (unsigned char *)outputs[9];
  o.calibs = (float *)outputs[10];
  o.indices = (long long *)outputs[11];
  o.objects = (float *)outputs[12];
  o.label_weight = (float *)outputs[13];
  o.ignore_boxes = (float *)outputs[14];
  o.ignore_mask = (unsigned char *)outputs[15];
  o.n_ignore = (int *)outputs[16];
  encode::encode_targets_kernel<<<B, encode::kLanes, 0, (hipStream_t)stream_>>>(rows, count, records, cls_mean_size, s, o);
  return (int)hipGetLastError();
}
