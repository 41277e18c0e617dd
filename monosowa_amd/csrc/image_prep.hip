// image_prep.hip -- the pixel side of KITTI_Dataset.__getitem__ as one launch per batch (include/monosowa_image.h;
// SURVEY 8 row f4, dataset.device_aug): photometric distortion of the source taps, flip, PIL's affine bilinear resampling,
// normalisation and HWC -> channels-last CHW, bit for bit equal to the CPU path.
//
// Exactness rests on the build and on the order of operations, not on tolerances:
//   * compiled with -ffp-contract=off (monosowa_amd/build.py): `(g - b) * k + 120`, `v * (1 - s * f)` and the coordinate sums
//     are a rounded product followed by a rounded sum on the CPU, never an FMA;
//   * float32 division is hipcc's default correctly rounded one (no fast-math); the one float64 division of RGB2HSV_f
//     (`(float)(60. / (double)(diff + eps))`) is done in float64;
//   * coordinates in float64 with floor() (PIL's affine_transform + bilinear_filter32RGB), result truncated like `(UINT8) v`;
//   * numpy's astype(uint8) of a float32 is truncation toward zero, then the low eight bits (values wrap, they do not saturate).
//
// Streaming kernel: a lane owns four neighbouring output pixels of one row = 12 floats = three 16-byte stores; the taps of
// each pixel are distorted on the fly (four taps per pixel, no scratch image, one launch: DESIGN.md section 5).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/monosowa_image.h"

namespace imgprep {

constexpr int kThreads = 256;
constexpr int kRec = MONO_IMAGE_RECORD_DOUBLES;
constexpr float kEps = 1.1920929e-07f;                   // FLT_EPSILON
constexpr float kHueScale = (float)(6.0 / 360.0);       // np.float32(6.0 / 360.0)

struct Photo {
  unsigned flags;
  float brightness, contrast, saturation, hue;
  int perm;
};

struct Tap {
  int c[3];
};

__device__ __forceinline__ int wrap_u8(float x) { return ((int)x) & 255; }      // astype(np.uint8): truncate, low byte

// monosowa_amd/photometric.py PhotometricDistort.apply on one pixel, then the wrapping uint8 cast.
__device__ __forceinline__ Tap distort(const uint8_t *px, const Photo &P) {
  Tap o;
  if (!(P.flags & MONO_IMAGE_PD)) {
    o.c[0] = px[0]; o.c[1] = px[1]; o.c[2] = px[2];
    return o;
  }
  float b = (float)px[0], g = (float)px[1], r = (float)px[2];       // the reference's channel names: (B, G, R) = channels 0, 1, 2
  if (P.flags & MONO_IMAGE_BRIGHTNESS) { b += P.brightness; g += P.brightness; r += P.brightness; }
  const bool contrast = (P.flags & MONO_IMAGE_CONTRAST) != 0, first = (P.flags & MONO_IMAGE_CONTRAST_FIRST) != 0;
  if (contrast && first) { b *= P.contrast; g *= P.contrast; r *= P.contrast; }
  // bgr_to_hsv (OpenCV's RGB2HSV_f)
  float v = fmaxf(fmaxf(b, g), r);
  const float diff = v - fminf(fminf(b, g), r);
  float s = diff / (fabsf(v) + kEps);
  const float k = (float)(60.0 / (double)(diff + kEps));
  float h;
  if (v == r) h = (g - b) * k;
  else if (v == g) h = (b - r) * k + 120.0f;
  else h = (r - g) * k + 240.0f;
  if (h < 0.0f) h += 360.0f;
  if (P.flags & MONO_IMAGE_SATURATION) s *= P.saturation;
  if (P.flags & MONO_IMAGE_HUE) {
    h += P.hue;
    if (h > 360.0f) h -= 360.0f;
    if (h < 0.0f) h += 360.0f;
  }
  // hsv_to_bgr (OpenCV's HSV2RGB_f, 360-degree hue)
  float hh = h * kHueScale;
  hh = hh - 6.0f * floorf(hh / 6.0f);
  if (hh >= 6.0f) hh -= 6.0f;
  const float sector_f = floorf(hh);
  const float f = hh - sector_f;
  int sector = ((int)sector_f) % 6;
  if (sector < 0) sector += 6;
  const float p = v * (1.0f - s);
  const float q = v * (1.0f - s * f);
  const float t = v * (1.0f - s * (1.0f - f));
  switch (sector) {
    case 0: r = v; g = t; b = p; break;
    case 1: r = q; g = v; b = p; break;
    case 2: r = p; g = v; b = t; break;
    case 3: r = p; g = q; b = v; break;
    case 4: r = t; g = p; b = v; break;
    default: r = v; g = p; b = q; break;
  }
  if (contrast && !first) { b *= P.contrast; g *= P.contrast; r *= P.contrast; }
  const int u0 = wrap_u8(b), u1 = wrap_u8(g), u2 = wrap_u8(r);
  if (P.flags & MONO_IMAGE_PERMUTE) {
    switch (P.perm) {
      case 1: o.c[0] = u0; o.c[1] = u2; o.c[2] = u1; break;
      case 2: o.c[0] = u1; o.c[1] = u0; o.c[2] = u2; break;
      case 3: o.c[0] = u1; o.c[1] = u2; o.c[2] = u0; break;
      case 4: o.c[0] = u2; o.c[1] = u0; o.c[2] = u1; break;
      case 5: o.c[0] = u2; o.c[1] = u1; o.c[2] = u0; break;
      default: o.c[0] = u0; o.c[1] = u1; o.c[2] = u2; break;
    }
  } else {
    o.c[0] = u0; o.c[1] = u1; o.c[2] = u2;
  }
  return o;
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kThreads) void image_prep_kernel(const uint8_t *__restrict__ raw, const double *__restrict__ records,
                                                              const float *__restrict__ lut, float *__restrict__ out,
                                                              long long total, int Hc, int Wc, int H, int W) {
  const long long idx = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (idx >= total) return;
  const int W4 = W >> 2;
  const int xq = (int)(idx % W4);
  const long long row_id = idx / W4;
  const int y = (int)(row_id % H);
  const int b = (int)(row_id / H);

  const double *R = records + (long long)b * kRec;
  const int w = clampi((int)R[0], 1, Wc), h = clampi((int)R[1], 1, Hc);       // clamped: no record can steer a read outside the canvas
  const double a0 = R[2], a1 = R[3], a2 = R[4], a3 = R[5], a4 = R[6], a5 = R[7];
  Photo P;
  P.flags = (unsigned)(int)R[8];
  P.brightness = (float)R[9];
  P.contrast = (float)R[10];
  P.saturation = (float)R[11];
  P.hue = (float)R[12];
  P.perm = (int)R[13];
  const bool flip = (P.flags & MONO_IMAGE_FLIP) != 0;
  const uint8_t *src = raw + (size_t)b * Hc * Wc * 3;

  float o[12];
  const double Y = (double)y + 0.5;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double X = (double)(xq * 4 + j) + 0.5;
    double xin = a0 * X + a1 * Y + a2;
    double yin = a3 * X + a4 * Y + a5;
    int u[3] = {0, 0, 0};                                                      // PIL's fill
    if (!(xin < 0.0 || xin >= (double)w || yin < 0.0 || yin >= (double)h)) {
      xin -= 0.5;
      yin -= 0.5;
      const double xf = floor(xin), yf = floor(yin);
      const double dx = xin - xf, dy = yin - yf;
      const int x0 = (int)xf, y0 = (int)yf;
      int c0 = clampi(x0, 0, w - 1), c1 = clampi(x0 + 1, 0, w - 1);
      if (flip) { c0 = w - 1 - c0; c1 = w - 1 - c1; }                          // PIL flips first: column c of the flipped image
      const size_t r0 = (size_t)clampi(y0, 0, h - 1) * Wc;
      const Tap ta = distort(src + (r0 + c0) * 3, P), tb = distort(src + (r0 + c1) * 3, P);
      double v1[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double a = (double)ta.c[c], bb = (double)tb.c[c];
        v1[c] = a + (bb - a) * dx;
      }
      if (y0 + 1 >= 0 && y0 + 1 < h) {
        const size_t r1 = (size_t)(y0 + 1) * Wc;
        const Tap tc = distort(src + (r1 + c0) * 3, P), td = distort(src + (r1 + c1) * 3, P);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double a = (double)tc.c[c], bb = (double)td.c[c];
          const double v2 = a + (bb - a) * dx;
          u[c] = (int)(v1[c] + (v2 - v1[c]) * dy);                             // (UINT8) v: truncated, not rounded
        }
      } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) u[c] = (int)v1[c];                              // no row below: v2 = v1, v = v1 + 0 * dy
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) o[j * 3 + c] = lut[(u[c] & 255) * 3 + c];
  }
  float4 *dst = reinterpret_cast<float4 *>(out + (idx * 4) * 3);               // idx * 4 = (b * H + y) * W + x
  dst[0] = make_float4(o[0], o[1], o[2], o[3]);
  dst[1] = make_float4(o[4], o[5], o[6], o[7]);
  dst[2] = make_float4(o[8], o[9], o[10], o[11]);
}

}  // namespace imgprep

extern "C" {

int mono_image_record_doubles(void) { return imgprep::kRec; }

int mono_image_prep_f32(const uint8_t *raw, const double *records, const float *lut, float *out, int B, int Hc, int Wc, int H,
                        int W, void *stream_) {
  if (!raw || !records || !lut || !out) return -1;
  if (B <= 0 || Hc <= 0 || Wc <= 0 || H <= 0 || W <= 0 || (W & 3) || ((uintptr_t)out & 15)) return -2;
  const long long total = (long long)B * H * (W >> 2);
  const long long blocks = (total + imgprep::kThreads - 1) / imgprep::kThreads;
  if (blocks > 0x7fffffffLL) return -2;
  imgprep::image_prep_kernel<<<(unsigned)blocks, imgprep::kThreads, 0, (hipStream_t)stream_>>>(raw, records, lut, out, total, Hc, Wc,
                                                                                              H, W);
  return (int)hipGetLastError();
}

}  // extern "C"
