/* monosowa_image.h -- C ABI of the image side of the KITTI loader (dataset.device_aug): what
 * KITTI_Dataset.__getitem__ does to a decoded image after the PNG decode -- photometric distortion, flip, PIL's affine
 * bilinear resampling to the network's resolution, normalisation, HWC -> CHW -- as ONE launch per batch, bit for bit equal
 * to the CPU path (monosowa_amd/kitti_dataset.py with Pillow's ImagingGenericTransform / bilinear filter and
 * monosowa_amd/photometric.py's float32 arithmetic).
 *
 * Device pointers, asynchronous on `stream`, no host synchronisation.
 * Return value: 0, -1 (NULL pointer), -2 (bad size: every extent >= 1, W a multiple of 4, `out` 16-byte aligned) or a hipError_t.
 *
 * One record of MONO_IMAGE_RECORD_DOUBLES float64 values per image (the float32 parameters are exact in float64):
 *   [0] w  [1] h          the image's true size inside the canvas (1 <= w <= Wc, 1 <= h <= Hc; the kernel clamps both)
 *   [2..7] a0..a5         output -> input affine coefficients, exactly as the CPU path hands them to Image.transform
 *   [8] flags             sum of MONO_IMAGE_* bits below
 *   [9] brightness  [10] contrast  [11] saturation  [12] hue      float32(draw) of each step that was taken
 *   [13] permutation      index 0..5 into ((0,1,2), (0,2,1), (1,0,2), (1,2,0), (2,0,1), (2,1,0))
 *   [14], [15]            reserved (0)
 */
#ifndef MONOSOWA_IMAGE_H
#define MONOSOWA_IMAGE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MONO_IMAGE_RECORD_DOUBLES 16
#define MONO_IMAGE_FLIP 1            /* horizontal flip before the resampling */
#define MONO_IMAGE_PD 2              /* photometric distortion on (the HSV round trip always runs then) */
#define MONO_IMAGE_BRIGHTNESS 4      /* += brightness */
#define MONO_IMAGE_CONTRAST_FIRST 8  /* contrast before the HSV steps (else after) */
#define MONO_IMAGE_CONTRAST 16       /* *= contrast */
#define MONO_IMAGE_SATURATION 32     /* S *= saturation */
#define MONO_IMAGE_HUE 64            /* H += hue, wrapped */
#define MONO_IMAGE_PERMUTE 128       /* channel permutation */

/* The record length this build reads (== MONO_IMAGE_RECORD_DOUBLES). */
int mono_image_record_doubles(void);

/* raw [B, Hc, Wc, 3] uint8 (each image in the top-left corner of its canvas; padding is never read), records
 * [B, MONO_IMAGE_RECORD_DOUBLES] float64, lut [256, 3] float32 (lut[u][c] = the normalised value of byte u in channel c)
 * -> out: float32 values of the logical [B, 3, H, W] batch in channels-last memory, i.e. out[((b * H + y) * W + x) * 3 + c]. */
int mono_image_prep_f32(const uint8_t *raw, const double *records, const float *lut, float *out, int B, int Hc, int Wc, int H,
                        int W, void *stream);

#ifdef __cplusplus
}
#endif
#endif
