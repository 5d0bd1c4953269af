// Internal: the cv2 byte arithmetic shared by imageops.hip (one image, full maps) and patch_inputs.hip (a batch, per-patch sums only).
// One definition of each expression, so the two paths agree bit for bit: OpenCV's fixed-point grey / YUV conversions, reflect-101
// borders, the Sobel normalisation, cv::equalizeHist's table rule.
#pragma once
#include <math.h>
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace mgu {

// cv2.COLOR_RGB2GRAY on 8-bit data: OpenCV 3.4 / 4.x use 15-bit coefficients (RY15 9798, GY15 19235, BY15 3735, gray_shift 15); only
// the YUV / YCrCb conversions below keep the 14-bit ones (yuv_shift 14)
__device__ __forceinline__ int cv_gray(const uint8_t* p) { return (p[0] * 9798 + p[1] * 19235 + p[2] * 3735 + (1 << 14)) >> 15; }
__device__ __forceinline__ int reflect101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }
// reflect-101 applied until the index lies inside [0, n): a kernel radius may exceed the image side (radius 15 on a 2-pixel row); n == 1 -> 0
__device__ __forceinline__ int reflect101_loop(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
  return i;
}
// squared 3x3 Sobel magnitude gx^2 + gy^2 of the grey neighbourhood g[dy][dx] (exact integers)
__device__ __forceinline__ int sobel_mag2(const int (&g)[3][3]) {
  const int gx = (g[0][2] + 2 * g[1][2] + g[2][2]) - (g[0][0] + 2 * g[1][0] + g[2][0]);
  const int gy = (g[2][0] + 2 * g[2][1] + g[2][2]) - (g[0][0] + 2 * g[0][1] + g[0][2]);
  return gx * gx + gy * gy;
}
// (e / max * 255).astype(uint8) of edge_detection.py:41-44: truncation; mx = sqrt(the image's largest squared magnitude)
__device__ __forceinline__ uint8_t sobel_norm_u8(int m, double mx) { return mx > 0.0 ? (uint8_t)(sqrt((double)m) / mx * 255.0) : (uint8_t)0; }

__device__ __forceinline__ int cv_descale14(int v) { return (v + (1 << 13)) >> 14; }
__device__ __forceinline__ int sat8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ void cv_rgb2yuv(const uint8_t* p, int& Y, int& U, int& V) {
  Y = cv_descale14(p[0] * 4899 + p[1] * 9617 + p[2] * 1868);
  U = sat8(cv_descale14((p[2] - Y) * 8061 + (128 << 14)));    // B2UF = 0.492
  V = sat8(cv_descale14((p[0] - Y) * 14369 + (128 << 14)));   // R2VF = 0.877
}
__device__ __forceinline__ void cv_yuv2rgb(int Y, int U, int V, int& r, int& g, int& b) {
  const int u = U - 128, v = V - 128;
  r = sat8(Y + cv_descale14(v * 18678));                  // V2RI = 1.140
  g = sat8(Y + cv_descale14(u * -6472 + v * -9519));      // U2GI = -0.395, V2GI = -0.581
  b = sat8(Y + cv_descale14(u * 33292));                  // U2BI = 2.032
}
// cv::equalizeHist: first non-empty bin i0; scale = 255 / (total - hist[i0]); lut[i] = saturate(round(cumsum_{i0 < j <= i} * scale)).
// Serial: one thread per table.
__device__ __forceinline__ void equalize_lut_build(const unsigned* __restrict__ hist, int64_t total, uint8_t* __restrict__ lut) {
  int i0 = 0;
  while (i0 < 256 && !hist[i0]) ++i0;
  if (i0 == 256 || hist[i0] == total) {
    for (int i = 0; i < 256; ++i) lut[i] = (uint8_t)(i0 < 256 ? i0 : i);   // a constant image maps to itself
    return;
  }
  const float scale = 255.f / (float)(total - hist[i0]);
  int sum = 0;
  for (int i = 0; i < 256; ++i) {
    if (i <= i0) {
      lut[i] = 0;
      continue;
    }
    sum += hist[i];
    lut[i] = (uint8_t)sat8((int)rintf((float)sum * scale));
  }
}

}  // namespace mgu
