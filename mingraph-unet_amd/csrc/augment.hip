// Training augmentation of ImagePreprocessor(apply_augmentation=True) (preprocessing/image_preprocessing/image_preprocess.py:34-51):
// RandomHorizontalFlip(p) then RandomRotation(degrees) on the resized PIL image, i.e. img.transpose(FLIP_LEFT_RIGHT) (when drawn) then
// img.rotate(angle, NEAREST, expand=False, center=None, fillcolor=0).
//   mgu_augment_flip_rotate        a device batch (fp32 images, any strides, + optional int64 masks), one launch, per-image parameters
//   mgu_preprocess_image_u8_aug    ImagePreprocessor.preprocess with the augmentation fused into the ToTensor + Normalize pass
//   mgu_preprocess_mask_u8_aug     preprocess_mask (nearest resize + clip) followed by the same flip / rotation, one launch
// PIL rotates with NEAREST through its 16.16 fixed-point affine path (affine_fixed, libImaging/Geometry.c): output pixel (x, y) reads
// source pixel (xin, yin) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) when it lies inside the image, else keeps the fill.
// The six int32 coefficients come from the host (mgunet.preprocess.pil_rotation_fixed).  Integer sums are associative, so each output
// pixel is computed on its own and the gather is bit-exact.  Nearest resampling only copies values, so rotating the normalised fp32
// image with fill (0/255 - mean)/std equals rotating the uint8 image and normalising afterwards.  PIL takes the fixed-point path for
// every rotation of an image up to 8192 pixels a side (all coordinates stay below 32768); larger images are refused.
#include <algorithm>

#include "ctx.h"

namespace mgu {

// imageops.hip: the PIL BILINEAR resize half of mgu_preprocess_image_u8 (result (H, W, channels) uint8)
int preprocess_resize_u8(mgu_ctx* c, const uint8_t* img_dev, int Hs, int Ws, int channels, int H, int W, hipStream_t s, const uint8_t** out);

constexpr int AUG_MAX_SIDE = 8192;
constexpr int AUG_MAX_C = 16;
constexpr int AUG_XV = 4;   // consecutive output x per thread (one 16-byte store per channel on the vector path)
constexpr int AUG_TX = 32, AUG_TY = 32;   // workgroup tile: 8 threads x 4 pixels across, 32 rows (256 threads)

struct AugRot {
  int flip, a0, a1, a2, a3, a4, a5;
};
struct AugStrides {
  int64_t b, c, h, w;
};
struct AugFill {
  float v[AUG_MAX_C];
};

// Source pixel (*xs, *ys) of output (x, y) of a W x H image; false when it lies outside the image.  32-bit wrap-around sums: identical to PIL's incremental
// int additions (which never overflow at these sizes); the shift is arithmetic, i.e. floor.
__device__ __forceinline__ bool aug_src(int a0, int a1, int a2, int a3, int a4, int a5, int flip, int x, int y, int W, int H, int* xs, int* ys) {
  const int xin = (int)((unsigned)a2 + (unsigned)y * (unsigned)a1 + (unsigned)x * (unsigned)a0) >> 16;
  const int yin = (int)((unsigned)a5 + (unsigned)y * (unsigned)a4 + (unsigned)x * (unsigned)a3) >> 16;
  *xs = flip ? W - 1 - xin : xin;   // hflip first, then rotate: the flipped image's column xin is the source's W-1-xin
  *ys = yin;
  return (unsigned)xin < (unsigned)W && (unsigned)yin < (unsigned)H;
}

// One thread: AUG_XV consecutive x of one output row of one image, every channel, and the mask label.  A workgroup covers a tile of
// AUG_TY rows x AUG_TX pixels, each wave 8 rows x 32 pixels: near-square, so the rotated source footprint of one wave instruction spans
// few source rows (a 256-pixel strip of one row would cross ~70 source rows at 15 degrees).  params: (B, 7) int32 {flip, a0..a5}.
// VEC: output x-stride 1 and every row / channel / image start 16-byte aligned (W % 4 == 0); mask rows then too.
template <bool VEC>
__global__ __launch_bounds__(256) void flip_rotate_nearest_kernel(const float* __restrict__ in, float* __restrict__ out, int B, int Cc, int H,
                                                                  int W, AugStrides si, AugStrides so, AugFill fill,
                                                                  const int64_t* __restrict__ mask_in, int64_t* __restrict__ mask_out,
                                                                  int64_t mask_fill, const int* __restrict__ params) {
  const unsigned tiles_x = (unsigned)((W + AUG_TX - 1) / AUG_TX), tiles_y = (unsigned)((H + AUG_TY - 1) / AUG_TY);
  const unsigned total = (unsigned)B * tiles_y * tiles_x;   // < 2^31 (checked on the host)
  const int lx = (int)(threadIdx.x % (AUG_TX / AUG_XV)) * AUG_XV, ly = (int)(threadIdx.x / (AUG_TX / AUG_XV));
  for (unsigned t = blockIdx.x; t < total; t += gridDim.x) {
    const int x0 = (int)(t % tiles_x) * AUG_TX + lx;
    const unsigned r = t / tiles_x;
    const int y = (int)(r % tiles_y) * AUG_TY + ly, b = (int)(r / tiles_y);
    if (y >= H || x0 >= W) continue;
    const int* p = params + 7 * b;
    const int flip = p[0], a0 = p[1], a1 = p[2], a2 = p[3], a3 = p[4], a4 = p[5], a5 = p[6];
    int64_t src[AUG_XV];   // element offset of the source pixel (channel 0) in the image, or -1 (fill)
    int msrc[AUG_XV];      // y * W + x of the source pixel in the mask
#pragma unroll
    for (int k = 0; k < AUG_XV; ++k) {
      int xs, ys;
      const bool ok = x0 + k < W && aug_src(a0, a1, a2, a3, a4, a5, flip, x0 + k, y, W, H, &xs, &ys);
      src[k] = ok ? b * si.b + ys * si.h + xs * si.w : -1;
      msrc[k] = ok ? ys * W + xs : -1;
    }
    const int64_t obase = b * so.b + y * so.h;
    for (int c = 0; c < Cc; ++c) {
      float v[AUG_XV];
      const float f = fill.v[c];
#pragma unroll
      for (int k = 0; k < AUG_XV; ++k) v[k] = src[k] >= 0 ? in[src[k] + c * si.c] : f;
      float* o = out + obase + c * so.c;
      if (VEC) {
        *(float4*)(o + x0) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
#pragma unroll
        for (int k = 0; k < AUG_XV; ++k)
          if (x0 + k < W) o[(x0 + k) * so.w] = v[k];
      }
    }
    if (mask_out) {
      const int64_t* mi = mask_in + (int64_t)b * H * W;
      int64_t* mo = mask_out + (int64_t)b * H * W + (int64_t)y * W + x0;
      int64_t m[AUG_XV];
#pragma unroll
      for (int k = 0; k < AUG_XV; ++k) m[k] = msrc[k] >= 0 ? mi[msrc[k]] : mask_fill;
      if (VEC) {
        ((longlong2*)mo)[0] = make_longlong2(m[0], m[1]);
        ((longlong2*)mo)[1] = make_longlong2(m[2], m[3]);
      } else {
#pragma unroll
        for (int k = 0; k < AUG_XV; ++k)
          if (x0 + k < W) mo[k] = m[k];
      }
    }
  }
}

// to_tensor_normalize_kernel (imageops.hip) reading the resized (H, W, Cin) uint8 image through the flip / rotation: a pixel outside
// the image reads the fill 0, so it becomes (0/255 - mean)/std by the same float operations.
__global__ __launch_bounds__(256) void to_tensor_normalize_aug_kernel(const uint8_t* __restrict__ in, int H, int W, int Cin, int bgr,
                                                                      float m0, float m1, float m2, float s0, float s1, float s2, AugRot rot,
                                                                      float* __restrict__ out, int64_t os_c, int64_t os_h, int64_t os_w) {
  const int64_t total = (int64_t)H * W * 3;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % 3);
    const int64_t pix = i / 3;
    const int x = (int)(pix % W), y = (int)(pix / W);
    int xs, ys;
    const bool ok = aug_src(rot.a0, rot.a1, rot.a2, rot.a3, rot.a4, rot.a5, rot.flip, x, y, W, H, &xs, &ys);
    const int sc = Cin == 1 ? 0 : (bgr ? 2 - c : c);
    const uint8_t u = ok ? in[((int64_t)ys * W + xs) * Cin + sc] : (uint8_t)0;
    out[c * os_c + y * os_h + x * os_w] = u8_normalize(u, c, m0, m1, m2, s0, s1, s2);
  }
}

// mask_nearest_kernel (imageops.hip: cv2 INTER_NEAREST to (H, W), clip) followed by the flip / rotation; outside pixels get mask_fill
// (not clipped: e.g. the ignore_index -100)
__global__ __launch_bounds__(256) void mask_nearest_aug_kernel(const uint8_t* __restrict__ in, int Hs, int Ws, int64_t* __restrict__ out, int H,
                                                               int W, int num_classes, AugRot rot, int64_t mask_fill) {
  const double ify = 1.0 / ((double)H / (double)Hs), ifx = 1.0 / ((double)W / (double)Ws);
  const int64_t total = (int64_t)H * W;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % W), y = (int)(i / W);
    int xs, ys;
    int64_t r = mask_fill;
    if (aug_src(rot.a0, rot.a1, rot.a2, rot.a3, rot.a4, rot.a5, rot.flip, x, y, W, H, &xs, &ys)) {
      const int sy = min((int)floor(ys * ify), Hs - 1), sx = min((int)floor(xs * ifx), Ws - 1);
      const int v = in[(size_t)sy * Ws + sx];
      r = (int64_t)min(max(v, 0), num_classes - 1);
    }
    out[i] = r;
  }
}

}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {
inline AugRot make_rot(int flip, const int32_t* fix) { return AugRot{flip ? 1 : 0, fix[0], fix[1], fix[2], fix[3], fix[4], fix[5]}; }
}  // namespace

extern "C" {

int mgu_augment_flip_rotate(mgu_ctx* c, const float* img_in, float* img_out, int B, int C, int H, int W, const int64_t* in_strides,
                            const int64_t* out_strides, const float* fill_c, const int64_t* mask_in, int64_t* mask_out, int64_t mask_fill,
                            const int32_t* params_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_in || !img_out || !in_strides || !out_strides || !fill_c || !params_dev || B < 1 || C < 1 || C > AUG_MAX_C || H < 1 || W < 1)
    return fail(c, MGU_ERR_INVALID, "bad augment_flip_rotate args (null pointer, B < 1, C outside [1, %d] or H, W < 1)", AUG_MAX_C);
  if (H > AUG_MAX_SIDE || W > AUG_MAX_SIDE)
    return fail(c, MGU_ERR_INVALID, "augment_flip_rotate: %d x %d is above %d pixels a side (PIL's float64 path, not reproduced)", H, W,
                AUG_MAX_SIDE);
  if (!mask_in != !mask_out) return fail(c, MGU_ERR_INVALID, "augment_flip_rotate: mask_in and mask_out go together");
  if ((const void*)img_in == (const void*)img_out || (mask_in && mask_in == mask_out))
    return fail(c, MGU_ERR_INVALID, "augment_flip_rotate is out of place");
  const int64_t tiles = (int64_t)B * ((H + AUG_TY - 1) / AUG_TY) * ((W + AUG_TX - 1) / AUG_TX);
  if (tiles >= ((int64_t)1 << 31)) return fail(c, MGU_ERR_INVALID, "augment_flip_rotate: batch too large for one launch");
  const int grid = (int)std::min<int64_t>(tiles, 256 * 16);
  HIPCHK(c, hipSetDevice(c->device));
  const AugStrides si{in_strides[0], in_strides[1], in_strides[2], in_strides[3]};
  const AugStrides so{out_strides[0], out_strides[1], out_strides[2], out_strides[3]};
  AugFill fill{};
  for (int i = 0; i < C; ++i) fill.v[i] = fill_c[i];
  const bool vec = so.w == 1 && W % 4 == 0 && so.h % 4 == 0 && so.c % 4 == 0 && so.b % 4 == 0 && aligned16(img_out) && (!mask_out || aligned16(mask_out));
  hipStream_t s = (hipStream_t)hip_stream;
  if (vec)
    hipLaunchKernelGGL(flip_rotate_nearest_kernel<true>, dim3(grid), dim3(256), 0, s, img_in, img_out, B, C, H, W, si, so, fill, mask_in,
                       mask_out, mask_fill, (const int*)params_dev);
  else
    hipLaunchKernelGGL(flip_rotate_nearest_kernel<false>, dim3(grid), dim3(256), 0, s, img_in, img_out, B, C, H, W, si, so, fill, mask_in,
                       mask_out, mask_fill, (const int*)params_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_preprocess_image_u8_aug(mgu_ctx* c, const uint8_t* img_dev, int Hs, int Ws, int channels, int bgr, int H, int W, const float* mean3,
                                const float* std3, void* out_dev, int64_t os_c, int64_t os_h, int64_t os_w, int flip, const int32_t* fix6,
                                void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_dev || !out_dev || !mean3 || !std3 || !fix6 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || (channels != 1 && channels != 3))
    return fail(c, MGU_ERR_INVALID, "bad preprocess_image_aug args (null pointer, sizes < 1, or not 1 or 3 channels)");
  if (H > AUG_MAX_SIDE || W > AUG_MAX_SIDE)
    return fail(c, MGU_ERR_INVALID, "preprocess_image_aug: %d x %d is above %d pixels a side (PIL's float64 path, not reproduced)", H, W,
                AUG_MAX_SIDE);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const uint8_t* cur = nullptr;
  int rc = preprocess_resize_u8(c, img_dev, Hs, Ws, channels, H, W, s, &cur);
  if (rc) return rc;
  hipLaunchKernelGGL(to_tensor_normalize_aug_kernel, dim3(grid_for((int64_t)H * W * 3, 256, 256 * 8)), dim3(256), 0, s, cur, H, W, channels, bgr, mean3[0], mean3[1],
                     mean3[2], std3[0], std3[1], std3[2], make_rot(flip, fix6), (float*)out_dev, os_c, os_h, os_w);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_preprocess_mask_u8_aug(mgu_ctx* c, const uint8_t* mask_dev, int Hs, int Ws, int H, int W, int num_classes, int flip, const int32_t* fix6,
                               int64_t mask_fill, int64_t* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!mask_dev || !out_dev || !fix6 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || num_classes < 1)
    return fail(c, MGU_ERR_INVALID, "bad preprocess_mask_aug args");
  if (H > AUG_MAX_SIDE || W > AUG_MAX_SIDE)
    return fail(c, MGU_ERR_INVALID, "preprocess_mask_aug: %d x %d is above %d pixels a side (PIL's float64 path, not reproduced)", H, W,
                AUG_MAX_SIDE);
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(mask_nearest_aug_kernel, dim3(grid_for((int64_t)H * W, 256, 256 * 8)), dim3(256), 0, (hipStream_t)hip_stream, mask_dev, Hs, Ws, out_dev, H, W,
                     num_classes, make_rot(flip, fix6), mask_fill);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
