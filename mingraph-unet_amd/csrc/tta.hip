// Test-time augmentation on the device: the flipped / rotated views of a batch and the merge of their softmaxes.
//   mgu_tta_views   a batch (fp32 images, any strides) -> the views of one shape group as one contiguous NCHW batch, view-major
//   mgu_tta_merge   the groups' NHWC logits -> mean of the K views' softmaxes mapped back to the input's pixels (NHWC probs), the
//                   first maximal class (int64) and its probability (fp32)
// A view is x, flipped (bit 0: torch.flip(x, (3,)), bit 1: torch.flip(x, (2,))), then turned r quarter turns (torch.rot90(x, r, (2, 3))).
// Quarter turns 1 and 3 swap H and W, so for H != W a view belongs to the (H, W) group (r even) or the (W, H) group (r odd); each group
// is one forward.  Both kernels are per-pixel gathers with the index arithmetic of mgunet.tta.view_source_index / view_inverse_index:
// the views kernel reads the source pixel of every view pixel, the merge kernel reads the view pixel of every output pixel.  Each
// output value depends on one pixel's C logits per view only: the result does not depend on the launch shape.  The views' fp32
// softmaxes are added in fp64, which has 29 bits to spare over a sum of 8 fp32 values, and the mean is rounded to fp32 once: equal
// softmaxes average to themselves for every K (a sequential fp32 sum of 8 times fl(1/3) is 1 ulp off 8 fl(1/3)), whatever the order.
#include <algorithm>

#include "ctx.h"

namespace mgu {
namespace {

constexpr int TTA_MAX_VIEWS = 8;
constexpr int TTA_MAX_C = 16;
constexpr int TTA_T = 16;   // 16 x 16 pixel tile per workgroup: a wave covers 4 rows x 16 columns, so a row-strided (quarter-turned)
                            // read still fills whole 128-byte lines across the workgroup's waves

struct TtaStrides {
  int64_t b, c, h, w;
};
// view v of the call: flip bits | quarter turns << 2 | slot << 4 | group << 8
struct TtaViews {
  int code[TTA_MAX_VIEWS];
};
struct TtaGroups {
  const float* p[2];
};

// (a, b) of the flipped H x W image -> view pixel (i, j) after r quarter turns (the inverse of torch.rot90(f, r, (0, 1)))
__device__ __forceinline__ void tta_to_view(int a, int b, int r, int H, int W, int* i, int* j) {
  switch (r) {
    case 0: *i = a, *j = b; break;
    case 1: *i = W - 1 - b, *j = a; break;
    case 2: *i = H - 1 - a, *j = W - 1 - b; break;
    default: *i = b, *j = H - 1 - a; break;
  }
}

// view pixel (i, j) -> source pixel (y, x) of the H x W image
__device__ __forceinline__ void tta_to_source(int i, int j, int flip, int r, int H, int W, int* y, int* x) {
  int a, b;
  switch (r) {
    case 0: a = i, b = j; break;
    case 1: a = j, b = W - 1 - i; break;
    case 2: a = H - 1 - i, b = W - 1 - j; break;
    default: a = H - 1 - j, b = i; break;
  }
  *y = (flip & 2) ? H - 1 - a : a;
  *x = (flip & 1) ? W - 1 - b : b;
}

// one thread per view pixel, every channel.  blockIdx.z = slot * B + b; out (G*B, C, Hg, Wg) contiguous.
__global__ __launch_bounds__(TTA_T * TTA_T) void tta_views_kernel(const float* __restrict__ in, TtaStrides s, int B, int C, int H, int W,
                                                                  TtaViews views, float* __restrict__ out) {
  const int z = blockIdx.z, slot = z / B, b = z - slot * B;
  const int code = views.code[slot], flip = code & 3, r = (code >> 2) & 3;
  const int Hg = (r & 1) ? W : H, Wg = (r & 1) ? H : W;
  const int j = blockIdx.x * TTA_T + (threadIdx.x & (TTA_T - 1)), i = blockIdx.y * TTA_T + (threadIdx.x / TTA_T);
  if (i >= Hg || j >= Wg) return;
  int y, x;
  tta_to_source(i, j, flip, r, H, W, &y, &x);
  const float* src = in + b * s.b + y * s.h + x * s.w;
  const int64_t plane = (int64_t)Hg * Wg;
  float* dst = out + (int64_t)z * C * plane + (int64_t)i * Wg + j;
  for (int c = 0; c < C; ++c) dst[c * plane] = src[c * s.c];
}

// one thread per output pixel: for each view (in order) the softmax of the mapped pixel's C logits (fp32, maximum subtracted, expf),
// summed in fp64, times 1/K (exact), rounded to fp32 once; then the first maximal class and its probability.  NC > 0: C == NC;
// NC == 0: C <= TTA_MAX_C at run time.
template <int NC>
__global__ __launch_bounds__(TTA_T * TTA_T) void tta_merge_kernel(TtaGroups g, int B, int Crt, int H, int W, int K, TtaViews views, double invK,
                                                                  float* __restrict__ probs, long long* __restrict__ labels,
                                                                  float* __restrict__ conf) {
  constexpr int CM = NC > 0 ? NC : TTA_MAX_C;
  const int C = NC > 0 ? NC : Crt;
  const int b = blockIdx.z;
  const int x = blockIdx.x * TTA_T + (threadIdx.x & (TTA_T - 1)), y = blockIdx.y * TTA_T + (threadIdx.x / TTA_T);
  if (y >= H || x >= W) return;
  double acc[CM];
#pragma unroll
  for (int c = 0; c < CM; ++c) acc[c] = 0.0;
  for (int v = 0; v < K; ++v) {
    const int code = views.code[v], flip = code & 3, r = (code >> 2) & 3, slot = (code >> 4) & 15, grp = code >> 8;
    const int Wg = (r & 1) ? H : W, Hg = (r & 1) ? W : H;
    const int a = (flip & 2) ? H - 1 - y : y, bb = (flip & 1) ? W - 1 - x : x;
    int i, j;
    tta_to_view(a, bb, r, H, W, &i, &j);
    const float* p = g.p[grp] + (((int64_t)(slot * B + b) * Hg + i) * Wg + j) * C;
    float e[CM];
    const float sum = pixel_softmax<CM>(p, C, e);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) acc[c] += (double)(e[c] / sum);
  }
  const int64_t pix = ((int64_t)b * H + y) * W + x;
  float best = 0.f;
  int bi = 0;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      const float q = (float)(acc[c] * invK);
      probs[pix * C + c] = q;
      if (c == 0 || q > best) best = q, bi = c;
    }
  labels[pix] = bi;
  conf[pix] = best;
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_tta_views(mgu_ctx* c, const float* img_dev, int B, int C, int H, int W, const int64_t* in_strides, int G, const int32_t* views,
                  float* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_dev || !out_dev || !in_strides || !views || B < 1 || C < 1 || H < 1 || W < 1 || G < 1 || G > TTA_MAX_VIEWS)
    return fail(c, MGU_ERR_INVALID, "bad tta_views args (null pointer, B, C, H, W < 1 or G outside [1, %d])", TTA_MAX_VIEWS);
  if ((int64_t)G * B > 65535) return fail(c, MGU_ERR_INVALID, "tta_views: at most 65535 view images per call");
  TtaViews v{};
  for (int k = 0; k < G; ++k) {
    const int flip = views[2 * k], r = views[2 * k + 1];
    if (flip < 0 || flip > 3 || r < 0 || r > 3) return fail(c, MGU_ERR_INVALID, "tta_views: view %d has flip %d, turns %d", k, flip, r);
    if (H != W && (r & 1) != (views[1] & 1)) return fail(c, MGU_ERR_INVALID, "tta_views: the views of one call must share their shape");
    v.code[k] = flip | r << 2;
  }
  const int Hg = (views[1] & 1) ? W : H, Wg = (views[1] & 1) ? H : W;
  HIPCHK(c, hipSetDevice(c->device));
  const TtaStrides s{in_strides[0], in_strides[1], in_strides[2], in_strides[3]};
  const dim3 grid((Wg + TTA_T - 1) / TTA_T, (Hg + TTA_T - 1) / TTA_T, G * B);
  hipLaunchKernelGGL(tta_views_kernel, grid, dim3(TTA_T * TTA_T), 0, (hipStream_t)hip_stream, img_dev, s, B, C, H, W, v, out_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_tta_merge(mgu_ctx* c, const float* logits0_dev, const float* logits1_dev, int B, int C, int H, int W, int K, const int32_t* views,
                  float* probs_dev, int64_t* labels_dev, float* conf_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!logits0_dev || !views || !probs_dev || !labels_dev || !conf_dev || B < 1 || H < 1 || W < 1 || B > 65535)
    return fail(c, MGU_ERR_INVALID, "bad tta_merge args (null pointer, B outside [1, 65535] or H, W < 1)");
  if (C < 1 || C > TTA_MAX_C) return fail(c, MGU_ERR_INVALID, "tta_merge: %d classes (at most %d)", C, TTA_MAX_C);
  if (K != 1 && K != 2 && K != 4 && K != 8) return fail(c, MGU_ERR_INVALID, "tta_merge: %d views (1, 2, 4 or 8)", K);
  TtaViews v{};
  int slots[2] = {0, 0};
  for (int k = 0; k < K; ++k) {
    const int grp = views[4 * k], slot = views[4 * k + 1], flip = views[4 * k + 2], r = views[4 * k + 3];
    if (grp < 0 || grp > 1 || slot < 0 || slot >= TTA_MAX_VIEWS || flip < 0 || flip > 3 || r < 0 || r > 3)
      return fail(c, MGU_ERR_INVALID, "tta_merge: view %d is (group %d, slot %d, flip %d, turns %d)", k, grp, slot, flip, r);
    if (grp != (H != W ? (r & 1) : 0)) return fail(c, MGU_ERR_INVALID, "tta_merge: view %d is in the wrong shape group", k);
    slots[grp] = std::max(slots[grp], slot + 1);
    v.code[k] = flip | r << 2 | slot << 4 | grp << 8;
  }
  if (slots[1] && !logits1_dev) return fail(c, MGU_ERR_INVALID, "tta_merge: group 1 has views but no logits");
  HIPCHK(c, hipSetDevice(c->device));
  const TtaGroups g{{logits0_dev, logits1_dev}};
  const dim3 grid((W + TTA_T - 1) / TTA_T, (H + TTA_T - 1) / TTA_T, B);
  hipStream_t s = (hipStream_t)hip_stream;
  long long* lab = (long long*)labels_dev;
  const double invK = 1.0 / (double)K;
  switch (C) {
    case 1: hipLaunchKernelGGL(tta_merge_kernel<1>, grid, dim3(TTA_T * TTA_T), 0, s, g, B, C, H, W, K, v, invK, probs_dev, lab, conf_dev); break;
    case 2: hipLaunchKernelGGL(tta_merge_kernel<2>, grid, dim3(TTA_T * TTA_T), 0, s, g, B, C, H, W, K, v, invK, probs_dev, lab, conf_dev); break;
    case 3: hipLaunchKernelGGL(tta_merge_kernel<3>, grid, dim3(TTA_T * TTA_T), 0, s, g, B, C, H, W, K, v, invK, probs_dev, lab, conf_dev); break;
    case 4: hipLaunchKernelGGL(tta_merge_kernel<4>, grid, dim3(TTA_T * TTA_T), 0, s, g, B, C, H, W, K, v, invK, probs_dev, lab, conf_dev); break;
    default: hipLaunchKernelGGL(tta_merge_kernel<0>, grid, dim3(TTA_T * TTA_T), 0, s, g, B, C, H, W, K, v, invK, probs_dev, lab, conf_dev); break;
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
