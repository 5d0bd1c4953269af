// Helpers shared by the segmentation-loss kernel files (losses.hip: dice; lovasz.hip; pixel_ce.hip): each is defined here and nowhere
// else under csrc/ (tests/test_csrc_helpers.py).  device.h keeps what every kernel file shares, PixelCE among it.
//   device: softmax_front (NoClassHook) | LossCall | LossTile, loss_tile, loss_item (LOSS_ITEMS, LOSS_TILE) | up_scale
//   host:   LossGrad | loss_call | with_nc, with_flag (int_c)
// seg_eval.hip and train_kernels.hip keep their own softmax (0.f padding, a runtime class count: the benchmarked step).
#pragma once
#include <type_traits>

#include "ctx.h"

namespace mgu {

// ---- the per-pixel softmax front end ------------------------------------------------------------------------------------------------
// The C <= NC logits of one pixel at p, class stride ls_c: mx = their maximum (fmaxf in class order from -inf), e[c] = expf(l_c - mx)
// (a padded class: 0.f), returns the sum of e in class order from 0.f; l, when given, gets the logits themselves (padded: -inf), and
// each(c, e[c]) is called in class order as every e[c] is formed (pc_pixel feeds PixelCE::add there: gathered into a loop of its own
// after the exponentials, the same statements cost hazard no-ops and 0.3 - 0.8 % of a call).  Every loss kernel forms its softmax through
// here, so all of them see the same bits.  Some callers run under `#pragma clang fp contract(off)`, which is lexical and does not reach
// in here: this function carries none because it has no multiply that feeds an add.  What does (e * inv into a sum, products of
// gradients) stays in the callers, under their own pragma, and so does the body of a hook, which is written there.
struct NoClassHook {
  __device__ __forceinline__ void operator()(int, float) const {}
};
template <int NC, typename F = NoClassHook>
__device__ __forceinline__ float softmax_front(const float* __restrict__ p, int64_t ls_c, int C, float (&e)[NC], float& mx,
                                               float (*l)[NC] = nullptr, F each = F()) {
  mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    e[c] = c < C ? p[c * ls_c] : -INFINITY;
    if (l) (*l)[c] = e[c];
    mx = fmaxf(mx, e[c]);
  }
  float se = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    e[c] = c < C ? expf(e[c] - mx) : 0.f;
    se += e[c];
    each(c, e[c]);
  }
  return se;
}

// ---- the call and its tiles -----------------------------------------------------------------------------------------------------------
// what every kernel knows of the call: the logits and labels, and how the P = B * HW pixels fall into G groups of Ng consecutive pixels
// (the batch, or one image each) of tiles_g tiles.  A kernel argument by value: it and what derives from it stay trivially copyable.
struct LossCall {
  const float* logits;
  const int64_t* labels;
  int64_t ls_n, ls_c, ls_p;
  long long ignore;
  int HW, C, P, G, Ng, tiles_g;
};

constexpr int LOSS_ITEMS = 16;                // pixels (keys) per thread
constexpr int LOSS_TILE = 256 * LOSS_ITEMS;   // pixels one workgroup of 256 threads takes

// the tile of workgroup blockIdx.x, in the class plane blockIdx.y (lovasz.hip; a grid without planes: c = 0 and seg = g)
struct LossTile {
  int c, g, seg, tile, lo, n;   // class, group, segment c * G + g, tile of the group, its first position inside the group, its pixels
  int first;                    // its first pixel
  size_t pfirst;                // index of that pixel in arrays of one plane of P entries per class
};
__device__ __forceinline__ LossTile loss_tile(const LossCall& k) {
  LossTile t;
  t.g = blockIdx.x / k.tiles_g;
  t.c = blockIdx.y, t.tile = blockIdx.x - t.g * k.tiles_g, t.seg = t.c * k.G + t.g;
  t.lo = t.tile * LOSS_TILE, t.n = min(LOSS_TILE, k.Ng - t.lo);
  t.first = t.g * k.Ng + t.lo;
  t.pfirst = (size_t)t.c * k.P + (size_t)t.g * k.Ng + t.lo;
  return t;
}
// position inside the tile of item i of this thread in the (wave, item, lane) order, which is the pixel order
__device__ __forceinline__ int loss_item(int i) { return (threadIdx.x >> 6) * (64 * LOSS_ITEMS) + i * 64 + (threadIdx.x & 63); }

// Every backward kernel multiplies by gs = grad_scale * (*grad_scale_dev if given): the upstream gradient of the scalar loss, as a
// host number, a device scalar (an autograd grad_output: no host synchronisation) or both.  (pc_grad_kernel folds its denominator
// into the same factor in double and does not come through here.)
__device__ __forceinline__ float up_scale(float gs, const float* __restrict__ gs_dev) { return gs_dev ? gs * *gs_dev : gs; }

}  // namespace mgu

namespace mgud {

// the gradient request of a *_backward entry point: the upstream factor, where the rows go and how
struct LossGrad {
  float scale;
  const float* scale_dev;
  float* dlogits;
  int64_t ds_n, ds_c, ds_p;
  int accumulate, zero_to;   // zero_to: classes [C, zero_to) of every pixel are written 0 (pixel_ce.hip)
};

// The checks every loss with a LossCall shares (hint: what the entry point's "bad args" message names in brackets; fn: its name as the
// messages spell it), then the device, the descriptor and the device pointer of the context's error word.
inline int loss_call(mgu_ctx* c, const char* fn, const char* hint, const void* logits, const int64_t* labels, int B, int64_t HW, int C,
                     int64_t ls_n, int64_t ls_c, int64_t ls_p, int per_image, int64_t ignore_index, mgu::LossCall* k, int** err_dev) {
  if (!logits || !labels || B < 1 || HW < 1 || C < 1 || C > 8) return fail(c, MGU_ERR_INVALID, "bad %s args (%s)", fn, hint);
  if ((double)B * (double)HW >= (double)(1 << 30)) return fail(c, MGU_ERR_INVALID, "%s: B*HW must stay below 2^30", fn);
  HIPCHK(c, hipSetDevice(c->device));
  k->logits = (const float*)logits, k->labels = labels, k->ls_n = ls_n, k->ls_c = ls_c, k->ls_p = ls_p, k->ignore = ignore_index;
  k->HW = (int)HW, k->C = C, k->P = (int)(B * HW), k->G = per_image ? B : 1, k->Ng = per_image ? (int)HW : k->P;
  k->tiles_g = (k->Ng + mgu::LOSS_TILE - 1) / mgu::LOSS_TILE;
  return err_word_dev(c, err_dev);
}

// Compile-time dispatch: f gets the padded class count of C (4 or 8), or a flag, as a type, and launches the kernel of
// decltype(arg)::value.  Only the combinations a call site spells are instantiated.
template <int V>
using int_c = std::integral_constant<int, V>;
template <typename F>
inline void with_nc(int C, F&& f) {
  if (C <= 4) f(int_c<4>{});
  else f(int_c<8>{});
}
template <typename F>
inline void with_flag(bool on, F&& f) {
  if (on) f(std::true_type{});
  else f(std::false_type{});
}

}  // namespace mgud
