// Scale / crop / rotation and colour augmentation of a uint8 batch, straight into the normalised fp32 batch and the int64 masks the
// trainer takes (include/mgunet.h, "scale, crop and colour augmentation": THIS BUILD'S DEFINITION, integers only up to the final
// ToTensor + Normalize).
//   affine_luma_kernel     per-image sums S = sum (77 R + 150 G + 29 B) of the SOURCE images into a uint64 table of the context's image
//                          scratch (cleared by the one fill of the stage); launched only when some image has a contrast gain k != 0
//   affine_color_kernel    one launch for the images and the masks of the whole batch: 16.16 fixed-point source coordinates in int64,
//                          bilinear blend with 8-bit fractions (image), nearest (mask), Q12 colour matrix, u8_normalize
// The source footprint is gathered from global memory, not staged in LDS: a 32 x 32 output tile at zoom 0.5 and 15 degrees covers about
// 80 x 80 source pixels (19 KB), which one pass over the tile reads about once anyway, and the whole 8 x 512 x 512 x 3 source (6.3 MB)
// stays in the L2 / Infinity Cache between the luma pass and the gather.  What bounded the first form was the NUMBER of gathers (twelve
// byte loads per pixel), not their bytes: aff_load_run.  NOTES.md ("Affine + colour augmentation") has the timings.
#include <algorithm>

#include "augment_affine.h"

namespace mgu {

constexpr int AFF_LUMA_TILE = 8192;       // source pixels per workgroup of the luma kernel: 24576 bytes = 6 x 16 bytes per thread

// Bytes [3 T tile, 3 T (tile + 1)) of image b (clipped to the image): the 16-byte chunks at 16-byte aligned ADDRESSES that lie wholly
// inside that range, several loads in flight per thread, and the fewer than 16 bytes in front of the first and behind the last of
// them one byte per thread, so no load leaves the range.  A byte at image offset o belongs to channel o % 3; a chunk at offset a has the
// channel phase a % 3, and its four words take the three packed weight words in turn (4 % 3 == 1).  Sums: at most 24576 bytes x 255
// x 150 per workgroup, exact in 32 bits.  One 64-bit atomic per workgroup and image: atomics on one address from all over the chip
// take their turns, which is what a tile of 4096 pixels (64 of them per 512 x 512 image) spent most of its 8 us on.
__global__ __launch_bounds__(256) void affine_luma_kernel(const uint8_t* __restrict__ img, int B, int n, int bgr,
                                                          unsigned long long* __restrict__ sums) {
  __shared__ unsigned sh[4];
  const int tiles_i = (n + AFF_LUMA_TILE - 1) / AFF_LUMA_TILE, nb = n * 3;   // n <= 8192^2: 3 n fits an int
  const unsigned total = (unsigned)B * (unsigned)tiles_i;                     // < 2^31 (checked on the host)
  const unsigned w[3] = {bgr ? 29u : 77u, 150u, bgr ? 77u : 29u};
  unsigned pk[3];   // weights of four consecutive bytes whose first has channel q
#pragma unroll
  for (int q = 0; q < 3; ++q) pk[q] = w[q] | (w[(q + 1) % 3] << 8) | (w[(q + 2) % 3] << 16) | (w[q] << 24);
  for (unsigned t = blockIdx.x; t < total; t += gridDim.x) {
    const int b = (int)(t / (unsigned)tiles_i), tile = (int)(t % (unsigned)tiles_i);
    const uint8_t* ib = img + (int64_t)b * nb;
    const int lo = tile * (AFF_LUMA_TILE * 3), hi = min(lo + AFF_LUMA_TILE * 3, nb);
    const int fa = min(lo + (int)((16u - (unsigned)(((uintptr_t)ib + (uintptr_t)lo) & 15)) & 15u), hi);   // first aligned address in range
    const int nfull = (hi - fa) / 16, fe = fa + nfull * 16;
    unsigned acc = 0;
#pragma unroll 2
    for (int i = (int)threadIdx.x; i < nfull; i += 256) {
      const int a = fa + i * 16;
      const unsigned ph = (unsigned)a % 3u;
      const uint4 v = *(const uint4*)(ib + a);
      acc = __builtin_amdgcn_udot4(v.x, pk[ph], acc, false);
      acc = __builtin_amdgcn_udot4(v.y, pk[(ph + 1) % 3], acc, false);
      acc = __builtin_amdgcn_udot4(v.z, pk[(ph + 2) % 3], acc, false);
      acc = __builtin_amdgcn_udot4(v.w, pk[ph], acc, false);
    }
    if (threadIdx.x < 32) {   // [lo, fa) and [fe, hi): fewer than 16 bytes each
      const int a = threadIdx.x < 16 ? lo + (int)threadIdx.x : fe + (int)threadIdx.x - 16;
      if (a < (threadIdx.x < 16 ? fa : hi)) acc += w[(unsigned)a % 3u] * (unsigned)ib[a];
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&sums[b], (unsigned long long)sh[0] + sh[1] + sh[2] + sh[3]);
    __syncthreads();
  }
}

// One thread: AFF_XV consecutive x of one output row of one image: three channels and the mask label.  params: (B, 16) int32
// {a0..a5, A row-major, k}.  sums == nullptr: no image has k != 0 (the host's statement), t = 0.
// VEC: output x-stride 1 and every row / channel / image start 16-byte aligned (W % 4 == 0); mask rows then too.
template <bool VEC>
__global__ __launch_bounds__(256) void affine_color_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, int B, int Hs,
                                                           int Ws, int bgr, int num_classes, float* __restrict__ out, int H, int W,
                                                           AffStrides so, AffNorm nm, int fill0, int fill1, int fill2,
                                                           int64_t* __restrict__ mask_out, int64_t mask_fill, const int* __restrict__ params,
                                                           const unsigned long long* __restrict__ sums) {
  const unsigned tiles_x = (unsigned)((W + AFF_TX - 1) / AFF_TX), tiles_y = (unsigned)((H + AFF_TY - 1) / AFF_TY);
  const unsigned total = (unsigned)B * tiles_y * tiles_x;   // < 2^31 (checked on the host)
  const int lx = (int)(threadIdx.x % (AFF_TX / AFF_XV)) * AFF_XV, ly = (int)(threadIdx.x / (AFF_TX / AFF_XV));
  const int fill[3] = {fill0, fill1, fill2};
  const int row = Ws * 3;
  const uint8_t* img_end = img + (int64_t)B * Hs * row;
  for (unsigned t = blockIdx.x; t < total; t += gridDim.x) {
    const int x0 = (int)(t % tiles_x) * AFF_TX + lx;
    const unsigned r = t / tiles_x;
    const int y = (int)(r % tiles_y) * AFF_TY + ly, b = (int)(r / tiles_y);
    if (y >= H || x0 >= W) continue;
    const int* p = params + 16 * b;
    const int64_t sx0 = (int64_t)p[2] + (int64_t)y * p[1] + (int64_t)x0 * p[0];
    const int64_t sy0 = (int64_t)p[5] + (int64_t)y * p[4] + (int64_t)x0 * p[3];
    const int a0 = p[0], a3 = p[3];
    int A[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = p[6 + i];
    const int kq = p[15];
    int tt = 0;
    if (kq != 0 && sums) tt = (int)(((int64_t)kq * aff_mean_q8(sums[b], Hs * Ws) + 128) >> 8);   // |k m| < 2^31
    const uint8_t* ib = img + (int64_t)b * Hs * row;
    const uint8_t* mb = mask + (int64_t)b * Hs * Ws;
    float val[3][AFF_XV];
    int64_t lab[AFF_XV];
#pragma unroll
    for (int k = 0; k < AFF_XV; ++k) {
      const int64_t sx = sx0 + (int64_t)k * a0, sy = sy0 + (int64_t)k * a3;
      // every index below -1 or above the side is as far outside as -2 / the side: no tap of it lies inside
      const int ix = (int)min(max(sx >> 16, (int64_t)-2), (int64_t)Ws), iy = (int)min(max(sy >> 16, (int64_t)-2), (int64_t)Hs);
      const unsigned fx = (unsigned)(sx >> 8) & 255u, fy = (unsigned)(sy >> 8) & 255u;
      const bool x0in = (unsigned)ix < (unsigned)Ws, x1in = (unsigned)(ix + 1) < (unsigned)Ws;
      const bool y0in = (unsigned)iy < (unsigned)Hs, y1in = (unsigned)(iy + 1) < (unsigned)Hs;
      const unsigned w00 = (256u - fx) * (256u - fy), w10 = fx * (256u - fy), w01 = (256u - fx) * fy, w11 = fx * fy;
      const int o = iy * row + ix * 3;   // dereferenced only where a tap of that row lies inside
      unsigned ta0, ta1, tb0, tb1;       // the two rows' six bytes
      aff_load_run(ib + o, img, img_end, (const uint8_t*)p, x0in && y0in, x1in && y0in, ta0, ta1);
      aff_load_run(ib + o + row, img, img_end, (const uint8_t*)p, x0in && y1in, x1in && y1in, tb0, tb1);
      int v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sc = bgr ? 2 - c : c;   // byte sc of the first tap, byte 3 + sc of the second
        const unsigned sh0 = 8u * (unsigned)sc, sh1 = 8u * (unsigned)((3 + sc) & 3);
        const unsigned p00 = (x0in && y0in) ? (ta0 >> sh0) & 255u : (unsigned)fill[c];
        const unsigned p10 = (x1in && y0in) ? ((sc == 0 ? ta0 : ta1) >> sh1) & 255u : (unsigned)fill[c];
        const unsigned p01 = (x0in && y1in) ? (tb0 >> sh0) & 255u : (unsigned)fill[c];
        const unsigned p11 = (x1in && y1in) ? ((sc == 0 ? tb0 : tb1) >> sh1) & 255u : (unsigned)fill[c];
        v[c] = (int)((w00 * p00 + w10 * p10 + w01 * p01 + w11 * p11 + 32768u) >> 16);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int q = (A[3 * c] * v[0] + A[3 * c + 1] * v[1] + A[3 * c + 2] * v[2] + tt + 2048) >> 12;   // below 2^25 + 2^23: int
        val[c][k] = u8_normalize((uint8_t)min(max(q, 0), 255), c, nm.m0, nm.m1, nm.m2, nm.s0, nm.s1, nm.s2);
      }
      if (mask_out) {
        const int mx = (int)min(max((sx + 32768) >> 16, (int64_t)-1), (int64_t)Ws), my = (int)min(max((sy + 32768) >> 16, (int64_t)-1), (int64_t)Hs);
        int64_t m = mask_fill;
        if ((unsigned)mx < (unsigned)Ws && (unsigned)my < (unsigned)Hs) {
          const int u = mb[my * Ws + mx];
          m = num_classes > 0 ? min(u, num_classes - 1) : u;
        }
        lab[k] = m;
      }
    }
    const int64_t obase = b * so.b + y * so.h;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = out + obase + c * so.c;
      if (VEC) {
        *(float4*)(o + x0) = make_float4(val[c][0], val[c][1], val[c][2], val[c][3]);
      } else {
#pragma unroll
        for (int k = 0; k < AFF_XV; ++k)
          if (x0 + k < W) o[(x0 + k) * so.w] = val[c][k];
      }
    }
    if (mask_out) {
      int64_t* mo = mask_out + (int64_t)b * H * W + (int64_t)y * W + x0;
      if (VEC) {
        ((longlong2*)mo)[0] = make_longlong2(lab[0], lab[1]);
        ((longlong2*)mo)[1] = make_longlong2(lab[2], lab[3]);
      } else {
#pragma unroll
        for (int k = 0; k < AFF_XV; ++k)
          if (x0 + k < W) mo[k] = lab[k];
      }
    }
  }
}

}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

// B * luma tiles of a batch of Hs x Ws images
int64_t luma_tiles(int B, int Hs, int Ws) { return (int64_t)B * (((int64_t)Hs * Ws + AFF_LUMA_TILE - 1) / AFF_LUMA_TILE); }

// the fill of the B sums and the luma kernel (sizes checked by the caller)
int luma_launch(mgu_ctx* c, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, unsigned long long* sums, hipStream_t s) {
  HIPCHK(c, hipMemsetAsync(sums, 0, (size_t)B * sizeof(unsigned long long), s));
  ProfScope ps(c, s, "augment luma");
  hipLaunchKernelGGL(affine_luma_kernel, dim3((unsigned)std::min<int64_t>(luma_tiles(B, Hs, Ws), 256 * 16)), dim3(256), 0, s, img_u8, B, Hs * Ws,
                     bgr ? 1 : 0, sums);
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_augment_luma_tile(void) { return AFF_LUMA_TILE; }

int mgu_augment_luma_sums(mgu_ctx* c, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, int64_t* sums_dev, void* hip_stream) {
  if (!img_u8 || !sums_dev) return fail(c, MGU_ERR_INVALID, "augment_luma_sums: null pointer (images or sums_dev)");
  if (B < 1 || Hs < 1 || Ws < 1) return fail(c, MGU_ERR_INVALID, "augment_luma_sums: B, Hs, Ws must be >= 1");
  if (Hs > AFF_MAX_SIDE || Ws > AFF_MAX_SIDE) return fail(c, MGU_ERR_INVALID, "augment_luma_sums: %d x %d is above %d pixels a side", Hs, Ws, AFF_MAX_SIDE);
  if (luma_tiles(B, Hs, Ws) >= ((int64_t)1 << 31)) return fail(c, MGU_ERR_INVALID, "augment_luma_sums: batch too large for one launch (B * tiles >= 2^31)");
  if (!c) return fail(c, MGU_ERR_INVALID, "augment_luma_sums: null context");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = luma_launch(c, img_u8, B, Hs, Ws, bgr, (unsigned long long*)sums_dev, (hipStream_t)hip_stream);
  if (rc) return rc;
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

// The argument checks come before the context check, so each refusal has its message (mgu_last_error(NULL) without a context).
int mgu_augment_affine_color(mgu_ctx* c, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, const uint8_t* mask_u8, int num_classes,
                             float* out, int H, int W, const int64_t* out_strides, const float* mean3, const float* std3,
                             const uint8_t* fill_rgb, int64_t* mask_out, int64_t mask_fill, const int32_t* params_dev, int need_mean,
                             void* hip_stream) {
  if (!img_u8 || !out || !out_strides || !mean3 || !std3 || !fill_rgb || !params_dev)
    return fail(c, MGU_ERR_INVALID, "augment_affine_color: null pointer (images, out, out_strides, mean3, std3, fill_rgb or params_dev)");
  if (B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || num_classes < 0)
    return fail(c, MGU_ERR_INVALID, "augment_affine_color: B, Hs, Ws, H, W must be >= 1 and num_classes >= 0");
  if (Hs > AFF_MAX_SIDE || Ws > AFF_MAX_SIDE || H > AFF_MAX_SIDE || W > AFF_MAX_SIDE)
    return fail(c, MGU_ERR_INVALID, "augment_affine_color: %d x %d -> %d x %d is above %d pixels a side", Hs, Ws, H, W, AFF_MAX_SIDE);
  if (!mask_u8 != !mask_out) return fail(c, MGU_ERR_INVALID, "augment_affine_color: mask_u8 and mask_out go together");
  const int64_t tiles = (int64_t)B * ((H + AFF_TY - 1) / AFF_TY) * ((W + AFF_TX - 1) / AFF_TX);
  if (tiles >= ((int64_t)1 << 31) || luma_tiles(B, Hs, Ws) >= ((int64_t)1 << 31))
    return fail(c, MGU_ERR_INVALID, "augment_affine_color: batch too large for one launch (B * tiles >= 2^31)");
  if (!c) return fail(c, MGU_ERR_INVALID, "augment_affine_color: null context");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  unsigned long long* sums = nullptr;
  if (need_mean) {
    int rc = ensure(c, &c->imgws, &c->imgws_bytes, (size_t)B * sizeof(unsigned long long));
    if (rc) return rc;
    sums = (unsigned long long*)c->imgws;
    if ((rc = luma_launch(c, img_u8, B, Hs, Ws, bgr, sums, s))) return rc;
  }
  const AffStrides so{out_strides[0], out_strides[1], out_strides[2], out_strides[3]};
  const AffNorm nm{mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
  const bool vec = so.w == 1 && W % 4 == 0 && so.h % 4 == 0 && so.c % 4 == 0 && so.b % 4 == 0 && aligned16(out) && (!mask_out || aligned16(mask_out));
  const dim3 grid((unsigned)std::min<int64_t>(tiles, 256 * 16));
  {
    ProfScope ps(c, s, "augment affine");
    if (vec)
      hipLaunchKernelGGL(affine_color_kernel<true>, grid, dim3(256), 0, s, img_u8, mask_u8, B, Hs, Ws, bgr ? 1 : 0, num_classes, out, H, W, so, nm,
                         (int)fill_rgb[0], (int)fill_rgb[1], (int)fill_rgb[2], mask_out, mask_fill, (const int*)params_dev, sums);
    else
      hipLaunchKernelGGL(affine_color_kernel<false>, grid, dim3(256), 0, s, img_u8, mask_u8, B, Hs, Ws, bgr ? 1 : 0, num_classes, out, H, W, so, nm,
                         (int)fill_rgb[0], (int)fill_rgb[1], (int)fill_rgb[2], mask_out, mask_fill, (const int*)params_dev, sums);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
