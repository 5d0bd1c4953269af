// Inputs of the graph branch for a whole batch, on the device: the per-patch node features scripts/graph_refinement.py:72-113
// defines and the per-patch labels scripts/train_end_to_end.py:340 describes ("argmax of initial_seg_logits_single, pooled over patch
// regions").  The training script draws both from torch's RNG (train_end_to_end.py:326, :342).
//   mgu_patch_node_features_u8   [patches.mean() x R | caller's U-Net patch rows | mean Sobel byte | mean equalised bytes | 0 ...]
//   mgu_patch_labels             per-patch class histogram, majority label, purity
// The byte columns are the composition mgu_sobel_edges_u8 / mgu_equalize_hist_rgb_u8 -> mgu_patch_mean_u8 per image, bit for bit: the
// arithmetic is imgmath.h's (shared with imageops.hip), the sums are integers, the mean is patch_mean_u8_kernel's expression.  What
// differs is the schedule.  mgu_patch_node_features_u8 is ONE memset and THREE kernel launches whatever B is:
//   1. patch_stats_kernel   per-image 256-bin luminance histogram and largest squared Sobel magnitude: LDS bins / LDS max per 32 x 32
//                           tile, then global integer atomicAdd / atomicMax (order-free, so bit-reproducible)
//   2. patch_lut_kernel     the B equalisation tables
//   3. patch_rows_kernel    one workgroup per patch (one WAVE per patch when the patch has <= 64 pixels): the patch's grey tile with its
//                           one-pixel reflect-101 halo (reflected at the IMAGE border) in LDS, Sobel and equalised bytes recomputed
//                           in registers and summed as integers, wave shuffles + LDS across the waves, the whole row written
// No Sobel map and no equalised image reaches memory; the workspace is B x 256 bins, B maxima and B x 256 table bytes (mgu_ctx::imgws).
// mgu_patch_labels is ONE launch: per-wave class counts by ballot (lane c keeps class c), summed in LDS counters per patch.
// All of it is byte / integer work bound by HBM and L2.
#include <limits.h>

#include "ctx.h"
#include "imgmath.h"

namespace mgu {
namespace {

constexpr int PI_THREADS = 256;
constexpr int PI_MAX_PATCH = 64;                                   // node features: the grey tile (patch + 2)^2 lives in LDS
constexpr int PI_TILE = 32;                                        // statistics pass: 32 x 32 pixels per workgroup, 4 per thread
constexpr int PI_MAX_CLASSES = 32;                                 // patch labels: lane c of a wave counts class c; key packs 6 bits
constexpr int PI_MAX_LABEL_PATCH = 4096;

// grey values of the (th + 2) x (tw + 2) window whose interior starts at (y0, x0), reflect-101 at the image border, into lds (row pitch
// tw + 2) by the `nthr` threads t = 0 .. nthr-1.  Window positions beyond the image's own halo (a tile overhanging the bottom / right
// edge) are clamped onto it: they are never read by a pixel inside the image.
__device__ __forceinline__ void stage_gray(const uint8_t* __restrict__ rgb, int H, int W, int y0, int x0, int th, int tw, uint8_t* lds, int t,
                                           int nthr) {
  const int pw = tw + 2, n = (th + 2) * pw;
  for (int i = t; i < n; i += nthr) {
    const int r = i / pw, q = i - r * pw;
    const int yy = H > 1 ? reflect101(min(y0 - 1 + r, H), H) : 0, xx = W > 1 ? reflect101(min(x0 - 1 + q, W), W) : 0;
    lds[i] = (uint8_t)cv_gray(rgb + ((size_t)yy * W + xx) * 3);
  }
}
__device__ __forceinline__ int sobel_mag2_lds(const uint8_t* lds, int pw, int ly, int lx) {   // interior pixel (ly, lx) of a staged window
  int g[3][3];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) g[dy][dx] = lds[(ly + dy) * pw + lx + dx];
  return sobel_mag2(g);
}

// ---- 1. per-image luminance histogram and largest squared gradient ------------------------------------------------------------------
__global__ __launch_bounds__(PI_THREADS) void patch_stats_kernel(const uint8_t* __restrict__ rgb, int H, int W, int tiles_x, int tiles_per_img,
                                                                 unsigned* __restrict__ hist, unsigned* __restrict__ max2) {
  __shared__ unsigned h[256];
  __shared__ unsigned mx;
  __shared__ uint8_t gray[(PI_TILE + 2) * (PI_TILE + 2)];
  const int b = blockIdx.x / tiles_per_img, tile = blockIdx.x - b * tiles_per_img;
  const int ty = tile / tiles_x, y0 = ty * PI_TILE, x0 = (tile - ty * tiles_x) * PI_TILE;
  const uint8_t* img = rgb + (size_t)b * H * W * 3;
  h[threadIdx.x] = 0;
  if (threadIdx.x == 0) mx = 0;
  stage_gray(img, H, W, y0, x0, PI_TILE, PI_TILE, gray, threadIdx.x, PI_THREADS);
  __syncthreads();
  unsigned local = 0;
#pragma unroll
  for (int k = 0; k < PI_TILE * PI_TILE / PI_THREADS; ++k) {
    const int i = threadIdx.x + k * PI_THREADS, ly = i / PI_TILE, lx = i % PI_TILE;
    const int y = y0 + ly, x = x0 + lx;
    if (y < H && x < W) {
      local = max(local, (unsigned)sobel_mag2_lds(gray, PI_TILE + 2, ly, lx));
      int Y, U, V;
      cv_rgb2yuv(img + ((size_t)y * W + x) * 3, Y, U, V);
      atomicAdd(&h[Y], 1u);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) local = max(local, (unsigned)__shfl_xor((int)local, off));   // unsigned max: not wave_max
  if ((threadIdx.x & 63) == 0 && local) atomicMax(&mx, local);
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[b * 256 + threadIdx.x], h[threadIdx.x]);
  if (threadIdx.x == 0 && mx) atomicMax(&max2[b], mx);
}

// ---- 2. the B equalisation tables -------------------------------------------------------------------------------------------------------
__global__ void patch_lut_kernel(const unsigned* __restrict__ hist, int64_t total, uint8_t* __restrict__ lut) {
  if (threadIdx.x == 0) equalize_lut_build(hist + blockIdx.x * 256, total, lut + blockIdx.x * 256);
}

// ---- 3. one row per patch ---------------------------------------------------------------------------------------------------------------
struct RowArgs {
  const uint8_t* rgb;        // (B, H, W, 3)
  const float* img;          // normalised image by strides, or NULL
  int64_t s_n, s_c, s_h, s_w;
  const float* unet;         // (B*Np, Cu) or NULL
  const unsigned* max2;      // (B)
  const uint8_t* lut;        // (B, 256)
  float* out;                // (B*Np, ld_out)
  int H, W, patch, nph, npw, R, Cu, per_channel, ld_out;
  int64_t rows;              // B * Np
};
// WPG waves work on one patch: 4 (the workgroup) or 1 (a patch of <= 64 pixels; the workgroup then takes 4 patches)
template <int WPG>
__global__ __launch_bounds__(PI_THREADS) void patch_rows_kernel(const RowArgs a) {
  constexpr int PPB = PI_THREADS / 64 / WPG, TPP = 64 * WPG;
  constexpr int TILE_BYTES = WPG == 4 ? (PI_MAX_PATCH + 2) * (PI_MAX_PATCH + 2) : 10 * 10;
  __shared__ uint8_t gray[PPB][TILE_BYTES];
  __shared__ uint8_t lut[PPB][256];
  __shared__ unsigned red_u[PI_THREADS / 64][4];
  __shared__ double red_d[PI_THREADS / 64];
  const int wave = threadIdx.x >> 6, grp = wave / WPG, t = threadIdx.x - grp * TPP;
  const int64_t row = (int64_t)blockIdx.x * PPB + grp;
  const bool live = row < a.rows;                       // a dead group runs the barriers and touches no memory
  const int p = a.patch, Np = a.nph * a.npw, pw = p + 2;
  const int b = live ? (int)(row / Np) : 0, pidx = live ? (int)(row - (int64_t)b * Np) : 0;
  const int py = pidx / a.npw, px = pidx - py * a.npw, y0 = py * p, x0 = px * p;
  const uint8_t* rgb = a.rgb + (size_t)b * a.H * a.W * 3;
  if (live) {
    stage_gray(rgb, a.H, a.W, y0, x0, p, p, gray[grp], t, TPP);
    for (int i = t; i < 256; i += TPP) lut[grp][i] = a.lut[b * 256 + i];
  }
  __syncthreads();
  unsigned s[4] = {0, 0, 0, 0};   // Sobel, equalised R, G, B: at most 255 * 64 * 64 each
  double sd = 0.0;
  if (live) {
    const double mx = sqrt((double)a.max2[b]);
    const bool mean = a.img && a.R > 0;
    const float* fimg = a.img + (mean ? b * a.s_n : 0);
    for (int i = t; i < p * p; i += TPP) {
      const int ly = i / p, lx = i - ly * p, y = y0 + ly, x = x0 + lx;
      if (y < a.H && x < a.W) {                          // pad pixels are zeros in every sum
        s[0] += sobel_norm_u8(sobel_mag2_lds(gray[grp], pw, ly, lx), mx);
        int Y, U, V, r, g, bl;
        cv_rgb2yuv(rgb + ((size_t)y * a.W + x) * 3, Y, U, V);
        cv_yuv2rgb(lut[grp][Y], U, V, r, g, bl);
        s[1] += r, s[2] += g, s[3] += bl;
        if (mean) {
          const float* q = fimg + y * a.s_h + x * a.s_w;
          sd += (double)q[0];
          sd += (double)q[a.s_c];
          sd += (double)q[2 * a.s_c];
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) s[k] = wave_sum(s[k]);
  sd = wave_sum(sd);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) red_u[wave][k] = s[k];
    red_d[wave] = sd;
  }
  __syncthreads();
  if (!live) return;
  unsigned tot[4] = {0, 0, 0, 0};
  double totd = 0.0;
#pragma unroll
  for (int w = 0; w < WPG; ++w) {                       // fixed order: the double sum is reproducible
#pragma unroll
    for (int k = 0; k < 4; ++k) tot[k] += red_u[grp * WPG + w][k];
    totd += red_d[grp * WPG + w];
  }
  const double pp = (double)p * p;
  const float fmean = (float)(totd / (3.0 * pp));
  const int c_sob = (a.img && a.R > 0 ? a.R : 0) + (a.unet ? a.Cu : 0), c_unet = c_sob - (a.unet ? a.Cu : 0);
  const int n_eq = a.per_channel ? 3 : 1;
  float* o = a.out + row * a.ld_out;
  for (int c = t; c < a.ld_out; c += TPP) {
    float v = 0.f;                                       // columns past the used ones
    if (c < c_unet) v = fmean;
    else if (c < c_sob) v = a.unet[row * a.Cu + (c - c_unet)];
    else if (c == c_sob) v = (float)((double)tot[0] / pp);
    else if (c <= c_sob + n_eq) {
      const int k = c - c_sob;
      v = a.per_channel ? (float)((double)(k == 1 ? tot[1] : (k == 2 ? tot[2] : tot[3])) / pp) : (float)((double)(tot[1] + tot[2] + tot[3]) / (pp * 3));
    }
    o[c] = v;
  }
}

// ---- patch labels -------------------------------------------------------------------------------------------------------------------------
// class of pixel g: the map's entry, or the first maximal channel of the logits (the pick of argmax_kernel); -1 = counted nowhere
template <int KIND>
__device__ __forceinline__ int pixel_class(const void* src, int64_t g, int C) {
  if constexpr (KIND == 0) {
    const long long v = reinterpret_cast<const long long*>(src)[g];
    return v >= 0 && v < C ? (int)v : -1;
  } else {
    const float* p = reinterpret_cast<const float*>(src) + g * C;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < C; ++c)
      if (p[c] > best) {
        best = p[c];
        bi = c;
      }
    return bi;
  }
}
template <int KIND, int WPG>
__global__ __launch_bounds__(PI_THREADS) void patch_labels_kernel(const void* __restrict__ src, int H, int W, int C, int patch, int nph, int npw,
                                                                  int64_t rows, int32_t* __restrict__ counts, int64_t* __restrict__ labels,
                                                                  float* __restrict__ purity) {
  constexpr int PPB = PI_THREADS / 64 / WPG, TPP = 64 * WPG;
  __shared__ int cnt[PPB][PI_MAX_CLASSES];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, grp = wave / WPG, t = threadIdx.x - grp * TPP;
  const int64_t row = (int64_t)blockIdx.x * PPB + grp;
  const bool live = row < rows;
  const int Np = nph * npw;
  const int b = live ? (int)(row / Np) : 0, pidx = live ? (int)(row - (int64_t)b * Np) : 0;
  const int py = pidx / npw, px = pidx - py * npw, y0 = py * patch, x0 = px * patch;
  if (threadIdx.x < PPB * PI_MAX_CLASSES) (&cnt[0][0])[threadIdx.x] = 0;
  __syncthreads();
  int mine = 0;                                          // lane c: this wave's pixels of class c
  const int n = patch * patch;
  for (int i0 = 0; i0 < n; i0 += TPP) {                  // whole waves take every trip: the ballots below need all 64 lanes
    const int i = i0 + t, ly = i / patch, lx = i - ly * patch, y = y0 + ly, x = x0 + lx;
    int v = -1;
    if (live && i < n && y < H && x < W) v = pixel_class<KIND>(src, ((int64_t)b * H + y) * W + x, C);
    for (int c = 0; c < C; ++c) {
      const unsigned long long m = __ballot(v == c);
      if (lane == c) mine += __popcll(m);
    }
  }
  if (lane < C && mine) atomicAdd(&cnt[grp][lane], mine);
  __syncthreads();
  if (!live || t >= 64) return;                          // the group's first wave finishes the patch
  const int my = lane < C ? cnt[grp][lane] : 0;
  const int key = wave_max(lane < C ? my * 64 + (63 - lane) : 0);   // largest count, lowest class on ties
  const int best = key >> 6;
  if (counts && lane < C) counts[row * C + lane] = my;
  if (lane == 0) {
    const int real = min(patch, H - y0) * min(patch, W - x0);
    labels[row] = best ? 63 - (key & 63) : 0;            // no counted pixel: label 0, purity 0
    if (purity) purity[row] = (float)((double)best / (double)real);
  }
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_patch_node_features_u8(mgu_ctx* c, const uint8_t* rgb_dev, int B, int H, int W, int patch, const float* img_dev, int64_t is_n, int64_t is_c,
                               int64_t is_h, int64_t is_w, int repeat, const float* unet_rows_dev, int unet_cols, int per_channel, float* out_dev,
                               int ld_out, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!rgb_dev || !out_dev || B < 1 || H < 1 || W < 1 || patch < 1 || patch > PI_MAX_PATCH || repeat < 0 || (unet_rows_dev && unet_cols < 1))
    return fail(c, MGU_ERR_INVALID, "bad patch_node_features args (patch 1..%d, repeat >= 0, unet_cols >= 1 with unet rows)", PI_MAX_PATCH);
  if ((int64_t)H * W > INT_MAX) return fail(c, MGU_ERR_INVALID, "patch_node_features: H * W must stay below 2^31");
  const int nph = (H + patch - 1) / patch, npw = (W + patch - 1) / patch;
  const int tiles_x = (W + PI_TILE - 1) / PI_TILE, tiles = tiles_x * ((H + PI_TILE - 1) / PI_TILE);
  const int64_t rows = (int64_t)B * nph * npw;
  if (rows > INT_MAX || (int64_t)B * tiles > INT_MAX) return fail(c, MGU_ERR_INVALID, "patch_node_features: B * patches must stay below 2^31");
  const int64_t used = (int64_t)(img_dev && repeat > 0 ? repeat : 0) + (unet_rows_dev ? unet_cols : 0) + 1 + (per_channel ? 3 : 1);
  if (ld_out < used) return fail(c, MGU_ERR_INVALID, "patch_node_features: ld_out %d below the %lld used columns", ld_out, (long long)used);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Carve cv;
  const size_t o_hist = cv.take((size_t)B * 257 * sizeof(unsigned)), o_lut = cv.take((size_t)B * 256);   // [B][256] bins, then [B] maxima
  int rc = ensure(c, &c->imgws, &c->imgws_bytes, cv.off);
  if (rc) return rc;
  unsigned* hist = (unsigned*)((char*)c->imgws + o_hist);
  unsigned* max2 = hist + (size_t)B * 256;
  uint8_t* lut = (uint8_t*)c->imgws + o_lut;
  HIPCHK(c, hipMemsetAsync(hist, 0, (size_t)B * 257 * sizeof(unsigned), s));
  hipLaunchKernelGGL(patch_stats_kernel, dim3(B * tiles), dim3(PI_THREADS), 0, s, rgb_dev, H, W, tiles_x, tiles, hist, max2);
  hipLaunchKernelGGL(patch_lut_kernel, dim3(B), dim3(64), 0, s, hist, (int64_t)H * W, lut);
  RowArgs a;
  a.rgb = rgb_dev, a.img = img_dev, a.s_n = is_n, a.s_c = is_c, a.s_h = is_h, a.s_w = is_w;
  a.unet = unet_rows_dev, a.max2 = max2, a.lut = lut, a.out = out_dev;
  a.H = H, a.W = W, a.patch = patch, a.nph = nph, a.npw = npw, a.R = repeat, a.Cu = unet_cols, a.per_channel = per_channel ? 1 : 0, a.ld_out = ld_out;
  a.rows = rows;
  if (patch * patch <= 64) hipLaunchKernelGGL(patch_rows_kernel<1>, dim3((unsigned)((rows + 3) / 4)), dim3(PI_THREADS), 0, s, a);
  else hipLaunchKernelGGL(patch_rows_kernel<4>, dim3((unsigned)rows), dim3(PI_THREADS), 0, s, a);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_patch_labels(mgu_ctx* c, const void* src_dev, int src_kind, int B, int H, int W, int C, int patch, int32_t* counts_dev, int64_t* labels_dev,
                     float* purity_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!src_dev || !labels_dev || B < 1 || H < 1 || W < 1 || patch < 1 || patch > PI_MAX_LABEL_PATCH) return fail(c, MGU_ERR_INVALID, "bad patch_labels args");
  if (src_kind != 0 && src_kind != 1) return fail(c, MGU_ERR_INVALID, "patch_labels: src_kind %d (0 int64 class map, 1 fp32 logits)", src_kind);
  if (C < 1 || C > PI_MAX_CLASSES) return fail(c, MGU_ERR_INVALID, "patch_labels: %d classes (1..%d)", C, PI_MAX_CLASSES);
  const int nph = (H + patch - 1) / patch, npw = (W + patch - 1) / patch;
  const int64_t rows = (int64_t)B * nph * npw;
  if (rows > INT_MAX) return fail(c, MGU_ERR_INVALID, "patch_labels: B * patches must stay below 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const bool small = patch * patch <= 64;
  const dim3 grid((unsigned)(small ? (rows + 3) / 4 : rows)), block(PI_THREADS);
#define MGU_PL(KIND, WPG) \
  hipLaunchKernelGGL((patch_labels_kernel<KIND, WPG>), grid, block, 0, s, src_dev, H, W, C, patch, nph, npw, rows, counts_dev, labels_dev, purity_dev)
  if (src_kind == 0) {
    if (small) MGU_PL(0, 1);
    else MGU_PL(0, 4);
  } else {
    if (small) MGU_PL(1, 1);
    else MGU_PL(1, 4);
  }
#undef MGU_PL
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
