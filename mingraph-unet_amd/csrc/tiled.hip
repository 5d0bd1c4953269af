// Tiled inference on the device: a large image runs through the network as overlapping tiles whose softmaxes are blended into one canvas.
//   mgu_tile_gather      tiles [t0, t0 + n) of a strided fp32 batch -> one contiguous NCHW batch (n, C, Th, Tw), reflect-101 padded
//   mgu_tile_gather_u8   the same from HWC uint8 images with ToTensor + Normalize applied (imageops.hip's arithmetic)
//   mgu_tile_accumulate  the chunk's NHWC logits (or probabilities) -> weighted sum on the NHWC fp32 canvas, in tile order
//   mgu_tile_finish      canvas -> first maximal class (int64) and its probability
// Grid (per axis, mgunet.tiled.tile_grid): length L, tile T, overlap o, stride S = T - o; one tile at 0 when L <= T, else
// ceil((L - T) / S) + 1 tiles at k S, the last moved back to L - T.  Tiles are numbered row-major within an image, image-major over
// the batch.  Every kernel is a gather: a thread owns output elements and looks up what it needs, so nothing is added atomically.  The
// accumulate kernel finds the tiles that cover its pixel from the two axes' origins (arithmetic, no tile list), adds them in ascending tile number,
// starts from 0 when the pixel's first covering tile lies in the chunk and loads the canvas otherwise: chunks given in ascending
// order produce, bit for bit, what one launch over all tiles produces, and the canvas needs no clearing.
#include <algorithm>

#include "ctx.h"

namespace mgu {
namespace {

constexpr int TILE_MAX_C = 16;

struct TileStrides {
  int64_t b, c, h, w;
};
// one axis of the grid: normalised weights (n, T; device, accumulate only), image length, tile, stride, tiles
struct TileAxis {
  const float* wn;
  int L, T, S, n;
};
// origin of tile k of the axis: k S, the last one moved back to L - T; 0 for the single tile of an image no longer than the tile
__host__ __device__ __forceinline__ int tile_origin(const TileAxis& a, int k) { return a.L <= a.T ? 0 : min(k * a.S, a.L - a.T); }
struct TileNorm {
  float mean[3], sd[3];
};

// reflect-101 index folding, repeated as often as needed (numpy.pad(mode="reflect")); L == 1 reads index 0
__device__ __forceinline__ int tile_fold(int i, int L) {
  if ((unsigned)i < (unsigned)L) return i;
  if (L == 1) return 0;
  const int p = 2 * (L - 1);
  i %= p;
  if (i < 0) i += p;
  return i < L ? i : p - i;
}

// [*k0, *k1]: the tiles of the axis that cover coordinate p (consecutive, because the origins ascend); empty when *k0 > *k1
__device__ __forceinline__ void tile_cover(const TileAxis& a, int p, int* k0, int* k1) {
  int lo = p < a.T ? 0 : (p - a.T) / a.S, hi = min(a.n - 1, p / a.S + 1);
  while (lo <= hi && (unsigned)(p - tile_origin(a, lo)) >= (unsigned)a.T) ++lo;
  while (hi >= lo && (unsigned)(p - tile_origin(a, hi)) >= (unsigned)a.T) --hi;
  *k0 = lo, *k1 = hi;
}

// One thread per (tile, row, group of 4 columns), every channel: 16-byte stores along x when Tw % 4 == 0, a 16-byte load where the four
// source pixels are inside the image, unit-stride and aligned, scalar loads through the fold otherwise.
template <bool U8>
__global__ __launch_bounds__(256) void tile_gather_kernel(const void* __restrict__ in, TileStrides s, int C, TileAxis ay, TileAxis ax, int t0,
                                                          int64_t total, int bgr, TileNorm nm, float* __restrict__ out) {
  const int Th = ay.T, Tw = ax.T, H = ay.L, W = ax.L, Tw4 = (Tw + 3) >> 2;
  const bool vec_store = (Tw & 3) == 0;
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int xg = (int)(i % Tw4), y = (int)(i / Tw4 % Th), k = (int)(i / ((int64_t)Tw4 * Th));
    const int t = t0 + k, col = t % ax.n, row = t / ax.n % ay.n, b = t / (ax.n * ay.n);
    const int ox = tile_origin(ax, col), x0 = 4 * xg, nx = min(4, Tw - x0);
    const int sy = tile_fold(tile_origin(ay, row) + y, H);
    const bool inside = nx == 4 && ox + x0 >= 0 && ox + x0 + 3 < W;
    int sx[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sx[j] = inside ? ox + x0 + j : tile_fold(ox + x0 + min(j, nx - 1), W);
    uint8_t px8[4][3];   // uint8 form: the 12 bytes of the four pixels, read once (contiguous when inside)
    if constexpr (U8) {
      const uint8_t* row = (const uint8_t*)in + ((int64_t)b * H + sy) * W * 3;
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int q = 0; q < 3; ++q) px8[j][q] = row[(int64_t)sx[j] * 3 + q];
    }
    for (int c = 0; c < C; ++c) {
      float v[4];
      if constexpr (U8) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const uint8_t u = bgr ? (c == 0 ? px8[j][2] : (c == 1 ? px8[j][1] : px8[j][0])) : (c == 0 ? px8[j][0] : (c == 1 ? px8[j][1] : px8[j][2]));
          v[j] = u8_normalize(u, c, nm.mean[0], nm.mean[1], nm.mean[2], nm.sd[0], nm.sd[1], nm.sd[2]);
        }
      } else {
        const float* src = (const float*)in + b * s.b + c * s.c + sy * s.h;
        if (inside && s.w == 1 && (((uintptr_t)(src + sx[0])) & 15) == 0) {
          const float4 q = *reinterpret_cast<const float4*>(src + sx[0]);
          v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) v[j] = src[sx[j] * s.w];
        }
      }
      float* dst = out + (((int64_t)k * C + c) * Th + y) * Tw + x0;
      if (vec_store) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        for (int j = 0; j < nx; ++j) dst[j] = v[j];
      }
    }
  }
}

// A workgroup covers 4 rows x 64 * PX columns of one image; a thread owns PX horizontally adjacent pixels (PX = 2 for two classes and an
// even W: the pair's canvas values are one aligned 16 bytes).  NC > 0: C == NC; NC == 0: C <= TILE_MAX_C at run time.
template <int NC, int PX>
__global__ __launch_bounds__(256) void tile_accumulate_kernel(const float* __restrict__ tiles, int is_prob, int Crt, TileAxis ay, TileAxis ax,
                                                              int b0, int y0, int t0, int n, float* __restrict__ canvas,
                                                              long long* __restrict__ labels, float* __restrict__ conf) {
  constexpr int CM = NC > 0 ? NC : TILE_MAX_C;
  const int C = NC > 0 ? NC : Crt;
  const int H = ay.L, W = ax.L, Th = ay.T, Tw = ax.T;
  const int b = b0 + blockIdx.z, y = y0 + blockIdx.y * 4 + (threadIdx.x >> 6), xb = (blockIdx.x * 64 + (threadIdx.x & 63)) * PX;
  if (y >= H || xb >= W) return;
  int r0, r1;
  tile_cover(ay, y, &r0, &r1);
  if (r0 > r1) return;
  const int tb = b * ay.n * ax.n, t1 = t0 + n;
  int c0[PX], c1[PX];
  bool touched[PX], fresh[PX], done[PX], any = false, load = false;
#pragma unroll
  for (int px = 0; px < PX; ++px) {
    touched[px] = fresh[px] = done[px] = false;
    if (xb + px >= W) continue;
    tile_cover(ax, xb + px, &c0[px], &c1[px]);
    if (c0[px] > c1[px]) continue;
    for (int r = r0; r <= r1; ++r) touched[px] |= tb + r * ax.n + c0[px] < t1 && tb + r * ax.n + c1[px] >= t0;
    fresh[px] = tb + r0 * ax.n + c0[px] >= t0;   // the pixel's first tile is in this chunk: nothing was added before
    done[px] = tb + r1 * ax.n + c1[px] < t1;     // its last tile too: the sum is final after this chunk
    any |= touched[px];
    load |= touched[px] && !fresh[px];
  }
  if (!any) return;
  const int64_t pix = ((int64_t)b * H + y) * W + xb;
  float acc[PX][CM];
#pragma unroll
  for (int px = 0; px < PX; ++px)
#pragma unroll
    for (int c = 0; c < CM; ++c) acc[px][c] = 0.f;
  if (load) {
    if constexpr (NC == 2 && PX == 2) {
      const float4 q = *reinterpret_cast<const float4*>(canvas + pix * 2);
      if (!fresh[0]) acc[0][0] = q.x, acc[0][1] = q.y;
      if (!fresh[1]) acc[1][0] = q.z, acc[1][1] = q.w;
    } else if constexpr (NC == 4) {
      const float4 q = *reinterpret_cast<const float4*>(canvas + pix * 4);
      acc[0][0] = q.x, acc[0][1] = q.y, acc[0][2] = q.z, acc[0][3] = q.w;
    } else if constexpr (NC == 2) {
      const float2 q = *reinterpret_cast<const float2*>(canvas + pix * 2);
      acc[0][0] = q.x, acc[0][1] = q.y;
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) acc[0][c] = canvas[pix * C + c];
    }
  }
#pragma unroll
  for (int px = 0; px < PX; ++px) {
    if (!touched[px]) continue;
    const int x = xb + px;
    for (int r = r0; r <= r1; ++r) {
      const int iy = y - tile_origin(ay, r);
      if ((unsigned)iy >= (unsigned)Th) continue;
      const float wy = ay.wn[r * Th + iy];
      for (int cc = c0[px]; cc <= c1[px]; ++cc) {
        const int t = tb + r * ax.n + cc, ix = x - tile_origin(ax, cc);
        if (t < t0 || t >= t1 || (unsigned)ix >= (unsigned)Tw) continue;
        const float w = wy * ax.wn[cc * Tw + ix];
        const float* p = tiles + (((int64_t)(t - t0) * Th + iy) * Tw + ix) * C;
        float q[CM];
        if (is_prob) {
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (c < C) q[c] = p[c];
        } else {
          const float sum = pixel_softmax<CM>(p, C, q);
#pragma unroll
          for (int c = 0; c < CM; ++c)
            if (c < C) q[c] = q[c] / sum;
        }
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) acc[px][c] += w * q[c];
      }
    }
  }
  if constexpr (NC == 2 && PX == 2) {
    if (touched[0] && touched[1]) {
      *reinterpret_cast<float4*>(canvas + pix * 2) = make_float4(acc[0][0], acc[0][1], acc[1][0], acc[1][1]);
    } else {
      const int px = touched[0] ? 0 : 1;
      *reinterpret_cast<float2*>(canvas + (pix + px) * 2) = make_float2(acc[px][0], acc[px][1]);
    }
  } else if constexpr (NC == 4) {
    *reinterpret_cast<float4*>(canvas + pix * 4) = make_float4(acc[0][0], acc[0][1], acc[0][2], acc[0][3]);
  } else if constexpr (NC == 2) {
    *reinterpret_cast<float2*>(canvas + pix * 2) = make_float2(acc[0][0], acc[0][1]);
  } else {
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) canvas[pix * C + c] = acc[0][c];
  }
  if (!labels) return;
#pragma unroll
  for (int px = 0; px < PX; ++px) {
    if (!touched[px] || !done[px]) continue;
    float best = 0.f;
    int bi = 0;
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C && (c == 0 || acc[px][c] > best)) best = acc[px][c], bi = c;
    labels[pix + px] = bi;
    conf[pix + px] = best;
  }
}

__global__ __launch_bounds__(256) void tile_finish_kernel(const float* __restrict__ canvas, int64_t npix, int C, long long* __restrict__ labels,
                                                          float* __restrict__ conf) {
  for (int64_t i = blockIdx.x * (int64_t)256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
    float best = canvas[i * C];
    int bi = 0;
    for (int c = 1; c < C; ++c) {
      const float q = canvas[i * C + c];
      if (q > best) best = q, bi = c;
    }
    labels[i] = bi;
    conf[i] = best;
  }
}

// tiles of one axis
int axis_tiles(int L, int T, int o) { return L <= T ? 1 : (L - T + (T - o) - 1) / (T - o) + 1; }

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

// the checks the three grid-walking entry points share; fills the axes (weights left NULL) and the tile count of the batch
int tile_check(mgu_ctx* c, const char* fn, int B, int H, int W, int Th, int Tw, int overlap_y, int overlap_x, int t0, int n, TileAxis* ay,
               TileAxis* ax) {
  if (B < 1 || H < 1 || W < 1 || Th < 1 || Tw < 1)
    return fail(c, MGU_ERR_INVALID, "bad %s args (B, H, W, Th or Tw < 1)", fn);
  if (overlap_y < 0 || overlap_y >= Th || overlap_x < 0 || overlap_x >= Tw)
    return fail(c, MGU_ERR_INVALID, "%s: overlap (%d, %d) must lie in [0, tile) for a (%d, %d) tile", fn, overlap_y, overlap_x, Th, Tw);
  const int nr = axis_tiles(H, Th, overlap_y), nc = axis_tiles(W, Tw, overlap_x);
  if ((int64_t)B * nr * nc > (1 << 30)) return fail(c, MGU_ERR_INVALID, "%s: more than 2^30 tiles", fn);
  if (t0 < 0 || n < 1 || (int64_t)t0 + n > (int64_t)B * nr * nc)
    return fail(c, MGU_ERR_INVALID, "%s: tiles [%d, %d + %d) outside the grid of %d x %d x %d tiles", fn, t0, t0, n, B, nr, nc);
  *ay = TileAxis{nullptr, H, Th, Th - overlap_y, nr};
  *ax = TileAxis{nullptr, W, Tw, Tw - overlap_x, nc};
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_tile_gather(mgu_ctx* c, const float* img_dev, int B, int C, int H, int W, const int64_t* in_strides, int Th, int Tw, int overlap_y,
                    int overlap_x, int t0, int n, float* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_dev || !out_dev || !in_strides || C < 1 || !aligned16(out_dev))
    return fail(c, MGU_ERR_INVALID, "bad tile_gather args (null pointer, C < 1 or out_dev not 16-byte aligned)");
  TileAxis ay, ax;
  int rc = tile_check(c, "tile_gather", B, H, W, Th, Tw, overlap_y, overlap_x, t0, n, &ay, &ax);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const TileStrides s{in_strides[0], in_strides[1], in_strides[2], in_strides[3]};
  const int64_t total = (int64_t)n * Th * ((Tw + 3) / 4);
  hipLaunchKernelGGL(tile_gather_kernel<false>, dim3(grid_for(total, 256, 1 << 20)), dim3(256), 0, (hipStream_t)hip_stream, (const void*)img_dev, s, C,
                     ay, ax, t0, total, 0, TileNorm{}, out_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_tile_gather_u8(mgu_ctx* c, const uint8_t* img_dev, int B, int H, int W, int bgr, const float* mean3, const float* std3, int Th, int Tw,
                       int overlap_y, int overlap_x, int t0, int n, float* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_dev || !out_dev || !mean3 || !std3 || !aligned16(out_dev))
    return fail(c, MGU_ERR_INVALID, "bad tile_gather_u8 args (null pointer or out_dev not 16-byte aligned)");
  TileAxis ay, ax;
  int rc = tile_check(c, "tile_gather_u8", B, H, W, Th, Tw, overlap_y, overlap_x, t0, n, &ay, &ax);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const TileNorm nm{{mean3[0], mean3[1], mean3[2]}, {std3[0], std3[1], std3[2]}};
  const int64_t total = (int64_t)n * Th * ((Tw + 3) / 4);
  hipLaunchKernelGGL(tile_gather_kernel<true>, dim3(grid_for(total, 256, 1 << 20)), dim3(256), 0, (hipStream_t)hip_stream, (const void*)img_dev,
                     TileStrides{}, 3, ay, ax, t0, total, bgr ? 1 : 0, nm, out_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_tile_accumulate(mgu_ctx* c, const float* tiles_dev, int is_prob, int B, int C, int H, int W, int Th, int Tw, int overlap_y, int overlap_x,
                        const float* wy_dev, const float* wx_dev, int t0, int n, float* acc_dev,
                        int64_t* labels_dev, float* conf_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!tiles_dev || !wy_dev || !wx_dev || !acc_dev || (!labels_dev) != (!conf_dev) || !aligned16(acc_dev))
    return fail(c, MGU_ERR_INVALID, "bad tile_accumulate args (null pointer, only one of labels_dev / conf_dev, or acc_dev not 16-byte aligned)");
  if (C < 1 || C > TILE_MAX_C) return fail(c, MGU_ERR_INVALID, "tile_accumulate: %d classes (at most %d)", C, TILE_MAX_C);
  TileAxis ay, ax;
  int rc = tile_check(c, "tile_accumulate", B, H, W, Th, Tw, overlap_y, overlap_x, t0, n, &ay, &ax);
  if (rc) return rc;
  ay.wn = wy_dev, ax.wn = wx_dev;
  // the rows the chunk can touch: those of its tile rows when it lies within one image, every row otherwise
  const int per = ay.n * ax.n, b0 = t0 / per, b1 = (t0 + n - 1) / per;
  int y0 = 0, y1 = H;
  if (b0 == b1) {
    y0 = tile_origin(ay, t0 / ax.n % ay.n);
    y1 = std::min(H, tile_origin(ay, (t0 + n - 1) / ax.n % ay.n) + Th);
  }
  const int px = (C == 2 && !(W & 1)) ? 2 : 1;
  const dim3 grid((W + 64 * px - 1) / (64 * px), (y1 - y0 + 3) / 4, b1 - b0 + 1);
  if (grid.y > 65535 || grid.z > 65535) return fail(c, MGU_ERR_INVALID, "tile_accumulate: the chunk spans too many rows or images for one launch");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  long long* lab = (long long*)labels_dev;
#define MGU_TILE_ACC(NC, PX)                                                                                                               \
  hipLaunchKernelGGL((tile_accumulate_kernel<NC, PX>), grid, dim3(256), 0, s, tiles_dev, is_prob ? 1 : 0, C, ay, ax, b0, y0, t0, n, acc_dev, lab, \
                     conf_dev)
  switch (C) {
    case 1: MGU_TILE_ACC(1, 1); break;
    case 2: if (px == 2) MGU_TILE_ACC(2, 2); else MGU_TILE_ACC(2, 1); break;
    case 3: MGU_TILE_ACC(3, 1); break;
    case 4: MGU_TILE_ACC(4, 1); break;
    default: MGU_TILE_ACC(0, 1); break;
  }
#undef MGU_TILE_ACC
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_tile_finish(mgu_ctx* c, const float* acc_dev, int B, int C, int H, int W, int64_t* labels_dev, float* conf_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!acc_dev || !labels_dev || !conf_dev || B < 1 || H < 1 || W < 1) return fail(c, MGU_ERR_INVALID, "bad tile_finish args (null pointer or B, H, W < 1)");
  if (C < 1 || C > TILE_MAX_C) return fail(c, MGU_ERR_INVALID, "tile_finish: %d classes (at most %d)", C, TILE_MAX_C);
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t npix = (int64_t)B * H * W;
  hipLaunchKernelGGL(tile_finish_kernel, dim3(grid_for(npix, 256, 1 << 20)), dim3(256), 0, (hipStream_t)hip_stream, acc_dev, npix, C,
                     (long long*)labels_dev, conf_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
