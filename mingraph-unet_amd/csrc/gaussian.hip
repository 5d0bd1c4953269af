// GaussianSmoother.smooth (preprocessing/graph_feature_processing/gaussian_smoothing.py:23-34: cv2.GaussianBlur on uint8) on the device,
// and its per-patch means for the node features of scripts/graph_refinement.py:81 ("Sobel, HistEq, Smooth per patch"):
//   mgu_gaussian_blur_u8       (B, H, W, 1..4) uint8 -> the same shape, one launch, no workspace
//   mgu_patch_smooth_mean_u8   the means mgu_patch_mean_u8 gives on mgu_gaussian_blur_u8 of image b, bit for bit, one launch, no image written
// The arithmetic is THIS BUILD'S DEFINITION (include/mgunet.h spells it out): separable Q8.8 integer weights that sum to 256 per axis
// (the host quantises them with error diffusion: mgunet.preprocess.gaussian_kernel_q8), a horizontal pass into 16 bits, a vertical pass,
// (v + 32768) >> 16, reflect-101 borders applied until the index is inside.  It follows the fixed-point scheme OpenCV 4.x publishes for
// 8-bit images; cv2 is not available to this build, so equality with an actual cv2 build is not verified.  No floating point runs on the
// device: the result is bitwise reproducible.
//
// Both kernels are one workgroup per tile (per patch): the tile with its ry / rx halo is staged as bytes in LDS -- border indices
// are resolved there -- the horizontal pass fills a 16-bit LDS plane, the vertical pass reads it.  A row of the tile is a run of
// pixels * channels bytes, and both passes work on those bytes: tap d of the horizontal pass is the byte d * channels further on.
//   horizontal  a thread makes 8 neighbouring sums: per tap three aligned LDS dwords, v_alignbyte to the tap's offset, and two sums per
//               multiply -- a row sum is at most 255 * 256 = 65280, so two of them share a register without a carry
//   vertical    a thread makes 16 neighbouring bytes of one output row (two ds_read_b128 per tap) and stores them as one 16-byte word
//               where the address allows (W * channels a multiple of 16), else byte by byte; the patch form adds them up instead
// The weights travel in the kernel arguments (uniform index: scalar loads).  LDS is sized per launch from the taps, so a 5 x 5 blur
// keeps 6-7 workgroups on a CU where 31 x 31 keeps two.
// Measured at 8 x 512^2 x 3 (tools/gaussian_blur_bench.py, profiles/gaussian_blur_bench.txt): 17 us at 5 x 5, 70 us at 31 x 31, against
// 2.7 us for a device copy of the same bytes -- the integer work of the passes sets the time, not memory.  The multiplies are written
// as __umul24 (both factors fit 24 bits): plain 32-bit products compile to the quarter-rate v_mul_lo_u32 / v_mad_u64_u32.  Staging rows
// that need no reflection as plain byte runs was tried and dropped: 2 % on the blur, and its registers took the patch kernel from 28
// to 36 us.
#include <limits.h>

#include "ctx.h"
#include "imgmath.h"

namespace mgu {
namespace {

constexpr int GS_THREADS = 256;
constexpr int GS_MAX_K = 31;                                        // taps per axis: radius <= 15
constexpr int GS_TH = 32;                                           // tile height, every channel count
__host__ __device__ constexpr int gs_tile_w(int C) { return C == 3 ? 64 : 256 / C; }   // tile rows of 256 bytes (192 for 3 channels)
constexpr int GS_MAX_PATCH = 64;                                    // as mgu_patch_node_features_u8

// LDS layout of a (rows + 2 ry) x (cols + 2 rx) window of C-channel pixels: the byte plane (row pitch a multiple of 4; 16 spare bytes:
// the horizontal pass reads whole dwords past its last tap), then the 16-bit plane (row pitch a multiple of 8 values)
__host__ __device__ constexpr int gs_s_pitch(int cols, int rx, int C) { return ((cols + 2 * rx) * C + 3) & ~3; }
__host__ __device__ constexpr int gs_h_pitch(int cols, int C) { return (cols * C + 7) & ~7; }
__host__ __device__ constexpr int gs_h_offset(int rows, int cols, int ry, int rx, int C) {
  return (gs_s_pitch(cols, rx, C) * (rows + 2 * ry) + 16 + 15) & ~15;
}
__host__ __device__ constexpr int gs_lds_bytes(int rows, int cols, int ry, int rx, int C) {
  return gs_h_offset(rows, cols, ry, rx, C) + gs_h_pitch(cols, C) * 2 * (rows + 2 * ry);
}
constexpr int GS_R = GS_MAX_K / 2;
static_assert(gs_lds_bytes(GS_TH, gs_tile_w(1), GS_R, GS_R, 1) <= 65536 && gs_lds_bytes(GS_TH, gs_tile_w(2), GS_R, GS_R, 2) <= 65536 &&
                  gs_lds_bytes(GS_TH, gs_tile_w(3), GS_R, GS_R, 3) <= 65536 && gs_lds_bytes(GS_TH, gs_tile_w(4), GS_R, GS_R, 4) <= 65536,
              "the blur tile with a 31 x 31 halo must fit the 64 KiB of LDS a workgroup can have");
static_assert(gs_lds_bytes(GS_MAX_PATCH, GS_MAX_PATCH, GS_R, GS_R, 3) <= 65536, "a 64 x 64 RGB patch with a 31 x 31 halo must fit 64 KiB of LDS");
static_assert(gs_tile_w(1) * 1 % 16 == 0 && gs_tile_w(2) * 2 % 16 == 0 && gs_tile_w(3) * 3 % 16 == 0 && gs_tile_w(4) * 4 % 16 == 0,
              "tile rows are whole 16-byte words");

struct GaussTaps {          // Q8.8 weights of the two axes, each summing to 256
  int kx[GS_MAX_K], ky[GS_MAX_K];
  int kw, kh;
};

// the window rows [y0 - ry, y0 - ry + rows) x pixels [x0 - rx, x0 - rx + cols) of one image into S (row pitch sp), borders reflected
template <int C>
__device__ __forceinline__ void gs_stage(const uint8_t* __restrict__ img, int H, int W, int y0, int x0, int rows, int cols, int ry, int rx,
                                         uint8_t* S, int sp) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ne = cols * C;
  for (int r = wave; r < rows; r += GS_THREADS / 64) {
    const uint8_t* src = img + (size_t)reflect101_loop(y0 - ry + r, H) * W * C;
    for (int e = lane; e < ne; e += 64) {
      const int q = e / C, c = e - q * C;
      S[r * sp + e] = src[(size_t)reflect101_loop(x0 - rx + q, W) * C + c];
    }
  }
}

// Hp[r][j] = sum_d kx[d] * S[r][j + d * C] for the `rows` staged rows and j < nb rounded up to 8 (the surplus is never read as a result)
template <int C>
__device__ __forceinline__ void gs_hpass(const uint8_t* S, int sp, int rows, int nb, const GaussTaps& t, uint16_t* Hp, int hp) {
  const int ncr = (nb + 7) >> 3, total = rows * ncr;
  const unsigned* S32 = reinterpret_cast<const unsigned*>(S);
  for (int i = threadIdx.x; i < total; i += GS_THREADS) {
    const int r = i / ncr, cj = i - r * ncr;
    const unsigned* row = S32 + r * (sp >> 2);
    unsigned a02 = 0, a13 = 0, a46 = 0, a57 = 0;          // sums of bytes 0 | 2, 1 | 3, 4 | 6, 5 | 7 in the low | high half
    for (int d = 0; d < t.kw; ++d) {
      const int base = cj * 8 + d * C;
      const unsigned* p = row + (base >> 2);
      const unsigned sh = base & 3, w0 = p[0], w1 = p[1], w2 = p[2];
      const unsigned lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
      const unsigned k = (unsigned)t.kx[d];
      a02 += __umul24(k, lo & 0x00ff00ffu);               // both factors fit 24 bits and the product 32: the full-rate multiply
      a13 += __umul24(k, (lo >> 8) & 0x00ff00ffu);
      a46 += __umul24(k, hi & 0x00ff00ffu);
      a57 += __umul24(k, (hi >> 8) & 0x00ff00ffu);
    }
    uint4 o;
    o.x = (a02 & 0xffffu) | (a13 << 16);
    o.y = (a02 >> 16) | (a13 & 0xffff0000u);
    o.z = (a46 & 0xffffu) | (a57 << 16);
    o.w = (a46 >> 16) | (a57 & 0xffff0000u);
    *reinterpret_cast<uint4*>(Hp + r * hp + cj * 8) = o;
  }
}

// the N blurred bytes of output row ly (row ly + d of the 16-bit plane under tap d) at plane columns [j, j + N), j a multiple of N
template <int N>
__device__ __forceinline__ void gs_vchunk(const uint16_t* Hp, int hp, int ly, int j, const GaussTaps& t, unsigned (&v)[N]) {
  static_assert(N == 4 || N % 8 == 0, "4 values (one 8-byte read) or whole 16-byte reads");
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = 0;
  for (int d = 0; d < t.kh; ++d) {
    const uint16_t* p = Hp + (ly + d) * hp + j;
    const unsigned k = (unsigned)t.ky[d];
    unsigned w[N / 2];
    if constexpr (N == 4) {
      const uint2 u = *reinterpret_cast<const uint2*>(p);
      w[0] = u.x, w[1] = u.y;
    } else {
#pragma unroll
      for (int q = 0; q < N / 8; ++q) {
        const uint4 u = reinterpret_cast<const uint4*>(p)[q];
        w[4 * q] = u.x, w[4 * q + 1] = u.y, w[4 * q + 2] = u.z, w[4 * q + 3] = u.w;
      }
    }
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      v[2 * i] += __umul24(k, w[i] & 0xffffu);
      v[2 * i + 1] += __umul24(k, w[i] >> 16);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = (v[i] + 32768u) >> 16;      // at most 255: the weights of an axis sum to 256
}

// ---- the blur: one workgroup per GS_TH x gs_tile_w(C) tile of one image ------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(GS_THREADS) void gaussian_blur_kernel(const uint8_t* __restrict__ img, uint8_t* __restrict__ out, int H, int W,
                                                                   int tiles_x, int tiles_per_img, const GaussTaps t) {
  constexpr int TW = gs_tile_w(C);
  extern __shared__ __attribute__((aligned(16))) uint8_t gs_lds[];
  const int b = blockIdx.x / tiles_per_img, tile = blockIdx.x - b * tiles_per_img;
  const int ty = tile / tiles_x, y0 = ty * GS_TH, x0 = (tile - ty * tiles_x) * TW;
  const int th = min(GS_TH, H - y0), tw = min(TW, W - x0), rx = t.kw >> 1, ry = t.kh >> 1;
  const int sp = gs_s_pitch(TW, rx, C), hp = gs_h_pitch(TW, C);
  uint8_t* S = gs_lds;
  uint16_t* Hp = reinterpret_cast<uint16_t*>(gs_lds + gs_h_offset(GS_TH, TW, ry, rx, C));
  const size_t ibase = (size_t)b * H * W * C;
  gs_stage<C>(img + ibase, H, W, y0, x0, th + 2 * ry, tw + 2 * rx, ry, rx, S, sp);
  __syncthreads();
  const int nb = tw * C;                                   // bytes of a tile row inside the image
  gs_hpass<C>(S, sp, th + 2 * ry, nb, t, Hp, hp);
  __syncthreads();
  const int ncr = (nb + 15) >> 4, total = th * ncr;
  for (int i = threadIdx.x; i < total; i += GS_THREADS) {
    const int ly = i / ncr, j = (i - ly * ncr) * 16;
    unsigned v[16];
    gs_vchunk<16>(Hp, hp, ly, j, t, v);
    uint8_t* o = out + ibase + ((size_t)(y0 + ly) * W + x0) * C + j;
    if (j + 16 <= nb && ((uintptr_t)o & 15) == 0) {
      uint4 q;
      q.x = v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24);
      q.y = v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24);
      q.z = v[8] | (v[9] << 8) | (v[10] << 16) | (v[11] << 24);
      q.w = v[12] | (v[13] << 8) | (v[14] << 16) | (v[15] << 24);
      *reinterpret_cast<uint4*>(o) = q;
    } else {
#pragma unroll
      for (int e = 0; e < 16; ++e)
        if (j + e < nb) o[e] = (uint8_t)v[e];
    }
  }
}

// ---- per-patch means of the blurred RGB image: one workgroup per patch ----------------------------------------------------------------------
__global__ __launch_bounds__(GS_THREADS) void patch_smooth_mean_kernel(const uint8_t* __restrict__ rgb, int H, int W, int patch, int nph, int npw,
                                                                       int per_channel, float* __restrict__ out, int ld_out, int col0,
                                                                       const GaussTaps t) {
  extern __shared__ __attribute__((aligned(16))) uint8_t gs_lds[];
  __shared__ unsigned red[GS_THREADS / 64][3];
  const int Np = nph * npw, b = blockIdx.x / Np, pidx = blockIdx.x - b * Np;
  const int py = pidx / npw, y0 = py * patch, x0 = (pidx - py * npw) * patch;
  const int ph = min(patch, H - y0), pw = min(patch, W - x0), rx = t.kw >> 1, ry = t.kh >> 1;   // pad pixels are zeros in every sum
  const int sp = gs_s_pitch(patch, rx, 3), hp = gs_h_pitch(patch, 3);
  uint8_t* S = gs_lds;
  uint16_t* Hp = reinterpret_cast<uint16_t*>(gs_lds + gs_h_offset(patch, patch, ry, rx, 3));
  gs_stage<3>(rgb + (size_t)b * H * W * 3, H, W, y0, x0, ph + 2 * ry, pw + 2 * rx, ry, rx, S, sp);
  __syncthreads();
  const int nb = pw * 3;
  gs_hpass<3>(S, sp, ph + 2 * ry, nb, t, Hp, hp);
  __syncthreads();
  unsigned s0 = 0, s1 = 0, s2 = 0;                         // R, G, B: at most 255 * 64 * 64 each
  const int ncr = (nb + 3) >> 2, total = ph * ncr;
  for (int i = threadIdx.x; i < total; i += GS_THREADS) {
    const int ly = i / ncr, j = (i - ly * ncr) * 4;
    unsigned v[4];
    gs_vchunk<4>(Hp, hp, ly, j, t, v);
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (j + e >= nb) v[e] = 0;
    const unsigned t0 = v[0] + v[3], t1 = v[1], t2 = v[2];   // bytes of channel c0, c0 + 1, c0 + 2 (mod 3), c0 = j mod 3
    const int c0 = j % 3;
    s0 += c0 == 0 ? t0 : (c0 == 1 ? t2 : t1);
    s1 += c0 == 0 ? t1 : (c0 == 1 ? t0 : t2);
    s2 += c0 == 0 ? t2 : (c0 == 1 ? t1 : t0);
  }
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = s0, red[threadIdx.x >> 6][1] = s1, red[threadIdx.x >> 6][2] = s2;
  __syncthreads();
  const int nout = per_channel ? 3 : 1;
  if ((int)threadIdx.x < nout) {
    unsigned acc = 0;                                      // patch_mean_u8_kernel's sum and its mean expression
    for (int w = 0; w < GS_THREADS / 64; ++w)
      for (int c = 0; c < 3; ++c)
        if (!per_channel || c == (int)threadIdx.x) acc += red[w][c];
    out[(size_t)blockIdx.x * ld_out + col0 + threadIdx.x] = (float)((double)acc / ((double)patch * patch * (per_channel ? 1 : 3)));
  }
}

// the taps of a call, checked: odd sizes 1..31, weights >= 0 that sum to 256 per axis
int gs_taps(mgu_ctx* c, const char* fn, const int32_t* kx, int kw, const int32_t* ky, int kh, GaussTaps* t) {
  if (!kx || !ky || kw < 1 || kh < 1 || kw > GS_MAX_K || kh > GS_MAX_K || !(kw & 1) || !(kh & 1))
    return mgud::fail(c, MGU_ERR_INVALID, "%s: kernel sizes %d x %d (odd, 1..%d, with their weights)", fn, kw, kh, GS_MAX_K);
  memset(t, 0, sizeof *t);
  t->kw = kw, t->kh = kh;
  for (int axis = 0; axis < 2; ++axis) {
    const int32_t* k = axis ? ky : kx;
    const int n = axis ? kh : kw;
    int64_t sum = 0;
    for (int i = 0; i < n; ++i) {
      if (k[i] < 0 || k[i] > 256) return mgud::fail(c, MGU_ERR_INVALID, "%s: weight %d of the %s axis is %d (0..256)", fn, i, axis ? "y" : "x", k[i]);
      sum += k[i];
      (axis ? t->ky : t->kx)[i] = k[i];
    }
    if (sum != 256) return mgud::fail(c, MGU_ERR_INVALID, "%s: the %s weights sum to %lld, not 256", fn, axis ? "y" : "x", (long long)sum);
  }
  return MGU_OK;
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_gaussian_blur_u8(mgu_ctx* c, const uint8_t* img_dev, int B, int H, int W, int channels, const int32_t* kx_host, int kw,
                         const int32_t* ky_host, int kh, uint8_t* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_dev || !out_dev || B < 1 || H < 1 || W < 1 || channels < 1 || channels > 4)
    return fail(c, MGU_ERR_INVALID, "bad gaussian_blur args (B, H, W >= 1, 1..4 channels)");
  GaussTaps t;
  if (int rc = gs_taps(c, "gaussian_blur", kx_host, kw, ky_host, kh, &t)) return rc;
  if ((int64_t)H * W > INT_MAX) return fail(c, MGU_ERR_INVALID, "gaussian_blur: H * W must stay below 2^31");
  const int TW = gs_tile_w(channels);
  const int tiles_x = (W + TW - 1) / TW, tiles = tiles_x * ((H + GS_TH - 1) / GS_TH);
  if ((int64_t)B * tiles > INT_MAX) return fail(c, MGU_ERR_INVALID, "gaussian_blur: B * tiles must stay below 2^31");
  const size_t bytes = (size_t)B * H * W * channels;
  if (img_dev < out_dev + bytes && out_dev < img_dev + bytes) return fail(c, MGU_ERR_INVALID, "gaussian_blur: the output must not alias the input");
  HIPCHK(c, hipSetDevice(c->device));
  const dim3 grid((unsigned)(B * tiles)), block(GS_THREADS);
  const size_t lds = (size_t)gs_lds_bytes(GS_TH, TW, kh >> 1, kw >> 1, channels);
  hipStream_t s = (hipStream_t)hip_stream;
#define MGU_GS(CH) hipLaunchKernelGGL(gaussian_blur_kernel<CH>, grid, block, lds, s, img_dev, out_dev, H, W, tiles_x, tiles, t)
  switch (channels) {
    case 1: MGU_GS(1); break;
    case 2: MGU_GS(2); break;
    case 3: MGU_GS(3); break;
    default: MGU_GS(4); break;
  }
#undef MGU_GS
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_patch_smooth_mean_u8(mgu_ctx* c, const uint8_t* rgb_dev, int B, int H, int W, int patch, const int32_t* kx_host, int kw,
                             const int32_t* ky_host, int kh, int per_channel, float* out_dev, int ld_out, int col0, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!rgb_dev || !out_dev || B < 1 || H < 1 || W < 1 || patch < 1 || patch > GS_MAX_PATCH)
    return fail(c, MGU_ERR_INVALID, "bad patch_smooth_mean args (B, H, W >= 1, patch 1..%d)", GS_MAX_PATCH);
  GaussTaps t;
  if (int rc = gs_taps(c, "patch_smooth_mean", kx_host, kw, ky_host, kh, &t)) return rc;
  if ((int64_t)H * W > INT_MAX) return fail(c, MGU_ERR_INVALID, "patch_smooth_mean: H * W must stay below 2^31");
  const int nph = (H + patch - 1) / patch, npw = (W + patch - 1) / patch;
  const int64_t rows = (int64_t)B * nph * npw;
  if (rows > INT_MAX) return fail(c, MGU_ERR_INVALID, "patch_smooth_mean: B * patches must stay below 2^31");
  const int nout = per_channel ? 3 : 1;
  if (col0 < 0 || (int64_t)col0 + nout > ld_out)
    return fail(c, MGU_ERR_INVALID, "patch_smooth_mean: columns [%d, %d) outside rows of %d", col0, col0 + nout, ld_out);
  HIPCHK(c, hipSetDevice(c->device));
  const size_t lds = (size_t)gs_lds_bytes(patch, patch, kh >> 1, kw >> 1, 3);
  hipLaunchKernelGGL(patch_smooth_mean_kernel, dim3((unsigned)rows), dim3(GS_THREADS), lds, (hipStream_t)hip_stream, rgb_dev, H, W, patch, nph, npw,
                     per_channel ? 1 : 0, out_dev, ld_out, col0, t);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
