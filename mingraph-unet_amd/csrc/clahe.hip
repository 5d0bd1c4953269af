// Contrast-limited adaptive histogram equalisation (cv2.createCLAHE(clipLimit, tileGridSize).apply on 8-bit images) on the device, and
// its per-patch means for the equalised block of the node features:
//   mgu_clahe_u8              (B, H, W, 1 | 3) uint8 -> the same shape (3 channels: on Y of cv2's YUV, as equalize_histogram_rgb), two launches
//   mgu_patch_clahe_mean_u8   the means mgu_patch_mean_u8 gives on mgu_clahe_u8 of image b, bit for bit, two launches, no image written
// The arithmetic is THIS BUILD'S DEFINITION (include/mgunet.h spells it out): OpenCV's tile geometry with its
// reflect-101 extension, a clipped histogram per tile with the excess put back in closed form, a byte table per tile from the fp32
// product cumsum * (255 / area), and a bilinear blend of the four nearest tables in fp32 with every operation rounded on its own.  It
// follows OpenCV 4.x's clahe.cpp for 8-bit images; cv2 is not available to this build, so equality with an actual cv2 build is not
// verified.  hipcc contracts a * b + c by default, and a fused blend gives other bytes wherever the tile side is no power of two: the
// whole file is compiled under `#pragma clang fp contract(off)` (below; the _rn intrinsics do not prevent the fusion).
//
// Launch 1, clahe_lut_kernel: one workgroup per (image, tile).  A wave counts 64 extended pixels per step into its own 256-bin LDS
// histogram; the lanes that hold the same value are found with eight ballots (one per bit of the value) and only the lowest of them
// issues one LDS add of their count, so a uniform tile costs one add per wave step, not 64 serialised ones.  Then 256 threads, one per
// bin: the clip with a workgroup sum of the excess, the closed-form redistribution, an inclusive scan, the table.  The match is what
// this launch costs (vector ALU), whatever the data: see DESIGN.md section 5 for the forms that were measured.
// Launch 2, clahe_apply_kernel: x splits at the pixels where the left table changes into grid_x + 1 cell columns, likewise y; inside a
// cell every pixel blends the same four tables.  The host finds the cell borders with the kernel's own fp32 expression (it is monotone
// in x), so a pixel's cell is the one the definition gives it.  A workgroup owns a CL_CHUNK_H x CL_CHUNK_W chunk of one cell whose
// columns start at a multiple of 16 pixels: it stages the four tables as 256 dwords (byte k of word v: table k at value v -- one
// ds_read_b32 per pixel), the chunk's xa per column and ya per row, and every thread then makes 16 neighbouring pixels of one row,
// read and stored as 16-byte words where the row bytes and the pointers allow, else byte by byte (and always at a cell's ragged edge).
// The patch form computes the same expression per pixel from the tables in global memory (a patch may straddle cells) and adds up.
// Measured at 8 x 512^2, grid 8 x 8, clip 2.0 (tools/clahe_bench.py, profiles/clahe_bench.txt): both launches 18.9 us with 3 channels
// and 14.5 us with 1, the same on a uniform image, against 2.9 / 2.3 us for a device copy of the same bytes.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <cmath>

#include "imgmath.h"
#include "objects_common.h"

// No a * b + c of this file may become one fused operation.  __fmul_rn / __fadd_rn / __fsub_rn do not see to that: this toolchain defines
// them as the plain operators inside its own header, where contraction is allowed, and cl_axis written with them came out as
// v_fma_f32 (x, inv, -0.5) even under this pragma.  So the expressions are plain operators, and the pragma takes the `contract` flag off
// every one of them, on the device and in cl_axis_host; the integer divisions keep their own fused sequences (they are exact).
#pragma clang fp contract(off)

namespace mgu {
namespace {

constexpr int CL_THREADS = 256;                                     // both kernels; the table kernel has one thread per bin
static_assert(CL_THREADS == 256, "clahe_lut_kernel: a thread per bin, block_exclusive_scan over 256 threads");
constexpr int CL_MAX_GRID = 64;                                     // tiles per axis
constexpr int CL_LUT_UNROLL = 4;                                    // pixels a lane of the table kernel has in flight
constexpr int CL_VEC = 16;                                          // pixels a thread makes: one 16-byte word per channel
constexpr int CL_CHUNK_W = 64;                                      // pixels: 4 threads per chunk row
constexpr int CL_CHUNK_H = CL_THREADS / (CL_CHUNK_W / CL_VEC);      // 64 rows: one item per thread
constexpr int CL_MAX_PATCH = 64;                                    // as mgu_patch_node_features_u8
static_assert(CL_CHUNK_W % CL_VEC == 0 && CL_CHUNK_H * (CL_CHUNK_W / CL_VEC) == CL_THREADS, "one 16-pixel item per thread");

struct ClaheGeom {
  int H, W, gy, gx, th, tw, area;
  int clip;                              // largest count a bin keeps before the excess is put back; 0: no clipping
  float lut_scale, inv_th, inv_tw;       // 255 / area, 1 / th, 1 / tw: one fp32 division each, on the host
};
// first pixel of every cell column / row (the last entry is W / H), and the chunks a cell is cut into
struct ClaheCells {
  int xb[CL_MAX_GRID + 2], yb[CL_MAX_GRID + 2];
  int ncx, ncy;
};

template <int C>
__device__ __forceinline__ int cl_plane(const uint8_t* p) {
  if constexpr (C == 1) return p[0];
  int Y, U, V;
  cv_rgb2yuv(p, Y, U, V);
  return Y;
}

// position p on an axis with tiles of side 1 / inv: the lower table's index before clamping, and the weight of the upper table
__device__ __forceinline__ float cl_axis(int p, float inv, int& i1) {
  const float f = (float)p * inv - 0.5f, fl = floorf(f);
  i1 = (int)fl;
  return f - fl;
}
// the blend of the four table entries packed in w (byte 0: (ty1, tx1), 1: (ty1, tx2), 2: (ty2, tx1), 3: (ty2, tx2))
__device__ __forceinline__ int cl_blend(unsigned w, float xa, float ya) {
  const float xa1 = 1.0f - xa, ya1 = 1.0f - ya;
  const float top = (float)(w & 255u) * xa1 + (float)((w >> 8) & 255u) * xa;
  const float bot = (float)((w >> 16) & 255u) * xa1 + (float)(w >> 24) * xa;
  return sat8((int)rintf(top * ya1 + bot * ya));
}

// ---- launch 1: the table of one tile -----------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(CL_THREADS) void clahe_lut_kernel(const uint8_t* __restrict__ img, const ClaheGeom g, uint8_t* __restrict__ luts) {
  constexpr int WAVES = CL_THREADS / 64;
  __shared__ unsigned hist[WAVES][256];
  __shared__ int sh[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int tiles = g.gy * g.gx, b = blockIdx.x / tiles, t = blockIdx.x - b * tiles, ty = t / g.gx, tx = t - ty * g.gx;
#pragma unroll
  for (int k = 0; k < 256 / 64; ++k) hist[wave][k * 64 + lane] = 0;
  __syncthreads();
  const uint8_t* src = img + (size_t)b * g.H * g.W * C;
  const int y0 = ty * g.th, x0 = tx * g.tw;
  // pixel i of the tile is (i / tw, i % tw): one division for a lane's first pixel, then steps of CL_THREADS pixels
  const int dq = CL_THREADS / g.tw, dr = CL_THREADS - dq * g.tw;
  int ly = tid / g.tw, lx = tid - ly * g.tw;
  // the same trip count for every lane of a wave; CL_LUT_UNROLL pixels per lane are loaded before the first is counted
  for (unsigned base = wave * 64u; base < (unsigned)g.area; base += CL_THREADS * CL_LUT_UNROLL) {
    uint8_t px[CL_LUT_UNROLL][C];
    bool valid[CL_LUT_UNROLL];
#pragma unroll
    for (int u = 0; u < CL_LUT_UNROLL; ++u) {
      valid[u] = base + u * CL_THREADS + lane < (unsigned)g.area;       // a lane past the tile's end reads its first pixel and counts nothing
      const uint8_t* p = src + ((size_t)reflect101_loop(y0 + (valid[u] ? ly : 0), g.H) * g.W + reflect101_loop(x0 + (valid[u] ? lx : 0), g.W)) * C;
#pragma unroll
      for (int k = 0; k < C; ++k) px[u][k] = p[k];
      lx += dr, ly += dq;
      if (lx >= g.tw) lx -= g.tw, ++ly;
    }
#pragma unroll
    for (int u = 0; u < CL_LUT_UNROLL; ++u) {
      const int v = cl_plane<C>(px[u]);
      // the valid lanes that hold this lane's value: per bit of the value, the lanes whose bit equals this lane's.  Written on the
      // two halves of the mask with the bit spread over a word (0 or ~0): five instructions a bit, where `on ? m : ~m` on 64 bits took nine
      const unsigned long long ok = __ballot(valid[u]);
      unsigned lo = (unsigned)ok, hi = (unsigned)(ok >> 32);
#pragma unroll
      for (int bit = 0; bit < 8; ++bit) {
        const int on = (v << (31 - bit)) >> 31;
        const unsigned long long m = __ballot(on != 0);
        lo &= ~((unsigned)m ^ (unsigned)on), hi &= ~((unsigned)(m >> 32) ^ (unsigned)on);
      }
      const int first = lo ? __ffs((int)lo) - 1 : 31 + __ffs((int)hi);
      if (valid[u] && lane == first) atomicAdd(&hist[wave][v], (unsigned)(__popc(lo) + __popc(hi)));
    }
  }
  __syncthreads();
  int h = 0;                                              // one thread per bin from here on
#pragma unroll
  for (int w = 0; w < WAVES; ++w) h += (int)hist[w][tid];
  if (g.clip > 0) {
    int clipped = wave_sum(max(h - g.clip, 0));
    if (lane == 0) sh[wave] = clipped;
    __syncthreads();
    clipped = sh[0] + sh[1] + sh[2] + sh[3];
    __syncthreads();
    const int batch = clipped >> 8, residual = clipped & 255;
    h = min(h, g.clip) + batch;
    if (residual > 0) {                                   // OpenCV's loop i = 0, step, 2 step ... while residual lasts: all below 256
      const int step = max(256 / residual, 1), k = tid / step;
      if (k * step == tid && k < residual) ++h;
    }
  }
  int total;
  const int S = block_exclusive_scan(h, sh, &total) + h;
  luts[(size_t)blockIdx.x * 256 + tid] = (uint8_t)sat8((int)rintf((float)S * g.lut_scale));
}

// ---- launch 2: the blend, one workgroup per chunk of a cell ---------------------------------------------------------------------------------
// the 16 * C bytes of an item as dwords: byte j
template <int N>
__device__ __forceinline__ unsigned cl_byte(const unsigned (&w)[N], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }

template <int C>
__global__ __launch_bounds__(CL_THREADS) void clahe_apply_kernel(const uint8_t* img, uint8_t* out, const uint8_t* __restrict__ luts,
                                                                 const ClaheGeom g, const ClaheCells cells, int vec_in, int vec_out) {
  __shared__ unsigned tab[256];
  __shared__ __attribute__((aligned(16))) float sxa[CL_CHUNK_W];
  __shared__ float sya[CL_CHUNK_H];
  const int tid = threadIdx.x, b = blockIdx.y;
  int q = blockIdx.x;
  const int kx = q % cells.ncx;
  q /= cells.ncx;
  const int cx = q % (g.gx + 1);
  q /= g.gx + 1;
  const int ky = q % cells.ncy, cy = q / cells.ncy;
  const int cx0 = cells.xb[cx], cx1 = cells.xb[cx + 1], cy0 = cells.yb[cy], cy1 = cells.yb[cy + 1];
  const int ws = (cx0 & ~(CL_VEC - 1)) + kx * CL_CHUNK_W;                  // the chunk's window starts at a multiple of 16 pixels
  const int xs = max(cx0, ws), xe = min(cx1, ws + CL_CHUNK_W), ys = cy0 + ky * CL_CHUNK_H, ye = min(cy1, ys + CL_CHUNK_H);
  if (xs >= xe || ys >= ye) return;                                        // the whole workgroup
  {
    const int tx1 = max(cx - 1, 0), tx2 = min(cx, g.gx - 1), ty1 = max(cy - 1, 0), ty2 = min(cy, g.gy - 1);
    const uint8_t* lb = luts + (size_t)b * g.gy * g.gx * 256 + tid;
    tab[tid] = (unsigned)lb[(ty1 * g.gx + tx1) * 256] | ((unsigned)lb[(ty1 * g.gx + tx2) * 256] << 8) |
               ((unsigned)lb[(ty2 * g.gx + tx1) * 256] << 16) | ((unsigned)lb[(ty2 * g.gx + tx2) * 256] << 24);
    int unused;
    if (tid < CL_CHUNK_W) sxa[tid] = cl_axis(ws + tid, g.inv_tw, unused);
    else if (tid < CL_CHUNK_W + CL_CHUNK_H) sya[tid - CL_CHUNK_W] = cl_axis(ys + tid - CL_CHUNK_W, g.inv_th, unused);
  }
  __syncthreads();
  constexpr int GROUPS = CL_CHUNK_W / CL_VEC, NW = CL_VEC * C / 4;
  const int grp = tid % GROUPS, row = tid / GROUPS, y = ys + row, x0 = ws + grp * CL_VEC;
  if (y >= ye || x0 >= xe || x0 + CL_VEC <= xs) return;
  const bool full = x0 >= xs && x0 + CL_VEC <= xe;                         // else the cell's ragged edge: the neighbour cell owns the rest
  const size_t off = (((size_t)b * g.H + y) * g.W + x0) * C;
  unsigned pw[NW], ow[NW];
  if (full && vec_in) {
#pragma unroll
    for (int k = 0; k < C; ++k) {
      const uint4 u = reinterpret_cast<const uint4*>(img + off)[k];
      pw[4 * k] = u.x, pw[4 * k + 1] = u.y, pw[4 * k + 2] = u.z, pw[4 * k + 3] = u.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < NW; ++k) pw[k] = 0;
#pragma unroll
    for (int j = 0; j < CL_VEC * C; ++j)
      if (full || (x0 + j / C >= xs && x0 + j / C < xe)) pw[j >> 2] |= (unsigned)img[off + j] << (8 * (j & 3));
  }
  float xa[CL_VEC];
#pragma unroll
  for (int k = 0; k < CL_VEC / 4; ++k) {
    const float4 f = reinterpret_cast<const float4*>(sxa + grp * CL_VEC)[k];
    xa[4 * k] = f.x, xa[4 * k + 1] = f.y, xa[4 * k + 2] = f.z, xa[4 * k + 3] = f.w;
  }
  const float ya = sya[row];
#pragma unroll
  for (int k = 0; k < NW; ++k) ow[k] = 0;
#pragma unroll
  for (int e = 0; e < CL_VEC; ++e) {
    if constexpr (C == 1) {
      ow[e >> 2] |= (unsigned)cl_blend(tab[cl_byte(pw, e)], xa[e], ya) << (8 * (e & 3));
    } else {
      const uint8_t p[3] = {(uint8_t)cl_byte(pw, 3 * e), (uint8_t)cl_byte(pw, 3 * e + 1), (uint8_t)cl_byte(pw, 3 * e + 2)};
      int Y, U, V, r, gg, bb;
      cv_rgb2yuv(p, Y, U, V);
      cv_yuv2rgb(cl_blend(tab[Y], xa[e], ya), U, V, r, gg, bb);
      ow[(3 * e) >> 2] |= (unsigned)r << (8 * ((3 * e) & 3));
      ow[(3 * e + 1) >> 2] |= (unsigned)gg << (8 * ((3 * e + 1) & 3));
      ow[(3 * e + 2) >> 2] |= (unsigned)bb << (8 * ((3 * e + 2) & 3));
    }
  }
  if (full && vec_out) {
#pragma unroll
    for (int k = 0; k < C; ++k) reinterpret_cast<uint4*>(out + off)[k] = make_uint4(ow[4 * k], ow[4 * k + 1], ow[4 * k + 2], ow[4 * k + 3]);
  } else {
#pragma unroll
    for (int j = 0; j < CL_VEC * C; ++j)
      if (full || (x0 + j / C >= xs && x0 + j / C < xe)) out[off + j] = (uint8_t)cl_byte(ow, j);
  }
}

// ---- per-patch means of the equalised RGB image: one workgroup per patch --------------------------------------------------------------------
__global__ __launch_bounds__(CL_THREADS) void patch_clahe_mean_kernel(const uint8_t* __restrict__ rgb, const uint8_t* __restrict__ luts,
                                                                      const ClaheGeom g, int patch, int nph, int npw, int per_channel,
                                                                      float* __restrict__ out, int ld_out, int col0) {
  __shared__ unsigned red[CL_THREADS / 64][3];
  const int Np = nph * npw, b = blockIdx.x / Np, pidx = blockIdx.x - b * Np;
  const int py = pidx / npw, y0 = py * patch, x0 = (pidx - py * npw) * patch;
  const uint8_t* src = rgb + (size_t)b * g.H * g.W * 3;
  const uint8_t* lb = luts + (size_t)b * g.gy * g.gx * 256;
  unsigned s0 = 0, s1 = 0, s2 = 0;                         // R, G, B: at most 255 * 64 * 64 each; pad pixels are zeros in every sum
  for (int i = threadIdx.x; i < patch * patch; i += CL_THREADS) {
    const int ly = i / patch, y = y0 + ly, x = x0 + i - ly * patch;
    if (y >= g.H || x >= g.W) continue;
    int Y, U, V, tx1, ty1, r, gg, bb;
    cv_rgb2yuv(src + ((size_t)y * g.W + x) * 3, Y, U, V);
    const float xa = cl_axis(x, g.inv_tw, tx1), ya = cl_axis(y, g.inv_th, ty1);
    const int tx2 = min(tx1 + 1, g.gx - 1), ty2 = min(ty1 + 1, g.gy - 1);
    tx1 = max(tx1, 0), ty1 = max(ty1, 0);
    const unsigned w = (unsigned)lb[(ty1 * g.gx + tx1) * 256 + Y] | ((unsigned)lb[(ty1 * g.gx + tx2) * 256 + Y] << 8) |
                       ((unsigned)lb[(ty2 * g.gx + tx1) * 256 + Y] << 16) | ((unsigned)lb[(ty2 * g.gx + tx2) * 256 + Y] << 24);
    cv_yuv2rgb(cl_blend(w, xa, ya), U, V, r, gg, bb);
    s0 += r, s1 += gg, s2 += bb;
  }
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][0] = s0, red[threadIdx.x >> 6][1] = s1, red[threadIdx.x >> 6][2] = s2;
  __syncthreads();
  const int nout = per_channel ? 3 : 1;
  if ((int)threadIdx.x < nout) {
    unsigned acc = 0;                                      // patch_mean_u8_kernel's sum and its mean expression
    for (int w = 0; w < CL_THREADS / 64; ++w)
      for (int c = 0; c < 3; ++c)
        if (!per_channel || c == (int)threadIdx.x) acc += red[w][c];
    out[(size_t)blockIdx.x * ld_out + col0 + threadIdx.x] = (float)((double)acc / ((double)patch * patch * (per_channel ? 1 : 3)));
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------
// floor(fl(fl(p * inv) - 0.5)) as cl_axis forms it: each operation rounded to fp32 on its own
int cl_axis_host(int p, float inv) {
  volatile float m = (float)p * inv;
  volatile float f = m - 0.5f;
  return (int)floorf(f);
}
// b[c], c = 0 .. tiles + 1: the first position of [0, n) whose unclamped lower table is >= c - 1 (the expression is monotone in p)
void cl_borders(int n, int t, float inv, int tiles, int* b) {
  b[0] = 0;
  for (int c = 1; c <= tiles; ++c) {
    int64_t p = ((int64_t)(2 * c - 1) * t + 1) / 2;       // ceil((c - 1/2) t): the border in exact arithmetic
    if (p > n) p = n;
    while (p > 0 && cl_axis_host((int)p - 1, inv) >= c - 1) --p;
    while (p < n && cl_axis_host((int)p, inv) < c - 1) ++p;
    b[c] = (int)p;
  }
  b[tiles + 1] = n;
}

// the checked geometry of a call
int cl_geometry(mgu_ctx* c, const char* fn, int B, int H, int W, int grid_y, int grid_x, double clip_limit, ClaheGeom* g) {
  if (B < 1 || H < 1 || W < 1) return mgud::fail(c, MGU_ERR_INVALID, "%s: B, H, W must be >= 1", fn);
  if (B > 65535) return mgud::fail(c, MGU_ERR_INVALID, "%s: B must stay at or below 65535", fn);
  if (grid_y < 1 || grid_y > CL_MAX_GRID || grid_x < 1 || grid_x > CL_MAX_GRID)
    return mgud::fail(c, MGU_ERR_INVALID, "%s: a grid of %d x %d tiles (1..%d per axis)", fn, grid_y, grid_x, CL_MAX_GRID);
  if (!std::isfinite(clip_limit)) return mgud::fail(c, MGU_ERR_INVALID, "%s: clip_limit must be finite", fn);
  if ((int64_t)H * W > INT_MAX) return mgud::fail(c, MGU_ERR_INVALID, "%s: H * W must stay below 2^31", fn);
  int64_t He = H, We = W;
  if (H % grid_y || W % grid_x) He = H + grid_y - H % grid_y, We = W + grid_x - W % grid_x;      // OpenCV extends both axes
  const int64_t th = He / grid_y, tw = We / grid_x;
  if (th * tw > INT_MAX) return mgud::fail(c, MGU_ERR_INVALID, "%s: a tile of %lld x %lld pixels (below 2^31)", fn, (long long)th, (long long)tw);
  memset(g, 0, sizeof *g);
  g->H = H, g->W = W, g->gy = grid_y, g->gx = grid_x, g->th = (int)th, g->tw = (int)tw, g->area = (int)(th * tw);
  if (clip_limit > 0.0) {
    const double cl = clip_limit * (double)g->area / 256.0;
    g->clip = cl >= (double)g->area ? g->area : std::max(1, (int)cl);   // no bin holds more than area: a larger limit clips nothing
  }
  g->lut_scale = 255.0f / (float)g->area;
  g->inv_th = 1.0f / (float)g->th, g->inv_tw = 1.0f / (float)g->tw;
  return MGU_OK;
}

bool cl_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uint8_t *p = (const uint8_t*)a, *q = (const uint8_t*)b;
  return p < q + nb && q < p + na;
}

// launch 1 into luts (B, gy, gx, 256)
void cl_tables(mgu_ctx* c, const uint8_t* img, int B, int channels, const ClaheGeom& g, uint8_t* luts, hipStream_t s) {
  mgud::ProfScope ps(c, s, "clahe_lut_kernel", 0, 0, -1);
  const dim3 grid((unsigned)(B * g.gy * g.gx)), block(CL_THREADS);
  if (channels == 1) hipLaunchKernelGGL(clahe_lut_kernel<1>, grid, block, 0, s, img, g, luts);
  else hipLaunchKernelGGL(clahe_lut_kernel<3>, grid, block, 0, s, img, g, luts);
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_clahe_u8(mgu_ctx* c, const uint8_t* img_dev, int B, int H, int W, int channels, int grid_y, int grid_x, double clip_limit,
                 uint8_t* out_dev, uint8_t* luts_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!img_dev || !out_dev) return fail(c, MGU_ERR_INVALID, "clahe: the image and the output are needed");
  if (channels != 1 && channels != 3) return fail(c, MGU_ERR_INVALID, "clahe: %d channels (1 or 3)", channels);
  ClaheGeom g;
  if (int rc = cl_geometry(c, "clahe", B, H, W, grid_y, grid_x, clip_limit, &g)) return rc;
  const size_t bytes = (size_t)B * H * W * channels, lut_bytes = (size_t)B * grid_y * grid_x * 256;
  if (out_dev != img_dev && cl_overlap(img_dev, bytes, out_dev, bytes))
    return fail(c, MGU_ERR_INVALID, "clahe: the output must be the input itself or not alias it");
  if (luts_dev && (cl_overlap(luts_dev, lut_bytes, img_dev, bytes) || cl_overlap(luts_dev, lut_bytes, out_dev, bytes)))
    return fail(c, MGU_ERR_INVALID, "clahe: the tables must not alias the images");
  ClaheCells cells;
  memset(&cells, 0, sizeof cells);
  cl_borders(W, g.tw, g.inv_tw, grid_x, cells.xb);
  cl_borders(H, g.th, g.inv_th, grid_y, cells.yb);
  int64_t ncx = 1, ncy = 1;
  for (int i = 0; i <= grid_x; ++i)
    ncx = std::max<int64_t>(ncx, ((int64_t)cells.xb[i + 1] - (cells.xb[i] & ~(CL_VEC - 1)) + CL_CHUNK_W - 1) / CL_CHUNK_W);
  for (int i = 0; i <= grid_y; ++i) ncy = std::max<int64_t>(ncy, ((int64_t)cells.yb[i + 1] - cells.yb[i] + CL_CHUNK_H - 1) / CL_CHUNK_H);
  const int64_t blocks = ncx * (grid_x + 1) * ncy * (grid_y + 1);
  if (blocks > INT_MAX) return fail(c, MGU_ERR_INVALID, "clahe: %lld chunks (below 2^31)", (long long)blocks);
  cells.ncx = (int)ncx, cells.ncy = (int)ncy;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (!luts_dev) {
    if (int rc = ensure(c, &c->imgws, &c->imgws_bytes, lut_bytes)) return rc;
    luts_dev = (uint8_t*)c->imgws;
  }
  cl_tables(c, img_dev, B, channels, g, luts_dev, s);
  const int row16 = ((size_t)W * channels) % 16 == 0;
  const int vec_in = row16 && ((uintptr_t)img_dev & 15) == 0, vec_out = row16 && ((uintptr_t)out_dev & 15) == 0;
  const dim3 grid((unsigned)blocks, (unsigned)B), block(CL_THREADS);
  {
    ProfScope ps(c, s, "clahe_apply_kernel", 0, 0, -1);
    if (channels == 1) hipLaunchKernelGGL(clahe_apply_kernel<1>, grid, block, 0, s, img_dev, out_dev, luts_dev, g, cells, vec_in, vec_out);
    else hipLaunchKernelGGL(clahe_apply_kernel<3>, grid, block, 0, s, img_dev, out_dev, luts_dev, g, cells, vec_in, vec_out);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_patch_clahe_mean_u8(mgu_ctx* c, const uint8_t* rgb_dev, int B, int H, int W, int patch, int grid_y, int grid_x, double clip_limit,
                            int per_channel, float* out_dev, int ld_out, int col0, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!rgb_dev || !out_dev || patch < 1 || patch > CL_MAX_PATCH)
    return fail(c, MGU_ERR_INVALID, "bad patch_clahe_mean args (the image, the rows, patch 1..%d)", CL_MAX_PATCH);
  ClaheGeom g;
  if (int rc = cl_geometry(c, "patch_clahe_mean", B, H, W, grid_y, grid_x, clip_limit, &g)) return rc;
  const int nph = (H + patch - 1) / patch, npw = (W + patch - 1) / patch;
  const int64_t rows = (int64_t)B * nph * npw;
  if (rows > INT_MAX) return fail(c, MGU_ERR_INVALID, "patch_clahe_mean: B * patches must stay below 2^31");
  const int nout = per_channel ? 3 : 1;
  if (col0 < 0 || (int64_t)col0 + nout > ld_out)
    return fail(c, MGU_ERR_INVALID, "patch_clahe_mean: columns [%d, %d) outside rows of %d", col0, col0 + nout, ld_out);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (int rc = ensure(c, &c->imgws, &c->imgws_bytes, (size_t)B * grid_y * grid_x * 256)) return rc;
  uint8_t* luts = (uint8_t*)c->imgws;
  cl_tables(c, rgb_dev, B, 3, g, luts, s);
  {
    ProfScope ps(c, s, "patch_clahe_mean_kernel", 0, 0, -1);
    hipLaunchKernelGGL(patch_clahe_mean_kernel, dim3((unsigned)rows), dim3(CL_THREADS), 0, s, rgb_dev, luts, g, patch, nph, npw,
                       per_channel ? 1 : 0, out_dev, ld_out, col0);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
