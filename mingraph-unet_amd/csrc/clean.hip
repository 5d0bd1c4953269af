// Mask cleanup on the device, between "argmax" and "label": close gaps, fill holes, open away spurs (include/mgunet.h states the
// definitions).  Integer and bit arithmetic only: bitwise repeatable.
//   mgu_clean_masks   int64 class map (B, H, W) or NHWC fp32 logits (argmax fused) -> int64 class map (B, H, W), pixel counts (B, 3)
// Close and open are bit-plane morphology (morph_kernel).  A workgroup owns a tile of 32 rows x 128 pixels with a halo of 2r rows
// and one 64-pixel word per side; the classes of the haloed tile sit in LDS as bytes.  For every class present in the tile, a wave's
// __ballot over a row segment gives one 64-bit word of that class's plane, and the disc is applied as row runs: with
// h(s) = floor(sqrt(r2 - s^2)), X (+) D = OR over s = 0..r of (OR of the rows |dy| <= h(s)) shifted by +s and -s, the shifts carrying
// bits between neighbouring words; erosion is the same with AND.  Two such passes (dilate, erode for the closing; erode, dilate for the
// opening) and the tile's result is written once.
// Fill labels the background of the class map with objects.hip's union-find (cc_roots_i32, 4-neighbours), keeps two counters per
// root -- area, and a word whose bit 0 says "touches the image border" and whose bit c says "has a 4-neighbour of class c" (one
// atomicOr stands for the border flag and the min and max neighbouring class: a hole has exactly one class bit and no border bit)
// -- and an apply pass writes the result.  The runs of one root are combined inside the wave first (wave_by_key): the outer
// background is one component holding most of the image.
// Between the stages the class map is uint8 (classes <= 31) in the context's scratch.  The launch count is fixed: it depends on
// no size, class count or hole count.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int CL_THREADS = 256;
constexpr int CL_MAX_R = 8;                            // floor(sqrt(64)): the largest disc radius
constexpr int CL_TW = 2;                               // tile: CL_TW words of 64 pixels ...
constexpr int CL_TH = 32;                              // ... by CL_TH rows
constexpr int CL_WW = CL_TW + 2;                       // words of a haloed tile row
constexpr int CL_ROWS = CL_TH + 4 * CL_MAX_R;          // rows of the largest haloed tile
constexpr int CL_PX = CL_WW * 64;                      // pixels of a haloed tile row
static_assert(CL_THREADS == CL_PX, "a thread owns one column of the haloed tile while it is loaded");
static_assert(2 * CL_MAX_R <= 64, "the halo of 2r pixels fits the one halo word");

typedef unsigned long long u64;

// the disc D(r2) as row runs: r = floor(sqrt(r2)), h[s] = floor(sqrt(r2 - s^2)) for s = 0..r (host-built)
struct Disc {
  int r;
  signed char h[CL_MAX_R + 1];
};

// bits of the 64-pixel word starting at x = xw of row y that lie inside the image
__device__ __forceinline__ u64 inside_word(int y, int xw, int H, int W) {
  if (y < 0 || y >= H) return 0;
  const int lo = max(0, -xw), hi = min(64, W - xw);
  if (hi <= lo) return 0;
  return (hi == 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1);
}

// One pass of the disc over the plane P (rows of CL_WW words) at word (row, j): OR = true dilates, false erodes.  Rows row - r ..
// row + r must exist; a word left of the first or right of the last reads as `edge` (the bits it reaches are never used).
template <bool OR>
__device__ __forceinline__ u64 disc_pass(const u64 (*P)[CL_WW], int row, int j, const Disc& d) {
  const u64 edge = OR ? 0ull : ~0ull;
  u64 acc = edge, L = edge, C = edge, R = edge;
  int done = -1;   // rows |dy| <= done are combined in L, C, R
  for (int s = d.r; s >= 0; --s) {
    const int h = d.h[s];
    for (int dy = done + 1; dy <= h; ++dy) {
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        if (sg == 1 && dy == 0) continue;
        const u64* p = P[sg ? row - dy : row + dy];
        const u64 l = j > 0 ? p[j - 1] : edge, c = p[j], q = j + 1 < CL_WW ? p[j + 1] : edge;
        if (OR) L |= l, C |= c, R |= q;
        else L &= l, C &= c, R &= q;
      }
    }
    done = max(done, h);
    // pixel x of the shifted plane is pixel x - s (x + s) of the combined rows
    const u64 up = s ? (C << s) | (L >> (64 - s)) : C, dn = s ? (C >> s) | (R << (64 - s)) : C;
    if (OR) acc |= up | dn;
    else acc &= up & dn;
  }
  return acc;
}

// Closing (OPEN false) or opening (OPEN true) of every class plane of one tile; KIN: the source (pix_key), OUT: int64 (the
// result) or uint8 (the next stage's input).  counts: this image's three counters, slot 0 (gained by closing) or 2 (removed by
// opening) is added to; may be nullptr.
template <int KIN, bool OPEN, typename OUT>
__global__ __launch_bounds__(CL_THREADS) void morph_kernel(const void* __restrict__ src, int H, int W, int C, int ncls, Disc d,
                                                            OUT* __restrict__ out, u64* __restrict__ counts) {
  __shared__ unsigned char cls[CL_ROWS][CL_PX];         // classes of the haloed tile
  __shared__ unsigned char res[CL_TH][CL_TW * 64];      // the tile's result
  __shared__ u64 X[CL_ROWS][CL_WW], Y[CL_ROWS][CL_WW], Z[CL_TH][CL_TW];
  __shared__ unsigned present;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = d.r, rows = CL_TH + 4 * r;
  const int x0 = blockIdx.x * CL_TW * 64, y0 = blockIdx.y * CL_TH, xh0 = x0 - 64, yh0 = y0 - 2 * r;
  const int64_t base = (int64_t)blockIdx.z * H * W;
  if (tid == 0) present = 0;
  __syncthreads();
  {   // load: thread = column tid of the haloed tile; only the 2r pixels of a halo word next to the tile are read
    const int x = xh0 + tid;
    const bool colin = x >= 0 && x < W && x >= x0 - 2 * r && x < x0 + CL_TW * 64 + 2 * r;
    unsigned seen = 0;
    for (int row = 0; row < rows; ++row) {
      const int y = yh0 + row;
      int v = 0;
      if (colin && y >= 0 && y < H) v = foreground_class(pix_key<KIN>(src, base + (int64_t)y * W + x, C), ncls);
      cls[row][tid] = (unsigned char)v;
      seen |= 1u << v;
    }
    seen = wave_or(seen);
    if (lane == 0) atomicOr(&present, seen);
  }
  __syncthreads();
  for (int i = tid; i < CL_TH * CL_TW * 64; i += CL_THREADS) res[i / (CL_TW * 64)][i % (CL_TW * 64)] = cls[2 * r + i / (CL_TW * 64)][64 + i % (CL_TW * 64)];
  const unsigned pres = present;
  for (int c = 1; c < ncls; ++c) {
    if (!((pres >> c) & 1)) continue;   // uniform: no pixel of class c in the haloed tile, nothing closes or opens
    // plane c: a wave's ballot is one word.  For the opening, pixels outside the image do not erode: they read as c
    for (int it = wave; it < rows * CL_WW; it += CL_THREADS / 64) {
      const int row = it / CL_WW, j = it % CL_WW;
      u64 m = __ballot(cls[row][j * 64 + lane] == c);
      if (OPEN) m |= ~inside_word(yh0 + row, xh0 + j * 64, H, W);
      if (lane == 0) X[row][j] = m;
    }
    __syncthreads();
    // first pass on rows r .. rows - r: the dilation (as on an infinite plane: it may leave the image), or the erosion, which is a
    // set of image pixels
    for (int it = tid; it < (rows - 2 * r) * CL_WW; it += CL_THREADS) {
      const int row = r + it / CL_WW, j = it % CL_WW;
      u64 m = disc_pass<!OPEN>(X, row, j, d);
      if (OPEN) m &= inside_word(yh0 + row, xh0 + j * 64, H, W);
      Y[row][j] = m;
    }
    __syncthreads();
    if (tid < CL_TH * CL_TW) Z[tid / CL_TW][tid % CL_TW] = disc_pass<OPEN>(Y, 2 * r + tid / CL_TW, 1 + tid % CL_TW, d);
    __syncthreads();
    for (int i = tid; i < CL_TH * CL_TW * 64; i += CL_THREADS) {
      const int ty = i / (CL_TW * 64), col = i % (CL_TW * 64);
      const bool bit = (Z[ty][col / 64] >> (col % 64)) & 1;
      const int v = cls[2 * r + ty][64 + col];
      if (OPEN) {
        if (v == c && !bit) res[ty][col] = 0;
      } else {
        if (v == 0 && bit && res[ty][col] == 0) res[ty][col] = (unsigned char)c;   // c ascends: the smallest closing class
      }
    }
    // the next plane writes X, Y and Z behind the barriers above; res and cls are touched by their own thread only
  }
  __syncthreads();
  unsigned changed = 0;
  for (int i = tid; i < CL_TH * CL_TW * 64; i += CL_THREADS) {
    const int ty = i / (CL_TW * 64), col = i % (CL_TW * 64), y = y0 + ty, x = x0 + col;
    if (y >= H || x >= W) continue;
    const int v = res[ty][col];
    out[base + (int64_t)y * W + x] = (OUT)v;
    changed += v != cls[2 * r + ty][64 + col];
  }
  if (!counts) return;
  changed = wave_sum(changed);
  if (lane == 0 && changed) atomicAdd(&counts[3 * blockIdx.z + (OPEN ? 2 : 0)], (u64)changed);
}

// no stage is on: the class map itself, background written as 0
template <int KIN>
__global__ __launch_bounds__(CL_THREADS) void clean_copy_kernel(const void* __restrict__ src, int64_t n, int C, int ncls, long long* __restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (g < n) out[g] = foreground_class(pix_key<KIN>(src, g, C), ncls);
}

// fill (1): the background mask for the union-find, the uint8 class map (KIN 3: src is that map already) and cleared counters
template <int KIN>
__global__ __launch_bounds__(CL_THREADS) void fill_prepare_kernel(const void* __restrict__ src, int64_t n, int C, int ncls, unsigned char* __restrict__ cm,
                                                                   int* __restrict__ bgmask, unsigned* __restrict__ area, unsigned* __restrict__ info) {
  const int64_t g = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  if (g >= n) return;
  const int v = foreground_class(pix_key<KIN>(src, g, C), ncls);
  if (KIN != 3) cm[g] = (unsigned char)v;
  bgmask[g] = v == 0;
  area[g] = 0;
  info[g] = 0;
}

// fill (2): every background pixel adds itself to its root's area, and the border flag (bit 0) and the classes of its foreground
// 4-neighbours (bit c) to its root's word; the pixels of one root are combined inside the wave
__global__ __launch_bounds__(CL_THREADS) void fill_stats_kernel(const unsigned char* __restrict__ cm, const int* __restrict__ P, int H, int W, int64_t n,
                                                                 unsigned* __restrict__ area, unsigned* __restrict__ info) {
  const int64_t g = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  int root = -1;
  unsigned m = 0;
  if (g < n) root = P[g];
  if (root >= 0) {
    const int64_t HW = (int64_t)H * W, i = g % HW;
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    unsigned nb = 0;   // bit v for a 4-neighbour holding v
    if (x > 0) nb |= 1u << cm[g - 1];
    if (x < W - 1) nb |= 1u << cm[g + 1];
    if (y > 0) nb |= 1u << cm[g - W];
    if (y < H - 1) nb |= 1u << cm[g + W];
    m = (nb & ~1u) | (unsigned)(x == 0 || y == 0 || x == W - 1 || y == H - 1);
  }
  wave_by_key(
      root,
      [=](int lr, bool mine, bool lead) {
        const unsigned o = wave_or(mine ? m : 0u);
        const unsigned cnt = (unsigned)__popcll(__ballot(mine));
        if (lead) {
          atomicAdd(&area[lr], cnt);
          if (o) atomicOr(&info[lr], o);
        }
      },
      [=] {
        atomicAdd(&area[root], 1u);
        if (m) atomicOr(&info[root], m);
      });
}

// fill (3): a background pixel whose component is a hole takes the one class around it
template <typename OUT>
__global__ __launch_bounds__(CL_THREADS) void fill_apply_kernel(const unsigned char* __restrict__ cm, const int* __restrict__ P, int64_t HW, int64_t n,
                                                                 const unsigned* __restrict__ area, const unsigned* __restrict__ info, long long max_area,
                                                                 OUT* __restrict__ out, u64* __restrict__ counts) {
  const int64_t g = (int64_t)blockIdx.x * CL_THREADS + threadIdx.x;
  bool filled = false;
  if (g < n) {
    int v = cm[g];
    const int root = P[g];
    if (root >= 0) {
      const unsigned o = info[root];
      if (!(o & 1) && __popc(o >> 1) == 1 && (max_area <= 0 || (long long)area[root] <= max_area)) {
        v = __ffs((int)(o >> 1));   // bit c of o is class c
        filled = true;
      }
    }
    out[g] = (OUT)v;
  }
  if (!counts) return;
  // a wave lies in at most two images (HW >= 64) or in several tiny ones: one atomic per image and wave
  const long long b = g < n && filled ? (long long)(g / HW) : -1;
  wave_by_key(
      b,
      [=](long long lb, bool mine, bool lead) {
        const unsigned cnt = (unsigned)__popcll(__ballot(mine));
        if (lead) atomicAdd(&counts[3 * lb + 1], (u64)cnt);
      },
      [=] { atomicAdd(&counts[3 * b + 1], 1ull); });
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

static Disc make_disc(int r2) {
  Disc d;
  memset(&d, 0, sizeof d);
  while ((d.r + 1) * (d.r + 1) <= r2) ++d.r;
  for (int s = 0; s <= d.r; ++s) {
    int h = 0;
    while ((h + 1) * (h + 1) <= r2 - s * s) ++h;
    d.h[s] = (signed char)h;
  }
  return d;
}

template <int KIN, bool OPEN, typename OUT>
static void launch_morph(const void* src, int B, int H, int W, int C, int ncls, int r2, OUT* out, u64* counts, hipStream_t s) {
  const dim3 tiles((W + CL_TW * 64 - 1) / (CL_TW * 64), (H + CL_TH - 1) / CL_TH, B);
  hipLaunchKernelGGL((morph_kernel<KIN, OPEN, OUT>), tiles, dim3(CL_THREADS), 0, s, src, H, W, C, ncls, make_disc(r2), out, counts);
}
// the source kind is the caller's (0, 1) or the uint8 map of the stage before (3)
template <bool OPEN, typename OUT>
static void morph(const void* src, int kin, int B, int H, int W, int C, int ncls, int r2, OUT* out, u64* counts, hipStream_t s) {
  if (kin == 0) launch_morph<0, OPEN, OUT>(src, B, H, W, C, ncls, r2, out, counts, s);
  else if (kin == 1) launch_morph<1, OPEN, OUT>(src, B, H, W, C, ncls, r2, out, counts, s);
  else launch_morph<3, OPEN, OUT>(src, B, H, W, C, ncls, r2, out, counts, s);
}

extern "C" {

int mgu_clean_masks(mgu_ctx* c, const void* src_dev, int src_kind, int B, int H, int W, int C, int64_t num_classes, int close_radius_sq,
                    int fill_holes, int64_t max_hole_area, int open_radius_sq, int64_t* out_dev, int64_t* counts_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!src_dev || !out_dev || B < 0 || H < 0 || W < 0) return fail(c, MGU_ERR_INVALID, "bad clean_masks args (null pointer or negative size)");
  if (src_kind != 0 && src_kind != 1) return fail(c, MGU_ERR_INVALID, "clean_masks: src_kind %d (0 int64 class map, 1 fp32 logits)", src_kind);
  if (src_kind == 1) num_classes = C;
  if (num_classes < 2 || num_classes > 32)
    return fail(c, MGU_ERR_INVALID, "clean_masks: num_classes %lld (2..32; the channels C for logits)", (long long)num_classes);
  const int r2max = CL_MAX_R * CL_MAX_R;
  if (close_radius_sq < 0 || close_radius_sq > r2max || open_radius_sq < 0 || open_radius_sq > r2max)
    return fail(c, MGU_ERR_INVALID, "clean_masks: close_radius_sq %d, open_radius_sq %d (0..%d)", close_radius_sq, open_radius_sq, r2max);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "clean_masks: at most 65535 images per call");
  if (int rc = check_pixel_count(c, "clean_masks", B, H, W)) return rc;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const char *s0 = (const char*)src_dev, *s1 = s0 + (size_t)n * (src_kind == 1 ? (size_t)C * 4 : 8);
  const char *o0 = (const char*)out_dev, *o1 = o0 + (size_t)n * 8;
  if (n > 0 && s0 < o1 && o0 < s1) return fail(c, MGU_ERR_INVALID, "clean_masks: the output must not alias the input");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  u64* counts = (u64*)counts_dev;
  if (counts) HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)B * 3 * sizeof(u64), s));
  if (n == 0) return MGU_OK;
  const int ncls = (int)num_classes;
  const bool do_close = close_radius_sq > 0, do_fill = fill_holes != 0, do_open = open_radius_sq > 0;
  Carve cv;
  const size_t oM0 = cv.take((size_t)n), oM1 = cv.take((size_t)n);   // the uint8 class maps between the stages
  const size_t oB = do_fill ? cv.take((size_t)n * 4) : 0, oP = do_fill ? cv.take((size_t)n * 4) : 0;
  const size_t oA = do_fill ? cv.take((size_t)n * 4) : 0, oI = do_fill ? cv.take((size_t)n * 4) : 0;
  int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off);
  if (rc) return rc;
  char* ws = (char*)c->objws;
  unsigned char* m0 = (unsigned char*)(ws + oM0);
  unsigned char* m1 = (unsigned char*)(ws + oM1);
  long long* out = (long long*)out_dev;
  const unsigned pixblocks = grid_for(n, CL_THREADS, INT_MAX);

  const void* cur = src_dev;   // what the next stage reads, and how (pix_key's KIND)
  int kin = src_kind;
  if (!do_close && !do_fill && !do_open) {
    if (kin == 0) hipLaunchKernelGGL(clean_copy_kernel<0>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cur, n, C, ncls, out);
    else hipLaunchKernelGGL(clean_copy_kernel<1>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cur, n, C, ncls, out);
  }
  if (do_close) {
    if (do_fill || do_open) {
      morph<false>(cur, kin, B, H, W, C, ncls, close_radius_sq, m0, counts, s);
      cur = m0, kin = 3;
    } else {
      morph<false>(cur, kin, B, H, W, C, ncls, close_radius_sq, out, counts, s);
    }
  }
  if (do_fill) {
    int* bgmask = (int*)(ws + oB);
    int* P = (int*)(ws + oP);
    unsigned* area = (unsigned*)(ws + oA);
    unsigned* info = (unsigned*)(ws + oI);
    const unsigned char* cm = kin == 3 ? (const unsigned char*)cur : m0;
    if (kin == 0) hipLaunchKernelGGL(fill_prepare_kernel<0>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cur, n, C, ncls, m0, bgmask, area, info);
    else if (kin == 1) hipLaunchKernelGGL(fill_prepare_kernel<1>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cur, n, C, ncls, m0, bgmask, area, info);
    else hipLaunchKernelGGL(fill_prepare_kernel<3>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cur, n, C, ncls, m0, bgmask, area, info);
    rc = cc_roots_i32(c, bgmask, B, H, W, P, s, false);
    if (rc) return rc;
    hipLaunchKernelGGL(fill_stats_kernel, dim3(pixblocks), dim3(CL_THREADS), 0, s, cm, P, H, W, n, area, info);
    if (do_open) {
      hipLaunchKernelGGL(fill_apply_kernel<unsigned char>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cm, P, HW, n, area, info,
                         (long long)max_hole_area, m1, counts);
      cur = m1, kin = 3;
    } else {
      hipLaunchKernelGGL(fill_apply_kernel<long long>, dim3(pixblocks), dim3(CL_THREADS), 0, s, cm, P, HW, n, area, info,
                         (long long)max_hole_area, out, counts);
    }
  }
  if (do_open) morph<true>(cur, kin, B, H, W, C, ncls, open_radius_sq, out, counts, s);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
