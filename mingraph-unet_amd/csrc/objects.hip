// Object counting on the device: connected components of a batch of class maps, per-object statistics and the greedy box matching
// of experiments/metrics.py:215-240 -- the instance step shape_loss.py:43-91 leaves commented out (skimage.measure.label).
//   mgu_connected_components  int64 class map (B, H*W) or NHWC fp32 logits (argmax fused) -> int32 labels (B, H, W), 0 = background,
//                             objects 1..n_b per image in raster order of their first pixel; counts (B) and offsets (B + 1)
//   mgu_object_stats          per object: class, area, bbox [xmin, ymin, xmax, ymax) and the coordinate sums, all integer
//   mgu_match_objects         the reference's greedy IoU matching, one workgroup per image; int64 totals accumulated
//   mgu_object_scores         per object: the mean probability of its class over its pixels (fixed-point integer sums, fp32 result)
// Labelling is block union-find: (1) a 32 x 32 tile joins its pixels in LDS, (2) tile borders are joined in global memory,
// (3) every pixel points straight at its root, (4) roots are numbered by a per-image scan of root flags in raster order.  Every
// union hooks the larger root under the smaller one with atomicMin, so each root ends as its component's smallest linear index:
// whatever order the atomics land in, the trees' roots, and so the numbering, are the same -- the labels are deterministic.
// All accumulations are integer atomics (exact, order-free); runs of equal labels are summed inside a wave before the atomic.
// split.hip labels its int32 zone map through steps (1)-(3) (cc_roots_i32) and numbers its own objects through (3)-(4)
// (cc_number_roots, the tail of mgu_connected_components); clean.hip labels the background of a class map through (1)-(3) with
// 4-neighbours; both are declared in ctx.h.  The wave pre-aggregation (wave_by_key), the scans, the pixel -> object rule and the
// value of a pixel (pix_key) are objects_common.h's, shared with shapes.hip, instances.hip and clean.hip.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int OB_THREADS = 256;
constexpr int TILE = 32;                      // labelling tile: TILE x TILE pixels, 4 per thread
constexpr int TILE_PIX = TILE * TILE;
constexpr int CHUNK = 4 * OB_THREADS;         // root numbering: 1024 consecutive pixels of one image per workgroup

// foreground: not the background value and, with a class range (ncls > 0), inside [0, ncls)
__device__ __forceinline__ bool is_fg(long long v, long long bg, long long ncls) { return v != bg && (ncls <= 0 || (v >= 0 && v < ncls)); }

// root of x (parents only ever point at smaller indices; volatile: another workgroup may be lowering them)
__device__ __forceinline__ int find_root(const volatile int* par, int x) {
  int p = par[x];
  while (p != x) {
    x = p;
    p = par[x];
  }
  return x;
}

// join the trees of a and b: the larger root is hooked under the smaller one (atomicMin); a failed hook (the root moved on
// meanwhile) retries from the value it found, so the two trees always end up joined and every root is its tree's minimum
__device__ __forceinline__ void unite(int* par, int a, int b) {
  while (true) {
    a = find_root(par, a);
    b = find_root(par, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&par[a], b);
    if (old == a) return;
    a = old;
  }
}

// (1) one tile in LDS: union-find over the tile's pixels, then every pixel's global parent is its tile root (global linear index)
template <int KIND, bool CONN8>
__global__ __launch_bounds__(OB_THREADS) void cc_local_kernel(const void* __restrict__ src, int H, int W, int C, long long bg, long long ncls,
                                                              int* __restrict__ P) {
  __shared__ long long key[TILE_PIX];
  __shared__ int par[TILE_PIX];
  const int tid = threadIdx.x, tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
  const int64_t HW = (int64_t)H * W, base = (int64_t)blockIdx.z * HW;
  bool fg[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = tid + k * OB_THREADS, y = ty0 + li / TILE, x = tx0 + li % TILE;
    long long v = 0;
    fg[k] = false;
    if (y < H && x < W) {
      v = pix_key<KIND>(src, base + (int64_t)y * W + x, C);
      fg[k] = is_fg(v, bg, ncls);
    }
    key[li] = v;
    par[li] = fg[k] ? li : -1;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (!fg[k]) continue;
    const int li = tid + k * OB_THREADS, r = li / TILE, c = li % TILE;
    const long long v = key[li];
    // the neighbours earlier in raster order; a foreground pixel's parent stays >= 0, so par[n] >= 0 tells foreground
    if (c > 0 && par[li - 1] >= 0 && key[li - 1] == v) unite(par, li, li - 1);
    if (r > 0 && par[li - TILE] >= 0 && key[li - TILE] == v) unite(par, li, li - TILE);
    if (CONN8 && r > 0 && c > 0 && par[li - TILE - 1] >= 0 && key[li - TILE - 1] == v) unite(par, li, li - TILE - 1);
    if (CONN8 && r > 0 && c < TILE - 1 && par[li - TILE + 1] >= 0 && key[li - TILE + 1] == v) unite(par, li, li - TILE + 1);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = tid + k * OB_THREADS, y = ty0 + li / TILE, x = tx0 + li % TILE;
    if (y >= H || x >= W) continue;
    int g = -1;
    if (fg[k]) {   // tile order is raster order inside the tile, so the tile root is the smallest global index as well
      const int rt = find_root(par, li);
      g = (int)(base + (int64_t)(ty0 + rt / TILE) * W + tx0 + rt % TILE);
    }
    P[base + (int64_t)y * W + x] = g;
  }
}

// (2) the borders of one tile: its first row, first and last column join their earlier neighbours that lie in another tile
template <int KIND, bool CONN8>
__global__ __launch_bounds__(128) void cc_border_kernel(const void* __restrict__ src, int H, int W, int C, int* __restrict__ P) {
  const int t = threadIdx.x, tx0 = blockIdx.x * TILE, ty0 = blockIdx.y * TILE;
  int y, x;
  if (t < TILE) y = ty0, x = tx0 + t;                              // first row
  else if (t < 2 * TILE) y = ty0 + t - TILE, x = tx0;              // first column
  else if (t < 3 * TILE) y = ty0 + t - 2 * TILE, x = tx0 + TILE - 1;   // last column
  else return;
  if (y >= H || x >= W) return;
  const int64_t HW = (int64_t)H * W, base = (int64_t)blockIdx.z * HW;
  const int g = (int)(base + (int64_t)y * W + x);
  if (P[g] < 0) return;
  const long long v = pix_key<KIND>(src, g, C);
  const int ny[4] = {y, y - 1, y - 1, y - 1}, nx[4] = {x - 1, x, x - 1, x + 1};
#pragma unroll
  for (int k = 0; k < (CONN8 ? 4 : 2); ++k) {
    const int yy = ny[k], xx = nx[k];
    if (yy < 0 || xx < 0 || xx >= W) continue;
    if (yy / TILE == blockIdx.y && xx / TILE == blockIdx.x) continue;   // same tile: joined in (1)
    const int n = (int)(base + (int64_t)yy * W + xx);
    if (P[n] >= 0 && pix_key<KIND>(src, n, C) == v) unite(P, g, n);
  }
}

// (3) every pixel points at its root; with a min_area, roots count their pixels (runs of one root summed inside the wave)
__global__ __launch_bounds__(OB_THREADS) void cc_flatten_kernel(int* __restrict__ P, int64_t n, unsigned* __restrict__ area) {
  const int64_t g = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  int r = -1;
  if (g < n && P[g] >= 0) {
    r = find_root(P, (int)g);
    P[g] = r;
  }
  if (!area) return;
  wave_by_key(
      r,
      [=](int lr, bool mine, bool lead) {
        const unsigned long long m = __ballot(mine);
        if (lead) atomicAdd(&area[lr], (unsigned)__popcll(m));
      },
      [=] { atomicAdd(&area[r], 1u); });
}

__device__ __forceinline__ bool is_root(const int* P, const unsigned* area, int min_area, int64_t g) {
  return P[g] == (int)g && (!area || area[g] >= (unsigned)min_area);
}

// (4a) roots per chunk of CHUNK consecutive pixels of one image (grid: chunks x images)
__global__ __launch_bounds__(OB_THREADS) void cc_count_kernel(const int* __restrict__ P, const unsigned* __restrict__ area, int min_area,
                                                              int64_t HW, int* __restrict__ cnt) {
  __shared__ int sh[4];
  const int64_t base = (int64_t)blockIdx.y * HW, i0 = (int64_t)blockIdx.x * CHUNK + 4 * threadIdx.x;
  int c = 0;
  for (int k = 0; k < 4; ++k)
    if (i0 + k < HW) c += is_root(P, area, min_area, base + i0 + k);
  int total;
  block_exclusive_scan(c, sh, &total);
  if (threadIdx.x == 0) cnt[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// (4b) one workgroup: exclusive scan of all chunk counts (images in order) -> first object index of every chunk; per-image counts
// and offsets (the first object of image b is offsets[b]; offsets[B] = all objects of the batch)
__global__ __launch_bounds__(SCAN_THREADS) void cc_scan_kernel(const int* __restrict__ cnt, int64_t nch, int B, long long* __restrict__ choff,
                                                               long long* __restrict__ counts, long long* __restrict__ offsets) {
  const long long all = chunk_sum_scan(cnt, nch * B, choff);
  __syncthreads();
  for (int b = threadIdx.x; b <= B; b += SCAN_THREADS) {   // image b starts at its first chunk
    const long long first = b < B ? choff[b * nch] : all;
    offsets[b] = first;
    if (b < B) counts[b] = (b + 1 < B ? choff[(b + 1) * nch] : all) - first;
  }
}

// (4c) number the roots of a chunk in raster order: label = object index - offsets[b] + 1, written at the root pixel
__global__ __launch_bounds__(OB_THREADS) void cc_number_kernel(const int* __restrict__ P, const unsigned* __restrict__ area, int min_area,
                                                               int64_t HW, const long long* __restrict__ choff, const long long* __restrict__ offsets,
                                                               int* __restrict__ labels) {
  __shared__ int sh[4];
  const int b = blockIdx.y;
  const int64_t base = (int64_t)b * HW, i0 = (int64_t)blockIdx.x * CHUNK + 4 * threadIdx.x;
  bool f[4];
  int c = 0;
  for (int k = 0; k < 4; ++k) {
    f[k] = i0 + k < HW && is_root(P, area, min_area, base + i0 + k);
    c += f[k];
  }
  int total;
  const int ex = block_exclusive_scan(c, sh, &total);
  const long long first = choff[(int64_t)b * gridDim.x + blockIdx.x] - offsets[b] + 1 + ex;
  int j = 0;
  for (int k = 0; k < 4; ++k)
    if (f[k]) labels[base + i0 + k] = (int)(first + j++);
}

// (4d) every other pixel takes its root's label; background and pixels of dropped (too small) objects get 0
__global__ __launch_bounds__(OB_THREADS) void cc_relabel_kernel(const int* __restrict__ P, const unsigned* __restrict__ area, int min_area,
                                                                int64_t n, int* __restrict__ labels) {
  const int64_t g = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  if (g >= n) return;
  const int r = P[g];
  if (r < 0) {
    labels[g] = 0;
    return;
  }
  const bool keep = !area || area[r] >= (unsigned)min_area;
  if (r == (int)g) {
    if (!keep) labels[g] = 0;   // a kept root holds its label already
    return;
  }
  labels[g] = keep ? labels[r] : 0;
}

// ---- per-object statistics -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OB_THREADS) void stats_init_kernel(const long long* __restrict__ offsets, int B, int64_t cap, long long* __restrict__ area,
                                                                int* __restrict__ bbox, long long* __restrict__ sums) {
  const int64_t n = objects_recorded(offsets, B, cap);
  for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OB_THREADS) {
    if (area) area[i] = 0;
    bbox[4 * i] = INT_MAX, bbox[4 * i + 1] = INT_MAX, bbox[4 * i + 2] = 0, bbox[4 * i + 3] = 0;
    if (sums) sums[2 * i] = 0, sums[2 * i + 1] = 0;
  }
}

// one thread per pixel; the lanes of one object are summed inside the wave (wave_by_key), the rest add directly
template <int KIND>
__global__ __launch_bounds__(OB_THREADS) void stats_kernel(const int* __restrict__ labels, const void* __restrict__ src, int C, int W, int64_t HW,
                                                           int64_t n, const long long* __restrict__ offsets, int64_t cap,
                                                           long long* __restrict__ cls, long long* __restrict__ area, int* __restrict__ bbox,
                                                           long long* __restrict__ sums) {
  const int64_t g = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  long long obj = -1;
  int x = 0, y = 0;
  if (g < n) {
    const int lab = labels[g];
    const int64_t b = g / HW, i = g - b * HW;
    y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    obj = object_index(lab, offsets, b, cap);
  }
  // one object's record: its class (every pixel of an object holds it: a plain store), pixel count, bbox corners, coordinate sums
  auto add = [=](long long o, unsigned long long cnt, int x0, int y0, int x1, int y1, unsigned long long sx, unsigned long long sy) {
    cls[o] = pix_key<KIND>(src, g, C);
    if (area) atomicAdd((unsigned long long*)&area[o], cnt);
    atomicMin(&bbox[4 * o], x0), atomicMin(&bbox[4 * o + 1], y0);
    atomicMax(&bbox[4 * o + 2], x1), atomicMax(&bbox[4 * o + 3], y1);
    if (sums) atomicAdd((unsigned long long*)&sums[2 * o], sx), atomicAdd((unsigned long long*)&sums[2 * o + 1], sy);
  };
  wave_by_key(
      obj,
      [=](long long lo, bool mine, bool lead) {
        const int x0 = wave_min(mine ? x : INT_MAX), y0 = wave_min(mine ? y : INT_MAX);
        const int x1 = wave_max(mine ? x + 1 : 0), y1 = wave_max(mine ? y + 1 : 0);
        unsigned long long sx = 0, sy = 0;
        if (sums) sx = wave_sum<unsigned long long>(mine ? x : 0), sy = wave_sum<unsigned long long>(mine ? y : 0);
        const int cnt = __popcll(__ballot(mine));
        if (lead) add(lo, (unsigned long long)cnt, x0, y0, x1, y1, sx, sy);
      },
      [=] { add(obj, 1ull, x, y, x + 1, y + 1, (unsigned long long)x, (unsigned long long)y); });
}

// ---- per-object confidence: mean probability of the object's class over its pixels ----------------------------------------------
__global__ __launch_bounds__(OB_THREADS) void scores_init_kernel(const long long* __restrict__ offsets, int B, int64_t cap,
                                                                 unsigned long long* __restrict__ acc) {
  const int64_t n = objects_recorded(offsets, B, cap);
  for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OB_THREADS) acc[i] = 0;
}

// one thread per pixel: the probability of its object's class, clamped to [0, 1], as the fixed-point integer round_half_even(p * 2^32)
// (exact in fp64); summed inside the wave per object as stats_kernel does, then one integer atomic per object and wave
__global__ __launch_bounds__(OB_THREADS) void scores_kernel(const int* __restrict__ labels, const float* __restrict__ probs, int C, int64_t HW,
                                                            int64_t n, const long long* __restrict__ offsets, int64_t cap,
                                                            const long long* __restrict__ cls, unsigned long long* __restrict__ acc) {
  const int64_t g = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x;
  long long obj = -1;
  unsigned long long q = 0;
  if (g < n) {
    obj = object_index(labels[g], offsets, g / HW, cap);
    if (obj >= 0) {
      const long long k = cls[obj];
      const float p = (k >= 0 && k < C) ? fminf(fmaxf(probs[g * C + k], 0.f), 1.f) : 0.f;
      q = __double2ull_rn((double)p * 4294967296.0);
    }
  }
  wave_by_key(
      obj,
      [=](long long lo, bool mine, bool lead) {
        const unsigned long long s = wave_sum<unsigned long long>(mine ? q : 0ull);
        if (lead) atomicAdd(&acc[lo], s);
      },
      [=] { atomicAdd(&acc[obj], q); });
}

// score = (acc * 2^-32) / area in fp64, rounded to fp32
__global__ __launch_bounds__(OB_THREADS) void scores_finish_kernel(const long long* __restrict__ offsets, int B, int64_t cap,
                                                                   const unsigned long long* __restrict__ acc, const long long* __restrict__ area,
                                                                   float* __restrict__ scores) {
  const int64_t n = objects_recorded(offsets, B, cap);
  for (int64_t i = (int64_t)blockIdx.x * OB_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * OB_THREADS)
    scores[i] = area[i] > 0 ? (float)(((double)acc[i] * 0x1p-32) / (double)area[i]) : 0.f;
}

// ---- greedy matching (metrics.py:215-240), one wave per image ---------------------------------------------------------------------
// Predictions in object order (every confidence 1.0: the stable sort keeps list order); for each, the unused GT objects of its class
// are scored by IoU (fp64, inter / (a1 + a2 - inter), = Python's correctly rounded int / int); the first strictly larger IoU wins
// and a match needs best > 0 and best >= thresh.  GT object j belongs to lane j % 64, which alone reads and writes its used flag.
__global__ __launch_bounds__(64) void match_kernel(const long long* __restrict__ goff, const long long* __restrict__ gcls, const int4* __restrict__ gbox,
                                                   int64_t gcap, const long long* __restrict__ poff, const long long* __restrict__ pcls,
                                                   const int4* __restrict__ pbox, int64_t pcap, double thresh, unsigned char* __restrict__ used,
                                                   unsigned long long* __restrict__ totals) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long g0 = goff[b], G = goff[b + 1] - g0, p0 = poff[b], NP = poff[b + 1] - p0;
  if (g0 + G > gcap || p0 + NP > pcap) return;   // objects past the arrays' capacity were not recorded
  for (long long j = lane; j < G; j += 64) used[g0 + j] = 0;
  unsigned long long matched = 0;
  for (long long p = 0; p < NP; ++p) {
    const long long pc = pcls[p0 + p];
    const int4 pb = pbox[p0 + p];
    const long long a1 = (long long)(pb.z - pb.x) * (pb.w - pb.y);
    double best = 0.0;
    long long bj = -1;
    for (long long j = lane; j < G; j += 64) {
      if (used[g0 + j] || gcls[g0 + j] != pc) continue;
      const int4 gb = gbox[g0 + j];
      const long long iw = max(0, min(pb.z, gb.z) - max(pb.x, gb.x)), ih = max(0, min(pb.w, gb.w) - max(pb.y, gb.y));
      const long long inter = iw * ih;
      if (inter == 0) continue;   // IoU 0.0 is never strictly larger than best
      const long long a2 = (long long)(gb.z - gb.x) * (gb.w - gb.y);
      const double iou = (double)inter / (double)(a1 + a2 - inter);
      if (iou > best) best = iou, bj = j;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {   // larger IoU; equal IoU: the smaller index (the first in list order)
      const double ob = __shfl_xor(best, off);
      const long long oj = __shfl_xor(bj, off);
      if (ob > best || (ob == best && oj >= 0 && (bj < 0 || oj < bj))) best = ob, bj = oj;
    }
    if (bj >= 0 && best >= thresh) {
      if (lane == (int)(bj % 64)) used[g0 + bj] = 1;
      ++matched;
    }
  }
  if (lane == 0) {
    atomicAdd(&totals[0], (unsigned long long)G);
    atomicAdd(&totals[1], (unsigned long long)NP);
    atomicAdd(&totals[2], matched);
  }
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace mgud {

int64_t cc_chunks(int64_t HW) { return (HW + CHUNK - 1) / CHUNK; }

int cc_roots_i32(mgu_ctx* c, const int32_t* map, int B, int H, int W, int* P, hipStream_t s, bool conn8) {
  const dim3 tiles((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, B);
  const int64_t n = (int64_t)B * H * W;
  if (conn8) {
    hipLaunchKernelGGL((cc_local_kernel<2, true>), tiles, dim3(OB_THREADS), 0, s, map, H, W, 0, 0ll, 0ll, P);
    hipLaunchKernelGGL((cc_border_kernel<2, true>), tiles, dim3(128), 0, s, map, H, W, 0, P);
  } else {
    hipLaunchKernelGGL((cc_local_kernel<2, false>), tiles, dim3(OB_THREADS), 0, s, map, H, W, 0, 0ll, 0ll, P);
    hipLaunchKernelGGL((cc_border_kernel<2, false>), tiles, dim3(128), 0, s, map, H, W, 0, P);
  }
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(grid_for(n, OB_THREADS, INT_MAX)), dim3(OB_THREADS), 0, s, P, n, (unsigned*)nullptr);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int cc_number_roots(mgu_ctx* c, int* P, unsigned* area, int min_area, int B, int64_t HW, int* cnt, long long* choff, int32_t* labels,
                    int64_t* counts, int64_t* offsets, hipStream_t s) {
  const int64_t n = (int64_t)B * HW, nch = cc_chunks(HW);
  if (area) HIPCHK(c, hipMemsetAsync(area, 0, (size_t)n * 4, s));
  const unsigned pixblocks = grid_for(n, OB_THREADS, INT_MAX);
  hipLaunchKernelGGL(cc_flatten_kernel, dim3(pixblocks), dim3(OB_THREADS), 0, s, P, n, area);
  const dim3 chunks((unsigned)nch, B);
  hipLaunchKernelGGL(cc_count_kernel, chunks, dim3(OB_THREADS), 0, s, P, area, min_area, HW, cnt);
  hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, cnt, nch, B, choff, (long long*)counts, (long long*)offsets);
  hipLaunchKernelGGL(cc_number_kernel, chunks, dim3(OB_THREADS), 0, s, P, area, min_area, HW, choff, (const long long*)offsets, (int*)labels);
  hipLaunchKernelGGL(cc_relabel_kernel, dim3(pixblocks), dim3(OB_THREADS), 0, s, P, area, min_area, n, (int*)labels);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // namespace mgud

extern "C" {

int mgu_connected_components(mgu_ctx* c, const void* src_dev, int src_kind, int B, int H, int W, int C, int connectivity, int64_t background,
                             int64_t num_classes, int min_area, int32_t* labels_dev, int64_t* counts_dev, int64_t* offsets_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!src_dev || !labels_dev || !counts_dev || !offsets_dev || B < 0 || H < 0 || W < 0 || min_area < 0)
    return fail(c, MGU_ERR_INVALID, "bad connected_components args (null pointer or negative size)");
  if (src_kind != 0 && src_kind != 1) return fail(c, MGU_ERR_INVALID, "connected_components: src_kind %d (0 int64 class map, 1 fp32 logits)", src_kind);
  if (src_kind == 1 && C < 1) return fail(c, MGU_ERR_INVALID, "connected_components: logits need C >= 1");
  if (connectivity != 1 && connectivity != 2) return fail(c, MGU_ERR_INVALID, "connected_components: connectivity %d (1 or 2)", connectivity);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "connected_components: at most 65535 images per call");
  if (int rc = check_pixel_count(c, "connected_components", B, H, W)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  if (n == 0) return clear_counts(c, B, counts_dev, offsets_dev, s);
  const int64_t nch = cc_chunks(HW);
  Carve cv;
  const size_t oP = cv.take((size_t)n * 4), oA = min_area > 0 ? cv.take((size_t)n * 4) : 0, oC = cv.take((size_t)nch * B * 4);
  int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off + (size_t)nch * B * 8);   // the last region ends the buffer: no padding behind it
  if (rc) return rc;
  char* ws = (char*)c->objws;
  int* P = (int*)(ws + oP);
  unsigned* area = min_area > 0 ? (unsigned*)(ws + oA) : nullptr;
  const long long bg = background, ncls = num_classes;
  const dim3 tiles((W + TILE - 1) / TILE, (H + TILE - 1) / TILE, B);
#define MGU_CC(KIND, C8)                                                                                                \
  do {                                                                                                                  \
    hipLaunchKernelGGL((cc_local_kernel<KIND, C8>), tiles, dim3(OB_THREADS), 0, s, src_dev, H, W, C, bg, ncls, P);     \
    hipLaunchKernelGGL((cc_border_kernel<KIND, C8>), tiles, dim3(128), 0, s, src_dev, H, W, C, P);                      \
  } while (0)
  if (src_kind == 0) {
    if (connectivity == 2) MGU_CC(0, true);
    else MGU_CC(0, false);
  } else {
    if (connectivity == 2) MGU_CC(1, true);
    else MGU_CC(1, false);
  }
#undef MGU_CC
  return cc_number_roots(c, P, area, min_area, B, HW, (int*)(ws + oC), (long long*)(ws + cv.off), labels_dev, counts_dev, offsets_dev, s);
}

int mgu_object_stats(mgu_ctx* c, const int32_t* labels_dev, const void* src_dev, int src_kind, int B, int H, int W, int C,
                     const int64_t* offsets_dev, int64_t capacity, int64_t* class_dev, int64_t* area_dev, int32_t* bbox_dev, int64_t* sums_dev,
                     void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !src_dev || !offsets_dev || !class_dev || !bbox_dev || B < 0 || H < 0 || W < 0 || capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad object_stats args (null pointer or negative size)");
  if (src_kind != 0 && src_kind != 1) return fail(c, MGU_ERR_INVALID, "object_stats: src_kind %d (0 int64 class map, 1 fp32 logits)", src_kind);
  if (src_kind == 1 && C < 1) return fail(c, MGU_ERR_INVALID, "object_stats: logits need C >= 1");
  if (int rc = check_pixel_count(c, "object_stats", B, H, W)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  if (n == 0 || capacity == 0) return MGU_OK;
  const long long* off = (const long long*)offsets_dev;
  long long* ar = (long long*)area_dev;
  long long* su = (long long*)sums_dev;
  const unsigned initblocks = grid_for(capacity, OB_THREADS, 1024);
  hipLaunchKernelGGL(stats_init_kernel, dim3(initblocks), dim3(OB_THREADS), 0, s, off, B, capacity, ar, bbox_dev, su);
  const unsigned pixblocks = grid_for(n, OB_THREADS, INT_MAX);
  if (src_kind == 0)
    hipLaunchKernelGGL(stats_kernel<0>, dim3(pixblocks), dim3(OB_THREADS), 0, s, labels_dev, src_dev, C, W, HW, n, off, capacity,
                       (long long*)class_dev, ar, bbox_dev, su);
  else
    hipLaunchKernelGGL(stats_kernel<1>, dim3(pixblocks), dim3(OB_THREADS), 0, s, labels_dev, src_dev, C, W, HW, n, off, capacity,
                       (long long*)class_dev, ar, bbox_dev, su);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_object_scores(mgu_ctx* c, const int32_t* labels_dev, const float* probs_dev, int B, int H, int W, int C, const int64_t* offsets_dev,
                      int64_t capacity, const int64_t* class_dev, const int64_t* area_dev, float* scores_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !probs_dev || !offsets_dev || !class_dev || !area_dev || !scores_dev || B < 0 || H < 0 || W < 0 || C < 1 || capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad object_scores args (null pointer, negative size or C < 1)");
  if (int rc = check_pixel_count(c, "object_scores", B, H, W)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  if (capacity == 0) return MGU_OK;
  int rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)capacity * 8);
  if (rc) return rc;
  unsigned long long* acc = (unsigned long long*)c->objws;
  const long long* off = (const long long*)offsets_dev;
  const unsigned objblocks = grid_for(capacity, OB_THREADS, 1024);
  hipLaunchKernelGGL(scores_init_kernel, dim3(objblocks), dim3(OB_THREADS), 0, s, off, B, capacity, acc);
  if (n > 0) {
    const unsigned pixblocks = grid_for(n, OB_THREADS, INT_MAX);
    hipLaunchKernelGGL(scores_kernel, dim3(pixblocks), dim3(OB_THREADS), 0, s, labels_dev, probs_dev, C, HW, n, off, capacity,
                       (const long long*)class_dev, acc);
  }
  hipLaunchKernelGGL(scores_finish_kernel, dim3(objblocks), dim3(OB_THREADS), 0, s, off, B, capacity, acc, (const long long*)area_dev,
                     scores_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_match_objects(mgu_ctx* c, int B, const int64_t* gt_offsets_dev, const int64_t* gt_class_dev, const int32_t* gt_bbox_dev, int64_t gt_capacity,
                      const int64_t* pred_offsets_dev, const int64_t* pred_class_dev, const int32_t* pred_bbox_dev, int64_t pred_capacity,
                      double iou_thresh, int64_t* totals_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!gt_offsets_dev || !pred_offsets_dev || !totals_dev || B < 0 || gt_capacity < 0 || pred_capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad match_objects args (null pointer or negative size)");
  if ((gt_capacity > 0 && (!gt_class_dev || !gt_bbox_dev)) || (pred_capacity > 0 && (!pred_class_dev || !pred_bbox_dev)))
    return fail(c, MGU_ERR_INVALID, "match_objects: class and bbox arrays are needed for a nonzero capacity");
  if (B > INT_MAX / 2) return fail(c, MGU_ERR_INVALID, "match_objects: too many images");
  HIPCHK(c, hipSetDevice(c->device));
  if (B == 0) return MGU_OK;
  int rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)std::max<int64_t>(gt_capacity, 1));
  if (rc) return rc;
  hipLaunchKernelGGL(match_kernel, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, (const long long*)gt_offsets_dev, (const long long*)gt_class_dev,
                     (const int4*)gt_bbox_dev, gt_capacity, (const long long*)pred_offsets_dev, (const long long*)pred_class_dev,
                     (const int4*)pred_bbox_dev, pred_capacity, iou_thresh, (unsigned char*)c->objws, (unsigned long long*)totals_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
