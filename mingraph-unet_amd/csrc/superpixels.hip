// Superpixel graphs on the device: an over-segmentation of a batch of uint8 photographs, its region adjacency graph as a CSR, a node
// feature table and the means of feature maps over the regions (include/mgunet.h has the definitions).
//   mgu_slic_labels          integer SLIC (gSLIC formulation): fixed-point CIELAB, T assignment passes, T - 1 centre updates
//   mgu_regions_connect      raw labels -> 4-connected components, small regions merged into their best large neighbour, renumbered
//   mgu_regions_adjacency    label map -> CSR (int32 rowptr / col, the GAT's index types) with border lengths
//   mgu_regions_features_u8  per region: mean L, a, b, centroid, area -> (node_capacity, 8) fp32
//   mgu_regions_pool_nhwc    per region: mean of D channels of an NHWC fp32 map (fixed-point integer sums, fp32 result)
// Everything is integer arithmetic with integer atomics (exact, order-free), so every output is bitwise equal to
// tests/superpixels_oracle.py and from run to run.  The labelling passes are objects.hip's (cc_roots_i32, cc_number_roots), the pair
// hash table and its scan / pour / rank kernels are objects_common.h's, shared with instances.hip.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_TILE = 32;   // assignment tile: 32 x 32 pixels, 4 per thread; a wave walks 8 x 8 blocks (few labels per wave)
// centres a tile can meet along one axis: its pixels' home cells (at most ceil(31 / S) + 1) and one cell either side: 11 for S >= 4
constexpr int SP_MAXC = 11;

struct LabTables {
  unsigned short lin[256];
  int m[12];   // 3 x 3, rows sum to 4096; padded
  unsigned short f[4096];
};

// quarter-unit CIELAB of one sRGB pixel: 12-bit linear light, 12-bit XYZ (rows of m sum to 4096, so xyz <= 4095), f in 1/1024
__device__ __forceinline__ void rgb_to_lab(const LabTables* __restrict__ t, unsigned r, unsigned g, unsigned b, int& L, int& A, int& Bq) {
  const int lr = t->lin[r], lg = t->lin[g], lb = t->lin[b];
  const int x = (t->m[0] * lr + t->m[1] * lg + t->m[2] * lb + 2048) >> 12;
  const int y = (t->m[3] * lr + t->m[4] * lg + t->m[5] * lb + 2048) >> 12;
  const int z = (t->m[6] * lr + t->m[7] * lg + t->m[8] * lb + 2048) >> 12;
  const int fx = t->f[x], fy = t->f[y], fz = t->f[z];
  L = (116 * fy - 16384 + 128) >> 8;    // >> on a negative int is an arithmetic shift: floor
  A = (500 * (fx - fy) + 128) >> 8;
  Bq = (200 * (fy - fz) + 128) >> 8;
}

// floor(a / b), b > 0
__device__ __forceinline__ int floordiv(int a, int b) {
  const int q = a / b;
  return (a % b < 0) ? q - 1 : q;
}

// ---- stage 1: SLIC ----------------------------------------------------------------------------------------------------------------
// the packed 8-byte pixel: .x = L | a << 16 (both 16-bit, a signed), .y = b
__global__ __launch_bounds__(SP_THREADS) void slic_lab_kernel(const unsigned char* __restrict__ rgb, int64_t n, const LabTables* __restrict__ t,
                                                              int2* __restrict__ lab) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n) return;
  int L, A, Bq;
  rgb_to_lab(t, rgb[3 * g], rgb[3 * g + 1], rgb[3 * g + 2], L, A, Bq);
  lab[g] = make_int2((int)((unsigned)(L & 0xffff) | ((unsigned)A << 16)), Bq);
}

// centre k = i * gx + j of image b: [x, y, L, a, b, n]; its accumulators [n, sum rx, sum ry, sum L, sum a, sum b] are cleared
__global__ __launch_bounds__(SP_THREADS) void slic_init_kernel(const int2* __restrict__ lab, int64_t total, int H, int W, int S, int gx, int gy,
                                                               int* __restrict__ cen, int* __restrict__ acc) {
  const int64_t idx = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (idx >= total) return;
  const int K = gx * gy, b = (int)(idx / K), k = (int)(idx - (int64_t)b * K), i = k / gx, j = k - i * gx;
  const int x = min(j * S + S / 2, W - 1), y = min(i * S + S / 2, H - 1);
  const int2 p = lab[(int64_t)b * H * W + (int64_t)y * W + x];
  int* c = cen + idx * 6;
  c[0] = x, c[1] = y, c[2] = (short)(p.x & 0xffff), c[3] = p.x >> 16, c[4] = p.y, c[5] = 0;
  for (int q = 0; q < 6; ++q) acc[idx * 6 + q] = 0;
}

// One assignment pass over a 32 x 32 tile: the tile's centres are staged in LDS, every pixel takes the best of the up to nine centres
// around its home cell (D = dc^2 S^2 + mq^2 ds^2 in int64, an equal D to the smaller k: the candidates are visited in ascending k and
// only a strictly smaller D replaces the best).  LAST writes the label map; every other pass accumulates the sums of the next centre
// update instead: the lanes of a wave that chose one centre are summed together (wave_by_key), added to the tile's accumulators in
// LDS, and every centre the tile touched sends six integer atomics to global memory.
// Accumulator widths.  A centre owns pixels of the 3 x 3 cells around its home cell only: n <= 9 S^2 <= 147456 (S <= 128).  x and y
// are summed relative to the corner of that window (rx, ry in [0, 3 S) = [0, 384)), L in [0, 400], |a|, |b| <= 431 for the tables of
// mgunet.lab_tables (|a|, |b| <= 2000 and L <= 464 for any table the entry point accepts): every sum stays below 147456 * 2000 < 2^29,
// and 2 sum + n below 2^30: int32 holds them all.
template <bool LAST>
__global__ __launch_bounds__(SP_THREADS) void slic_assign_kernel(const int2* __restrict__ lab, const int* __restrict__ cen, int* __restrict__ acc,
                                                                 int* __restrict__ labels, int H, int W, int S, int gx, int gy, long long mq2) {
  __shared__ int sc[SP_MAXC * SP_MAXC * 5];
  __shared__ int sa[SP_MAXC * SP_MAXC * 6];
  const int tid = threadIdx.x, tx0 = blockIdx.x * SP_TILE, ty0 = blockIdx.y * SP_TILE, b = blockIdx.z;
  const int K = gx * gy;
  const int cj0 = max(tx0 / S - 1, 0), cj1 = min(min(tx0 + SP_TILE - 1, W - 1) / S + 1, gx - 1);
  const int ci0 = max(ty0 / S - 1, 0), ci1 = min(min(ty0 + SP_TILE - 1, H - 1) / S + 1, gy - 1);
  const int ncj = cj1 - cj0 + 1, nc = ncj * (ci1 - ci0 + 1);
  for (int c = tid; c < nc; c += SP_THREADS) {
    const int ii = ci0 + c / ncj, jj = cj0 + c % ncj;
    const int* src = cen + ((int64_t)b * K + ii * gx + jj) * 6;
    for (int q = 0; q < 5; ++q) sc[c * 5 + q] = src[q];
    if (!LAST)
      for (int q = 0; q < 6; ++q) sa[c * 6 + q] = 0;
  }
  __syncthreads();
  const int64_t base = (int64_t)b * H * W;
  const long long S2 = (long long)S * S;
  const int wave = tid >> 6, lane = tid & 63;
  for (int k = 0; k < 4; ++k) {
    const int x = tx0 + 8 * k + (lane & 7), y = ty0 + 8 * wave + (lane >> 3);
    const bool in = x < W && y < H;
    int bestc = -1, bestk = 0, rx = 0, ry = 0, pL = 0, pA = 0, pB = 0;
    if (in) {
      const int2 p = lab[base + (int64_t)y * W + x];
      pL = (short)(p.x & 0xffff), pA = p.x >> 16, pB = p.y;
      const int i = y / S, j = x / S;
      long long bestD = LLONG_MAX;
      int bi = 0, bj = 0;
      for (int di = -1; di <= 1; ++di) {
        const int ii = i + di;
        if (ii < 0 || ii >= gy) continue;
        for (int dj = -1; dj <= 1; ++dj) {
          const int jj = j + dj;
          if (jj < 0 || jj >= gx) continue;
          const int c = (ii - ci0) * ncj + (jj - cj0);
          const int* s = sc + c * 5;
          const int dx = x - s[0], dy = y - s[1], dL = pL - s[2], dA = pA - s[3], dB = pB - s[4];
          const long long D = (long long)(dL * dL + dA * dA + dB * dB) * S2 + mq2 * (long long)(dx * dx + dy * dy);
          if (D < bestD) bestD = D, bestc = c, bi = ii, bj = jj;
        }
      }
      bestk = bi * gx + bj;
      rx = x - (bj - 1) * S, ry = y - (bi - 1) * S;
    }
    if (LAST) {
      if (in) labels[base + (int64_t)y * W + x] = bestk;
    } else {
      wave_by_key(
          bestc,
          [=](int kc, bool mine, bool lead) {
            const int n = __popcll(__ballot(mine));
            const int s1 = wave_sum<int>(mine ? rx : 0), s2 = wave_sum<int>(mine ? ry : 0), s3 = wave_sum<int>(mine ? pL : 0);
            const int s4 = wave_sum<int>(mine ? pA : 0), s5 = wave_sum<int>(mine ? pB : 0);
            if (lead) {
              int* a = sa + kc * 6;
              atomicAdd(a, n), atomicAdd(a + 1, s1), atomicAdd(a + 2, s2), atomicAdd(a + 3, s3), atomicAdd(a + 4, s4), atomicAdd(a + 5, s5);
            }
          },
          [=] {
            int* a = sa + bestc * 6;
            atomicAdd(a, 1), atomicAdd(a + 1, rx), atomicAdd(a + 2, ry), atomicAdd(a + 3, pL), atomicAdd(a + 4, pA), atomicAdd(a + 5, pB);
          });
    }
  }
  if (LAST) return;
  __syncthreads();
  for (int c = tid; c < nc; c += SP_THREADS) {
    if (sa[c * 6] == 0) continue;
    const int ii = ci0 + c / ncj, jj = cj0 + c % ncj;
    int* dst = acc + ((int64_t)b * K + ii * gx + jj) * 6;
    for (int q = 0; q < 6; ++q) atomicAdd(dst + q, sa[c * 6 + q]);
  }
}

// centre update: every value becomes floor((2 sum + n) / (2 n)) over the pixels just assigned (x, y: the window corner added back,
// which commutes with the floor); n = 0 keeps the centre; [5] = n; the accumulators are cleared for the next pass
__global__ __launch_bounds__(SP_THREADS) void slic_update_kernel(int64_t total, int S, int gx, int gy, int* __restrict__ cen, int* __restrict__ acc) {
  const int64_t idx = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (idx >= total) return;
  int* a = acc + idx * 6;
  int* c = cen + idx * 6;
  const int n = a[0];
  if (n > 0) {
    const int k = (int)(idx % ((int64_t)gx * gy)), i = k / gx, j = k - i * gx;
    c[0] = (j - 1) * S + floordiv(2 * a[1] + n, 2 * n);
    c[1] = (i - 1) * S + floordiv(2 * a[2] + n, 2 * n);
    for (int q = 2; q < 5; ++q) c[q] = floordiv(2 * a[q + 1] + n, 2 * n);
  }
  c[5] = n;
  for (int q = 0; q < 6; ++q) a[q] = 0;
}

// ---- stage 2: connected, merged regions -------------------------------------------------------------------------------------------
// cc_roots_i32 reads 0 as background: raw labels >= 0 move up by one (negative values stay: they are components of their own too)
__global__ __launch_bounds__(SP_THREADS) void shift_labels_kernel(const int* raw, int64_t n, int delta, int* out) {   // raw == out in the last launch
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n) return;
  const int v = raw[g];
  out[g] = delta > 0 ? (v >= 0 ? (int)((unsigned)v + 1u) : v) : v - 1;
}

// every pixel edge between a small region s (area < min_area) and a large one d adds 1 to the pair (s, d); P holds every pixel's root
// (the region's first pixel), area is indexed by root.  A pixel looks right and down, so each pixel edge is met once.
__global__ __launch_bounds__(SP_THREADS) void merge_count_kernel(const int* __restrict__ P, const unsigned* __restrict__ area, unsigned min_area,
                                                                 int64_t n, int H, int W, PairTable t) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n) return;
  const int x = (int)(g % W), y = (int)((g / W) % H);
  const int r = P[g];
  const bool rs = area[r] < min_area;
  for (int d = 0; d < 2; ++d) {
    if (d == 0 ? x + 1 >= W : y + 1 >= H) continue;
    const int q = P[g + (d == 0 ? 1 : W)];
    if (q == r) continue;
    const bool qs = area[q] < min_area;
    if (rs && !qs) pair_add(t, ((unsigned long long)(unsigned)r << 32) | (unsigned)q, 1u);
    if (qs && !rs) pair_add(t, ((unsigned long long)(unsigned)q << 32) | (unsigned)r, 1u);
  }
}

// best[s] = max over the pairs (s, d) of (shared edges << 32 | ~d): the most shared edges, then the smaller d (its first pixel comes
// first in raster order)
__global__ __launch_bounds__(SP_THREADS) void merge_best_kernel(PairTable t, unsigned long long* __restrict__ best) {
  for (int64_t s = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; s < t.slots; s += (int64_t)gridDim.x * SP_THREADS) {
    const unsigned long long k = t.keys[s];
    if (k == PAIR_EMPTY) continue;
    atomicMax(&best[k >> 32], ((unsigned long long)t.cnt[s] << 32) | (0xFFFFFFFFull - (k & 0xFFFFFFFFull)));
  }
}

// the merged region's root is its first pixel: the smallest of d and the roots merging into it ...
__global__ __launch_bounds__(SP_THREADS) void merge_min_kernel(const unsigned long long* __restrict__ best, int64_t n, int* __restrict__ P) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n || best[g] == 0) return;
  atomicMin(&P[0xFFFFFFFFu - (unsigned)best[g]], (int)g);
}
// ... and every other merging root points at d, which points at that first pixel (d is large: no launch of this round writes P[d] now)
__global__ __launch_bounds__(SP_THREADS) void merge_link_kernel(const unsigned long long* __restrict__ best, int64_t n, int* __restrict__ P) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n || best[g] == 0) return;
  const int d = (int)(0xFFFFFFFFu - (unsigned)best[g]);
  if (P[d] != (int)g) P[g] = d;
}

// ---- stage 3: adjacency -----------------------------------------------------------------------------------------------------------
// node of pixel g: offsets[b] + label, or -1 (label outside [0, n_b), or an image whose nodes pass the capacity)
__device__ __forceinline__ long long node_index(int lab, const long long* __restrict__ offsets, int64_t b, int64_t cap) {
  const long long o0 = offsets[b], o1 = offsets[b + 1];
  if (lab < 0 || o0 < 0 || o1 > cap || (long long)lab >= o1 - o0) return -1;
  return o0 + lab;
}

__global__ __launch_bounds__(SP_THREADS) void adj_count_kernel(const int* __restrict__ labels, int64_t n, int H, int W, const long long* __restrict__ offsets,
                                                               int64_t cap, PairTable t) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (g >= n) return;
  const int64_t HW = (int64_t)H * W, b = g / HW;
  const int x = (int)(g % W), y = (int)((g / W) % H);
  const int la = labels[g];
  const long long u = node_index(la, offsets, b, cap);
  if (u < 0) return;
  for (int d = 0; d < 2; ++d) {
    if (d == 0 ? x + 1 >= W : y + 1 >= H) continue;
    const int lb = labels[g + (d == 0 ? 1 : W)];
    if (lb == la) continue;
    const long long v = node_index(lb, offsets, b, cap);
    if (v < 0) continue;
    pair_add(t, ((unsigned long long)u << 32) | (unsigned long long)v, 1u);
    pair_add(t, ((unsigned long long)v << 32) | (unsigned long long)u, 1u);
  }
}

// one workgroup: exclusive scan of the chunk sums; the number of directed edges; the status bits
__global__ __launch_bounds__(SCAN_THREADS) void adj_scan_kernel(const int* __restrict__ csum, int64_t nch, long long* __restrict__ choff,
                                                                long long* __restrict__ total_out, int64_t edge_cap, int B,
                                                                const long long* __restrict__ offsets, int64_t cap, int* __restrict__ status) {
  const int tid = threadIdx.x;
  const long long edges = chunk_sum_scan(csum, nch, choff);
  int bits = 0;
  for (int b = tid; b < B; b += SCAN_THREADS)
    if (offsets[b + 1] > cap) bits |= 2;
  if (tid == SCAN_THREADS - 1) {
    *total_out = edges;
    if (edges > edge_cap) bits |= 1;
  }
  if (bits) atomicOr(status, bits);
}

// ---- stages 4 and 5: per-region sums ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SP_THREADS) void zero_i64_kernel(long long* __restrict__ p, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SP_THREADS) p[i] = 0;
}

// stats[node] = [area, sum x, sum y, sum L, sum a, sum b]; the lanes of one node are summed inside the wave
__global__ __launch_bounds__(SP_THREADS) void feat_sum_kernel(const unsigned char* __restrict__ rgb, const int* __restrict__ labels, int64_t n, int H, int W,
                                                              const long long* __restrict__ offsets, int64_t cap, const LabTables* __restrict__ t,
                                                              long long* __restrict__ stats) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  long long node = -1;
  int x = 0, y = 0, L = 0, A = 0, Bq = 0;
  if (g < n) {
    const int64_t HW = (int64_t)H * W;
    node = node_index(labels[g], offsets, g / HW, cap);
    if (node >= 0) {
      x = (int)(g % W), y = (int)((g / W) % H);
      rgb_to_lab(t, rgb[3 * g], rgb[3 * g + 1], rgb[3 * g + 2], L, A, Bq);
    }
  }
  wave_by_key(
      node,
      [=](long long k, bool mine, bool lead) {
        const long long cnt = __popcll(__ballot(mine));
        const long long sx = wave_sum<long long>(mine ? x : 0), sy = wave_sum<long long>(mine ? y : 0);
        const long long sL = wave_sum<long long>(mine ? L : 0), sA = wave_sum<long long>(mine ? A : 0), sB = wave_sum<long long>(mine ? Bq : 0);
        if (lead) {
          unsigned long long* a = (unsigned long long*)(stats + k * 6);
          atomicAdd(a, (unsigned long long)cnt), atomicAdd(a + 1, (unsigned long long)sx), atomicAdd(a + 2, (unsigned long long)sy);
          atomicAdd(a + 3, (unsigned long long)sL), atomicAdd(a + 4, (unsigned long long)sA), atomicAdd(a + 5, (unsigned long long)sB);
        }
      },
      [=] {
        unsigned long long* a = (unsigned long long*)(stats + node * 6);
        atomicAdd(a, 1ull), atomicAdd(a + 1, (unsigned long long)(long long)x), atomicAdd(a + 2, (unsigned long long)(long long)y);
        atomicAdd(a + 3, (unsigned long long)(long long)L), atomicAdd(a + 4, (unsigned long long)(long long)A);
        atomicAdd(a + 5, (unsigned long long)(long long)Bq);
      });
}

// one double expression per column, cast once; a row of no node (or of no pixel) is zero
__global__ __launch_bounds__(SP_THREADS) void feat_finish_kernel(const long long* __restrict__ stats, int64_t cap, int H, int W, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= cap) return;
  const long long* s = stats + i * 6;
  const long long area = s[0];
  float* o = out + i * 8;
  for (int q = 0; q < 8; ++q) o[q] = 0.f;
  if (area <= 0) return;
  o[0] = (float)((double)s[3] / (double)(400 * area));
  o[1] = (float)((double)s[4] / (double)(512 * area));
  o[2] = (float)((double)s[5] / (double)(512 * area));
  o[3] = (float)((double)(2 * s[1] + area) / (double)(2 * area * W));
  o[4] = (float)((double)(2 * s[2] + area) / (double)(2 * area * H));
  o[5] = (float)((double)area / (double)((long long)H * W));
}

// q = round_half_even(clamp(v, -65536, 65536) * 2^20) (the product is exact in fp32), NaN -> 0
__device__ __forceinline__ long long pool_quant(float v) {
  if (v != v) return 0;
  return __float2ll_rn(fminf(fmaxf(v, -65536.f), 65536.f) * 1048576.f);
}

// one thread per pixel: the lanes of one node are grouped once, then every channel is summed over the group (acc[node][D + 1]:
// D channel sums and the area)
__global__ __launch_bounds__(SP_THREADS) void pool_sum_kernel(const float* __restrict__ feat, int ld, int c_off, int D, const int* __restrict__ labels,
                                                              int64_t n, int64_t HW, const long long* __restrict__ offsets, int64_t cap,
                                                              long long* __restrict__ acc) {
  const int64_t g = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  long long node = -1;
  if (g < n) node = node_index(labels[g], offsets, g / HW, cap);
  const float* src = feat + (g < n ? g : 0) * ld + c_off;
  wave_by_key(
      node,
      [=](long long k, bool mine, bool lead) {
        unsigned long long* a = (unsigned long long*)(acc + k * (D + 1));
        const long long cnt = __popcll(__ballot(mine));
        if (lead) atomicAdd(a + D, (unsigned long long)cnt);
        for (int ch = 0; ch < D; ++ch) {
          const long long s = wave_sum<long long>(mine ? pool_quant(src[ch]) : 0ll);
          if (lead) atomicAdd(a + ch, (unsigned long long)s);
        }
      },
      [=] {
        unsigned long long* a = (unsigned long long*)(acc + node * (D + 1));
        atomicAdd(a + D, 1ull);
        for (int ch = 0; ch < D; ++ch) atomicAdd(a + ch, (unsigned long long)pool_quant(src[ch]));
      });
}

__global__ __launch_bounds__(SP_THREADS) void pool_finish_kernel(const long long* __restrict__ acc, int64_t cap, int D, float* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= cap * D) return;
  const int64_t node = i / D;
  const int ch = (int)(i - node * D);
  const long long area = acc[node * (D + 1) + D];
  out[i] = area > 0 ? (float)((double)acc[node * (D + 1) + ch] / (double)area * 0x1p-20) : 0.f;
}

bool sp_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a && b && na && nb && a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

// the context's device copy of the three host tables, refreshed when their contents change (checked before anything is written:
// lin <= 4095 and rows of m that are >= 0 and sum to 4096 keep xyz inside f; f <= 1024 keeps L, a, b inside 16 bits)
int lab_tables_dev(mgu_ctx* c, const char* fn, const uint16_t* lin, const int32_t* m, const uint16_t* f, hipStream_t s, const LabTables** out) {
  if (!lin || !m || !f) return fail(c, MGU_ERR_INVALID, "%s: the Lab tables (lin, m, f) are host arrays and must be given", fn);
  std::vector<unsigned char> h(sizeof(LabTables), 0);
  LabTables* t = (LabTables*)h.data();
  memcpy(t->lin, lin, sizeof t->lin);
  memcpy(t->m, m, 9 * sizeof(int32_t));
  memcpy(t->f, f, sizeof t->f);
  if (!c->labtab || h != c->labtab_host) {
    for (int i = 0; i < 256; ++i)
      if (t->lin[i] > 4095) return fail(c, MGU_ERR_INVALID, "%s: lin[%d] = %d is above 4095", fn, i, (int)t->lin[i]);
    for (int r = 0; r < 3; ++r) {
      if (t->m[3 * r] < 0 || t->m[3 * r + 1] < 0 || t->m[3 * r + 2] < 0 || t->m[3 * r] + t->m[3 * r + 1] + t->m[3 * r + 2] != 4096)
        return fail(c, MGU_ERR_INVALID, "%s: row %d of m must be >= 0 and sum to 4096", fn, r);
    }
    for (int i = 0; i < 4096; ++i)
      if (t->f[i] > 1024) return fail(c, MGU_ERR_INVALID, "%s: f[%d] = %d is above 1024", fn, i, (int)t->f[i]);
    if (!c->labtab) HIPCHK(c, hipMalloc(&c->labtab, sizeof(LabTables)));
    c->labtab_host.swap(h);
    HIPCHK(c, hipMemcpyAsync(c->labtab, c->labtab_host.data(), sizeof(LabTables), hipMemcpyHostToDevice, s));
  }
  *out = (const LabTables*)c->labtab;
  return MGU_OK;
}

int check_batch(mgu_ctx* c, const char* fn, int B, int H, int W) {
  if (B < 0 || H < 0 || W < 0) return fail(c, MGU_ERR_INVALID, "%s: negative size", fn);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "%s: at most 65535 images per call", fn);
  return check_pixel_count(c, fn, B, H, W);
}

}  // namespace

extern "C" {

int mgu_slic_labels(mgu_ctx* c, const uint8_t* rgb_dev, int B, int H, int W, int step, int mq, int passes, const uint16_t* lin_host,
                    const int32_t* m_host, const uint16_t* f_host, int32_t* raw_labels_dev, int32_t* centres_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B != 0 && (!rgb_dev || !raw_labels_dev)) return fail(c, MGU_ERR_INVALID, "slic_labels: null pointer");
  if (int rc = check_batch(c, "slic_labels", B, H, W)) return rc;
  if (step < 4 || step > 128) return fail(c, MGU_ERR_INVALID, "slic_labels: step %d outside 4..128", step);
  if (mq < 1 || mq > 1024) return fail(c, MGU_ERR_INVALID, "slic_labels: mq %d outside 1..1024 (mq = round(4 * compactness))", mq);
  if (passes < 1 || passes > 32) return fail(c, MGU_ERR_INVALID, "slic_labels: %d passes outside 1..32", passes);
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const int gx = W > 0 ? (W + step - 1) / step : 0, gy = H > 0 ? (H + step - 1) / step : 0;
  const int64_t K = (int64_t)gx * gy, KB = K * B;
  if (sp_overlap(raw_labels_dev, (size_t)n * 4, rgb_dev, (size_t)n * 3) || sp_overlap(centres_dev, (size_t)KB * 24, rgb_dev, (size_t)n * 3) ||
      sp_overlap(centres_dev, (size_t)KB * 24, raw_labels_dev, (size_t)n * 4))
    return fail(c, MGU_ERR_INVALID, "slic_labels: an output overlaps the image or the other output");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (n == 0) return MGU_OK;
  const LabTables* tab;
  if (int rc = lab_tables_dev(c, "slic_labels", lin_host, m_host, f_host, s, &tab)) return rc;
  Carve cv;
  const size_t oL = cv.take((size_t)n * 8), oC = cv.take((size_t)KB * 24), oA = cv.take((size_t)KB * 24);
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
  char* ws = (char*)c->objws;
  int2* lab = (int2*)(ws + oL);
  int* cen = centres_dev ? (int*)centres_dev : (int*)(ws + oC);
  int* acc = (int*)(ws + oA);
  const unsigned pixblocks = grid_for(n, SP_THREADS, INT_MAX), cenblocks = grid_for(KB, SP_THREADS, INT_MAX);
  const dim3 tiles((W + SP_TILE - 1) / SP_TILE, (H + SP_TILE - 1) / SP_TILE, B);
  const long long mq2 = (long long)mq * mq;
  {
    ProfScope p(c, s, "slic_lab");
    hipLaunchKernelGGL(slic_lab_kernel, dim3(pixblocks), dim3(SP_THREADS), 0, s, rgb_dev, n, tab, lab);
  }
  {
    ProfScope p(c, s, "slic_init");
    hipLaunchKernelGGL(slic_init_kernel, dim3(cenblocks), dim3(SP_THREADS), 0, s, lab, KB, H, W, step, gx, gy, cen, acc);
  }
  for (int t = 1; t < passes; ++t) {
    {
      ProfScope p(c, s, "slic_assign");
      hipLaunchKernelGGL(slic_assign_kernel<false>, tiles, dim3(SP_THREADS), 0, s, lab, cen, acc, (int*)nullptr, H, W, step, gx, gy, mq2);
    }
    ProfScope p(c, s, "slic_update");
    hipLaunchKernelGGL(slic_update_kernel, dim3(cenblocks), dim3(SP_THREADS), 0, s, KB, step, gx, gy, cen, acc);
  }
  {
    ProfScope p(c, s, "slic_assign");
    hipLaunchKernelGGL(slic_assign_kernel<true>, tiles, dim3(SP_THREADS), 0, s, lab, cen, acc, (int*)raw_labels_dev, H, W, step, gx, gy, mq2);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_regions_connect(mgu_ctx* c, const int32_t* raw_labels_dev, int B, int H, int W, int min_area, int rounds, int32_t* labels_dev,
                        int64_t* counts_dev, int64_t* offsets_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B != 0 && (!raw_labels_dev || !labels_dev || !counts_dev || !offsets_dev)) return fail(c, MGU_ERR_INVALID, "regions_connect: null pointer");
  if (int rc = check_batch(c, "regions_connect", B, H, W)) return rc;
  if (min_area < 0) return fail(c, MGU_ERR_INVALID, "regions_connect: min_area %d is negative", min_area);
  if (rounds < 0 || rounds > 8) return fail(c, MGU_ERR_INVALID, "regions_connect: %d rounds outside 0..8", rounds);
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const void* outs[3] = {labels_dev, counts_dev, offsets_dev};
  const size_t out_bytes[3] = {(size_t)n * 4, (size_t)B * 8, (size_t)(B + 1) * 8};
  for (int i = 0; i < 3; ++i) {
    if (sp_overlap(outs[i], out_bytes[i], raw_labels_dev, (size_t)n * 4)) return fail(c, MGU_ERR_INVALID, "regions_connect: an output overlaps raw_labels");
    for (int j = 0; j < i; ++j)
      if (sp_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return fail(c, MGU_ERR_INVALID, "regions_connect: two outputs overlap");
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (B == 0) return MGU_OK;
  if (n == 0) return clear_counts(c, B, counts_dev, offsets_dev, s);
  const int64_t nch = cc_chunks(HW);
  PairTable t;
  t.slots = (unsigned)std::min<int64_t>(4 * n + 64, 0xFFFFFFFFll);   // distinct (small, large) pairs <= pixel edges < 2 n: at most half full
  t.rows = n, t.deg = nullptr;
  Carve cv;
  const size_t oM = cv.take((size_t)n * 4), oP = cv.take((size_t)n * 4), oA = cv.take((size_t)n * 4), oC = cv.take((size_t)nch * B * 4),
               oO = cv.take((size_t)nch * B * 8), oK = cv.take((size_t)t.slots * 8), oZ = cv.take((size_t)t.slots * 4), oB = cv.take((size_t)n * 8);
  const size_t zero_bytes = cv.off - oZ;   // pair counts and the best words are cleared together
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
  char* ws = (char*)c->objws;
  int *map = (int*)(ws + oM), *P = (int*)(ws + oP), *cnt = (int*)(ws + oC);
  unsigned* area = (unsigned*)(ws + oA);
  long long* choff = (long long*)(ws + oO);
  unsigned long long* best = (unsigned long long*)(ws + oB);
  t.keys = (unsigned long long*)(ws + oK), t.cnt = (unsigned*)(ws + oZ);
  const unsigned pixblocks = grid_for(n, SP_THREADS, INT_MAX), slotblocks = grid_for(t.slots, SP_THREADS, 4096);
  {
    ProfScope p(c, s, "regions_shift");
    hipLaunchKernelGGL(shift_labels_kernel, dim3(pixblocks), dim3(SP_THREADS), 0, s, (const int*)raw_labels_dev, n, 1, map);
  }
  {
    ProfScope p(c, s, "regions_components");
    if (int rc = cc_roots_i32(c, map, B, H, W, P, s, false)) return rc;
  }
  {
    ProfScope p(c, s, "regions_number");
    if (int rc = cc_number_roots(c, P, area, 0, B, HW, cnt, choff, labels_dev, counts_dev, offsets_dev, s)) return rc;
  }
  for (int r = 0; r < rounds; ++r) {
    HIPCHK(c, hipMemsetAsync(t.keys, 0xFF, (size_t)t.slots * 8, s));
    HIPCHK(c, hipMemsetAsync(t.cnt, 0, zero_bytes, s));
    {
      ProfScope p(c, s, "regions_merge_count");
      hipLaunchKernelGGL(merge_count_kernel, dim3(pixblocks), dim3(SP_THREADS), 0, s, P, area, (unsigned)min_area, n, H, W, t);
    }
    {
      ProfScope p(c, s, "regions_merge_best");
      hipLaunchKernelGGL(merge_best_kernel, dim3(slotblocks), dim3(SP_THREADS), 0, s, t, best);
    }
    {
      ProfScope p(c, s, "regions_merge_apply");
      hipLaunchKernelGGL(merge_min_kernel, dim3(pixblocks), dim3(SP_THREADS), 0, s, best, n, P);
      hipLaunchKernelGGL(merge_link_kernel, dim3(pixblocks), dim3(SP_THREADS), 0, s, best, n, P);
    }
    ProfScope p(c, s, "regions_number");
    if (int rc = cc_number_roots(c, P, area, 0, B, HW, cnt, choff, labels_dev, counts_dev, offsets_dev, s)) return rc;
  }
  {
    ProfScope p(c, s, "regions_shift");   // cc_number_roots numbers from 1 (0 is its background); regions are numbered from 0
    hipLaunchKernelGGL(shift_labels_kernel, dim3(pixblocks), dim3(SP_THREADS), 0, s, (const int*)labels_dev, n, -1, (int*)labels_dev);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_regions_adjacency(mgu_ctx* c, const int32_t* labels_dev, const int64_t* offsets_dev, int B, int H, int W, int64_t node_capacity,
                          int64_t edge_capacity, int32_t* rowptr_dev, int32_t* col_dev, int32_t* border_dev, int32_t* status_dev,
                          void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B != 0 && (!labels_dev || !offsets_dev || !rowptr_dev || !status_dev)) return fail(c, MGU_ERR_INVALID, "regions_adjacency: null pointer");
  if (int rc = check_batch(c, "regions_adjacency", B, H, W)) return rc;
  if (node_capacity < 0 || edge_capacity < 0 || node_capacity >= 2147483647ll || edge_capacity >= 2147483647ll)
    return fail(c, MGU_ERR_INVALID, "regions_adjacency: capacities must lie in [0, 2^31 - 1)");
  if (B != 0 && edge_capacity > 0 && (!col_dev || !border_dev)) return fail(c, MGU_ERR_INVALID, "regions_adjacency: col and border are needed for a nonzero edge_capacity");
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  if (4 * n >= 2147483647ll) return fail(c, MGU_ERR_INVALID, "regions_adjacency: B*H*W must stay below 2^29 (directed edges are counted in int32)");
  const void* outs[4] = {rowptr_dev, col_dev, border_dev, status_dev};
  const size_t out_bytes[4] = {(size_t)(node_capacity + 1) * 4, (size_t)edge_capacity * 4, (size_t)edge_capacity * 4, 4};
  for (int i = 0; i < 4; ++i) {
    if (sp_overlap(outs[i], out_bytes[i], labels_dev, (size_t)n * 4) || sp_overlap(outs[i], out_bytes[i], offsets_dev, (size_t)(B + 1) * 8))
      return fail(c, MGU_ERR_INVALID, "regions_adjacency: an output overlaps an input");
    for (int j = 0; j < i; ++j)
      if (sp_overlap(outs[i], out_bytes[i], outs[j], out_bytes[j])) return fail(c, MGU_ERR_INVALID, "regions_adjacency: two outputs overlap");
  }
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (B == 0) return MGU_OK;
  const int64_t nptr = node_capacity + 1;
  PairTable t;
  t.rows = std::min<int64_t>(node_capacity, n);   // an image has at most H*W regions: no row past n can be a node's
  // directed pairs <= 2 * pixel edges < 4 n, and <= rows^2: the table stays at most half full
  const double sq = 2.0 * (double)t.rows * (double)t.rows + 64.0;
  t.slots = (unsigned)std::min<double>(std::min<double>(8.0 * (double)n + 64.0, sq), 4294967295.0);
  const int64_t maxpairs = std::min<int64_t>(4 * n, (int64_t)(t.slots / 2)) + 1;
  const int64_t nch = (nptr + PAIR_ROWCHUNK - 1) / PAIR_ROWCHUNK;
  Carve cv;
  const size_t oK = cv.take((size_t)t.slots * 8), oZ = cv.take((size_t)t.slots * 4), oD = cv.take((size_t)(t.rows + 1) * 4);
  const size_t zero_bytes = cv.off - oZ;
  const size_t oP = cv.take((size_t)maxpairs * 4), oG = cv.take((size_t)maxpairs * 4), oC = cv.take((size_t)maxpairs * 4);
  const size_t oS = cv.take((size_t)nch * 4), oO = cv.take((size_t)nch * 8), oT = cv.take(8);
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
  char* ws = (char*)c->objws;
  t.keys = (unsigned long long*)(ws + oK), t.cnt = (unsigned*)(ws + oZ), t.deg = (int*)(ws + oD);
  int *tp = (int*)(ws + oP), *csum = (int*)(ws + oS);
  unsigned *tg = (unsigned*)(ws + oG), *tc = (unsigned*)(ws + oC);
  long long *choff = (long long*)(ws + oO), *total = (long long*)(ws + oT);
  const long long* off = (const long long*)offsets_dev;
  HIPCHK(c, hipMemsetAsync(t.keys, 0xFF, (size_t)t.slots * 8, s));
  HIPCHK(c, hipMemsetAsync(t.cnt, 0, zero_bytes, s));
  {
    ProfScope p(c, s, "adjacency_count");
    hipLaunchKernelGGL(adj_count_kernel, dim3(grid_for(n, SP_THREADS, INT_MAX)), dim3(SP_THREADS), 0, s, (const int*)labels_dev, n, H, W, off,
                       t.rows, t);
  }
  {
    ProfScope p(c, s, "adjacency_scan");
    hipLaunchKernelGGL(degree_count_kernel<0>, dim3((unsigned)nch), dim3(PAIR_THREADS), 0, s, t.deg, t.rows, csum);
    hipLaunchKernelGGL(adj_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, csum, nch, choff, total, edge_capacity, B, off, node_capacity,
                       (int*)status_dev);
    hipLaunchKernelGGL(degree_write_kernel<int>, dim3((unsigned)nch), dim3(PAIR_THREADS), 0, s, t.deg, t.rows, nptr, choff, (int*)rowptr_dev);
  }
  {
    ProfScope p(c, s, "adjacency_pour");
    hipLaunchKernelGGL(pair_pour_kernel<int>, dim3(grid_for(t.slots, PAIR_THREADS, 4096)), dim3(PAIR_THREADS), 0, s, t, (const int*)rowptr_dev, tp,
                       tg, tc);
  }
  {
    ProfScope p(c, s, "adjacency_place");
    hipLaunchKernelGGL((pair_place_kernel<int, int>), dim3(grid_for(maxpairs, PAIR_THREADS, 4096)), dim3(PAIR_THREADS), 0, s, total,
                       (const int*)rowptr_dev, tp, tg, tc, edge_capacity, (int*)col_dev, (int*)border_dev);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_regions_features_u8(mgu_ctx* c, const uint8_t* rgb_dev, const int32_t* labels_dev, const int64_t* offsets_dev, int B, int H, int W,
                            const uint16_t* lin_host, const int32_t* m_host, const uint16_t* f_host, int64_t node_capacity, float* feat_dev,
                            int64_t* stats_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B != 0 && node_capacity != 0 && (!rgb_dev || !labels_dev || !offsets_dev || !feat_dev)) return fail(c, MGU_ERR_INVALID, "regions_features_u8: null pointer");
  if (int rc = check_batch(c, "regions_features_u8", B, H, W)) return rc;
  if (node_capacity < 0 || node_capacity >= 2147483647ll) return fail(c, MGU_ERR_INVALID, "regions_features_u8: node_capacity must lie in [0, 2^31 - 1)");
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const void* ins[3] = {rgb_dev, labels_dev, offsets_dev};
  const size_t in_bytes[3] = {(size_t)n * 3, (size_t)n * 4, (size_t)(B + 1) * 8};
  for (int i = 0; i < 3; ++i)
    if (sp_overlap(feat_dev, (size_t)node_capacity * 32, ins[i], in_bytes[i]) || sp_overlap(stats_dev, (size_t)node_capacity * 48, ins[i], in_bytes[i]))
      return fail(c, MGU_ERR_INVALID, "regions_features_u8: an output overlaps an input");
  if (sp_overlap(feat_dev, (size_t)node_capacity * 32, stats_dev, (size_t)node_capacity * 48))
    return fail(c, MGU_ERR_INVALID, "regions_features_u8: the two outputs overlap");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (B == 0 || node_capacity == 0) return MGU_OK;
  const LabTables* tab;
  if (int rc = lab_tables_dev(c, "regions_features_u8", lin_host, m_host, f_host, s, &tab)) return rc;
  long long* stats = (long long*)stats_dev;
  if (!stats) {
    if (int rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)node_capacity * 48)) return rc;
    stats = (long long*)c->objws;
  }
  const unsigned capblocks = grid_for(node_capacity, SP_THREADS, INT_MAX);
  {
    ProfScope p(c, s, "features_clear");
    hipLaunchKernelGGL(zero_i64_kernel, dim3(grid_for(node_capacity * 6, SP_THREADS, 4096)), dim3(SP_THREADS), 0, s, stats, node_capacity * 6);
  }
  if (n > 0) {
    ProfScope p(c, s, "features_sum");
    hipLaunchKernelGGL(feat_sum_kernel, dim3(grid_for(n, SP_THREADS, INT_MAX)), dim3(SP_THREADS), 0, s, rgb_dev, (const int*)labels_dev, n, H, W,
                       (const long long*)offsets_dev, node_capacity, tab, stats);
  }
  {
    ProfScope p(c, s, "features_finish");
    hipLaunchKernelGGL(feat_finish_kernel, dim3(capblocks), dim3(SP_THREADS), 0, s, stats, node_capacity, H, W, feat_dev);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_regions_pool_nhwc(mgu_ctx* c, const float* feat_dev, int ld, int c_off, int D, const int32_t* labels_dev, const int64_t* offsets_dev,
                          int B, int H, int W, int64_t node_capacity, float* out_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B != 0 && node_capacity != 0 && (!feat_dev || !labels_dev || !offsets_dev || !out_dev)) return fail(c, MGU_ERR_INVALID, "regions_pool_nhwc: null pointer");
  if (int rc = check_batch(c, "regions_pool_nhwc", B, H, W)) return rc;
  if (D < 1 || D > 4096 || c_off < 0 || ld < c_off + D) return fail(c, MGU_ERR_INVALID, "regions_pool_nhwc: channels [%d, %d + %d) of a pitch of %d (D in 1..4096)", c_off, c_off, D, ld);
  if (node_capacity < 0 || node_capacity >= 2147483647ll) return fail(c, MGU_ERR_INVALID, "regions_pool_nhwc: node_capacity must lie in [0, 2^31 - 1)");
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const size_t ob = (size_t)node_capacity * D * 4;
  if (sp_overlap(out_dev, ob, feat_dev, (size_t)n * ld * 4) || sp_overlap(out_dev, ob, labels_dev, (size_t)n * 4) ||
      sp_overlap(out_dev, ob, offsets_dev, (size_t)(B + 1) * 8))
    return fail(c, MGU_ERR_INVALID, "regions_pool_nhwc: the output overlaps an input");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (B == 0 || node_capacity == 0) return MGU_OK;
  const int64_t words = node_capacity * (D + 1);
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)words * 8)) return rc;
  long long* acc = (long long*)c->objws;
  {
    ProfScope p(c, s, "pool_clear");
    hipLaunchKernelGGL(zero_i64_kernel, dim3(grid_for(words, SP_THREADS, 4096)), dim3(SP_THREADS), 0, s, acc, words);
  }
  if (n > 0) {
    ProfScope p(c, s, "pool_sum");
    hipLaunchKernelGGL(pool_sum_kernel, dim3(grid_for(n, SP_THREADS, INT_MAX)), dim3(SP_THREADS), 0, s, feat_dev, ld, c_off, D, (const int*)labels_dev,
                       n, HW, (const long long*)offsets_dev, node_capacity, acc);
  }
  {
    ProfScope p(c, s, "pool_finish");
    hipLaunchKernelGGL(pool_finish_kernel, dim3(grid_for(node_capacity * D, SP_THREADS, INT_MAX)), dim3(SP_THREADS), 0, s, acc, node_capacity, D, out_dev);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
