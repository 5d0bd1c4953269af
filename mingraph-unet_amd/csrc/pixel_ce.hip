// Imbalance-aware pixel-wise cross-entropy, value and gradient on the device (the definition is INTEGRATION.md section S):
//   mgu_pixel_ce            loss value (+ the test hooks: the per-pixel loss plane and the kept map)
//   mgu_pixel_ce_backward   d loss / d logits (+ the value of the same pass)
// Per counted pixel (label != ignore_index) with lp the fp32 log-softmax, p the softmax, w the class weights (absent: ones):
//   gamma == 0   l = (1 - eps) w_y (-lp_y) + (eps / C) sum_c w_c (-lp_c)       torch's F.cross_entropy(weight, label_smoothing) per pixel
//   gamma >= 1   l = w_y (1 - p_y)^gamma (-lp_y)                               the focal loss (eps must be 0); 1 - p_y as PixelCE::miss
// clamped to >= +0.0f; its fp32 bits are the ranking key (31 bits).  A group is the batch or one image; of its n counted pixels the
// K = min(n, max(min_kept, ceil(keep_fraction * n))) (IEEE double) with the largest l are KEPT, among equal fp32 l the lower pixel index
// (b, y, x) first: part of the interface.  keep_fraction == 1 keeps every counted pixel and runs no select.
//   L = sum_kept l / sum_kept w_y     one numerator, one denominator over all groups; both sums in double in a fixed order
// and the gradient is that of exactly this expression with the kept set held fixed: ignored and dropped pixels get exact zeros.
//   mgu_pixel_ce_map / mgu_pixel_ce_map_backward   the same with a per-pixel weight map m >= 0 (fp32, one per pixel, e.g. border.hip's):
// the pixel's loss is m l (clamped to >= +0.0f, the key the select ranks), L = sum_kept m l / sum_kept m w_y, m held fixed in the
// gradient.  The same kernels, instantiated a second time with the map read in (the entries without one run the code they ran before),
// and the same launch counts; without a map, or with m == 1 everywhere, the same bits.
//
// The select is a radix SELECT, not a sort: four counting passes over 8 + 8 + 8 + 7 key bits from the top.  A pass counts the keys
// that match the prefix chosen so far into 256 bins per group (LDS counters per workgroup, then integer atomic adds of the non-empty
// bins to the group's row: a count does not depend on arrival order); the digit where the count from above crosses the remaining K
// is the next digit of the threshold key t, and what is left of K after the last pass is r, the pixels with key == t still to keep.
// No kernel of its own picks a digit: every workgroup repeats the pick of the earlier passes from the group's rows (256 counts each).
// Ties are decided as lovasz.hip decides positions, no atomic deciding anything: per-tile counts of key == t, an exclusive scan along
// the group's tiles, and inside a tile the rank among the equals from wave ballots + mbcnt in the fixed (wave, item, lane) order;
// a pixel with key == t is kept iff that rank is < r.
// Launches, whatever B, C, per_image and the data are (no host synchronisation, no host read of n or K):
//   keep_fraction == 1   2 for the value (sums, finish), 3 with the gradient (+ the gradient rows)
//   keep_fraction <  1   8 for the value (pixel losses + top digit, three counting passes, tie counts, tie scan, sums, finish), 9 with
//                        the gradient; before them one memset of the digit counters
// The sums pass marks a dropped pixel in the loss plane (the key's free sign bit), so the gradient pass reads one word to know.  The
// gradient pass reads the logits once more instead of keeping softmaxes.
// Scratch (the context's, grown on first use), P = B*HW, G = per_image ? B : 1, T = G * ceil(P / G / mgu_pixel_ce_tile()) tiles, each
// region rounded up to 256 bytes: 16 * T of partial sums + 16; with the select also 4 * P (the loss plane) + 4096 * G (digit counters)
// + 4 * T (tie counts) + 8 * G (thresholds): 8 x 512 x 512 over the batch: 8 403 456 bytes = 8.0 MiB.
#include <algorithm>

#include "loss_common.h"
#include "objects_common.h"

namespace mgu {

// a workgroup counts the LOSS_TILE keys of one tile (loss_common.h) per pass
constexpr unsigned PC_IGNORED = 0xFFFFFFFFu; // loss plane: a pixel that is not counted (ignore_index or a label outside [0, C))
constexpr unsigned PC_DROPPED = 0x80000000u; // loss plane: set by the sums pass on a counted pixel that is not kept
constexpr int PC_PASSES = 4;
// the digits of the 31 key bits from the top: 8 + 8 + 8 + 7
__host__ __device__ constexpr int pc_shift(int pass) { return pass == 3 ? 0 : 23 - 8 * pass; }
__host__ __device__ constexpr int pc_bins(int pass) { return pass == 3 ? 128 : 256; }

// what every kernel knows of the call: the shared descriptor and this loss's options
struct PcCall : LossCall {
  const float* weight;   // C class weights or nullptr
  const float* pmap;     // the per-pixel weight map m (P floats) of the _map entries, or nullptr
  long long min_kept;
  double keep;
  float eps, gamma;
};
static_assert(std::is_trivially_copyable<PcCall>::value, "a kernel argument by value");

// One counted pixel: the softmax pieces and its loss.  Contraction is off: the select's passes and the sums must see the same bits.
template <int NC>
struct PcPixel {
  float e[NC], w[NC];   // exp(l_c - max) (softmax_front), class weights
  float inv, loss, miss, py, ty;   // 1 / sum e; the loss; 1 - p_y; p_y; -lp_y
};
template <int NC>
__device__ __forceinline__ void pc_weights(const PcCall& k, float (&w)[NC]) {
#pragma unroll
  for (int c = 0; c < NC; ++c) w[c] = c < k.C ? (k.weight ? k.weight[c] : 1.f) : 0.f;
}
template <int NC, bool MAP>
__device__ __forceinline__ void pc_pixel(const PcCall& k, int q, int y, PcPixel<NC>& x) {
#pragma clang fp contract(off)
  const int b = q / k.HW;
  const float* p = k.logits + b * k.ls_n + (int64_t)(q - b * k.HW) * k.ls_p;
  float l[NC], mx, ly = 0.f, ey = 0.f;
  PixelCE s;   // fed in class order as the front end forms e: s.se is its sum, the same adds in the same order (a padded class adds 0.f)
  softmax_front(p, k.ls_c, k.C, x.e, mx, &l, [&](int c, float e) {
    if (c < k.C) s.add(c, e);
    if (c == y) ey = e;
  });
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c == y) ly = l[c];
  x.inv = 1.f / s.se;
  x.ty = s.term(mx, ly);
  x.miss = s.miss(y, ey);
  x.py = ey * x.inv;
  float wy = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c == y) wy = x.w[c];
  float v;
  if (k.gamma > 0.f) {
    const float pw1 = k.gamma == 1.f ? 1.f : (k.gamma == 2.f ? x.miss : powf(x.miss, k.gamma - 1.f));
    v = wy * (pw1 * x.miss) * x.ty;
  } else {
    v = (1.f - k.eps) * wy * x.ty;
    if (k.eps > 0.f) {
      const float lse = log1pf(s.rest);
      float sm = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < k.C) sm += x.w[c] * (lse + (mx - l[c]));
      v += (k.eps / (float)k.C) * sm;
    }
  }
  if (MAP) v = k.pmap[q] * v;   // the _map entries rank, sum and differentiate m * l
  x.loss = v > 0.f ? v : 0.f;   // >= +0.0f (a NaN too): the key stays inside 31 bits
}
// the pixel's share of the denominator: w_y, times m in the _map entries (m == 1 leaves the double as it is).  MAP is a template
// argument of every kernel that reads the map, so the entries without one run the code they ran before it existed.
template <bool MAP>
__device__ __forceinline__ double pc_den(const PcCall& k, int q, int y) {
  const double wy = (double)(k.weight ? k.weight[y] : 1.f);
  return MAP ? (double)k.pmap[q] * wy : wy;
}
// d loss / d logit_j of that pixel (contraction off, as above).  Both forms are A (p_j - [j == y]) plus the smoothing term, with p_y - 1 as -miss (no cancellation)
// and sum_c w_c (p_j - [j == c]) as p_j (W - w_j) - w_j (1 - p_j).
template <int NC>
__device__ __forceinline__ void pc_row(const PcCall& k, int y, const PcPixel<NC>& x, float (&d)[NC]) {
#pragma clang fp contract(off)
  float wy = 0.f;
#pragma unroll
  for (int c = 0; c < NC; ++c)
    if (c == y) wy = x.w[c];
  float A;
  if (k.gamma > 0.f) {
    const float pw1 = k.gamma == 1.f ? 1.f : (k.gamma == 2.f ? x.miss : powf(x.miss, k.gamma - 1.f));
    A = wy * (k.gamma * pw1 * x.py * x.ty + pw1 * x.miss);
  } else {
    A = (1.f - k.eps) * wy;
  }
  const float sm = k.gamma > 0.f ? 0.f : k.eps / (float)k.C;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const float pj = x.e[j] * x.inv;
    float v = j == y ? -A * x.miss : A * pj;
    if (sm > 0.f) {
      float rest = 0.f;   // W - w_j
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c != j) rest += x.w[c];
      const float mj = j == y ? x.miss : 1.f - pj;
      v += sm * (pj * rest - x.w[j] * mj);
    }
    d[j] = j < k.C ? v : 0.f;
  }
}

// ---- the select ---------------------------------------------------------------------------------------------------------------------
// hist[(pass * G + g) * 256 + digit]: the group's keys that match the prefix of the earlier passes, by the digit of this pass
__device__ __forceinline__ int* pc_row_of(int* hist, const PcCall& k, int pass, int g) { return hist + ((size_t)pass * k.G + g) * 256; }

// The whole workgroup (256 threads) walks the passes [0, NP) of group g: per pass the digit d with
//   (keys with a larger digit) < K <= (keys with a larger or that digit),  K -= (keys with a larger digit)
// K starts as the group's K from its counted pixels n, the sum of the first pass's row.  Returns the prefix of the digits chosen
// (the threshold key after four passes) and leaves the rest of K in `rem`; a group that keeps nothing (n == 0): prefix PC_IGNORED, rem 0.
__device__ __forceinline__ unsigned pc_threshold(const PcCall& k, int* hist, int g, int NP, int& rem, int* shs /* 4 */, int* shp /* 2 */) {
  unsigned prefix = 0;
  long long K = 0;
  bool none = false;
  for (int pass = 0; pass < NP; ++pass) {
    const int bins = pc_bins(pass), d = bins - 1 - (int)threadIdx.x;   // thread 0 holds the largest digit
    const int v = d >= 0 ? pc_row_of(hist, k, pass, g)[d] : 0;
    int total;
    const int above = block_exclusive_scan(v, shs, &total);
    if (pass == 0) {
      const long long byf = (long long)ceil(k.keep * (double)total);
      K = k.min_kept > byf ? k.min_kept : byf;
      if (K > total) K = total;
    }
    if (threadIdx.x == 0) shp[0] = -1, shp[1] = 0;
    __syncthreads();
    if (v > 0 && above < K && K <= (long long)above + v) shp[0] = d, shp[1] = (int)(K - above);
    __syncthreads();
    const int digit = shp[0];
    K = shp[1];
    __syncthreads();
    if (digit < 0) none = true;
    prefix = (prefix << (pass == 3 ? 7 : 8)) | (unsigned)(digit & 0xFF);
  }
  rem = none ? 0 : (int)K;
  return none ? PC_IGNORED : prefix;
}

// the workgroup's LDS counters go to the group's row (integer adds: the sum does not depend on their order)
__device__ __forceinline__ void pc_flush(int* cnt, int* row, int bins) {
  __syncthreads();
  for (int d = threadIdx.x; d < bins; d += 256)
    if (cnt[d]) atomicAdd(&row[d], cnt[d]);
}

// pass 0: the loss of every pixel into the plane (PC_IGNORED where it is not counted), the hook, and the counts of the top digit
template <int NC, bool MAP>
__global__ __launch_bounds__(256) void pc_loss_kernel(PcCall k, unsigned* __restrict__ plane, int* __restrict__ hist,
                                                      float* __restrict__ pixel_loss, int* __restrict__ err_word) {
  __shared__ int cnt[256];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const LossTile t = loss_tile(k);
  PcPixel<NC> x;
  pc_weights(k, x.w);
  bool bad = false;
#pragma unroll 2
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const int j = i * 256 + threadIdx.x;
    if (j >= t.n) continue;
    const int q = t.first + j;
    const long long y = k.labels[q];
    unsigned key = PC_IGNORED;
    if (y != k.ignore) {
      if (y < 0 || y >= k.C) {
        bad = true;
      } else {
        pc_pixel<NC, MAP>(k, q, (int)y, x);
        key = __float_as_uint(x.loss);
        atomicAdd(&cnt[key >> 23], 1);
      }
    }
    plane[q] = key;
    if (pixel_loss) pixel_loss[q] = key == PC_IGNORED ? 0.f : __uint_as_float(key);
  }
  if (bad && err_word) atomicOr(err_word, 1);
  pc_flush(cnt, pc_row_of(hist, k, 0, t.g), 256);
}

// passes 1 .. 3: the keys under the prefix of the earlier passes, by this pass's digit
__global__ __launch_bounds__(256) void pc_count_kernel(PcCall k, const unsigned* __restrict__ plane, int* __restrict__ hist, int pass) {
  __shared__ int cnt[256];
  __shared__ int shs[4], shp[2];
  const LossTile t = loss_tile(k);
  int rem;
  const unsigned prefix = pc_threshold(k, hist, t.g, pass, rem, shs, shp);
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const int above = pc_shift(pass - 1), shift = pc_shift(pass), mask = pc_bins(pass) - 1;
  if (prefix != PC_IGNORED) {
#pragma unroll 4
    for (int i = 0; i < LOSS_ITEMS; ++i) {
      const int j = i * 256 + threadIdx.x;
      if (j >= t.n) continue;
      const unsigned key = plane[t.first + j];
      if (key != PC_IGNORED && (key >> above) == prefix) atomicAdd(&cnt[(key >> shift) & mask], 1);
    }
  }
  pc_flush(cnt, pc_row_of(hist, k, pass, t.g), pc_bins(pass));
}

// keys equal to the threshold per tile
__global__ __launch_bounds__(256) void pc_tie_count_kernel(PcCall k, const unsigned* __restrict__ plane, int* __restrict__ hist,
                                                           int* __restrict__ ties) {
  __shared__ int shs[4], shp[2];
  const LossTile t = loss_tile(k);
  int rem;
  const unsigned thr = pc_threshold(k, hist, t.g, PC_PASSES, rem, shs, shp);
  int s = 0;
  if (thr != PC_IGNORED) {
#pragma unroll 4
    for (int i = 0; i < LOSS_ITEMS; ++i) {
      const int j = i * 256 + threadIdx.x;
      if (j < t.n) s += plane[t.first + j] == thr;
    }
  }
  int total;
  block_exclusive_scan(s, shs, &total);
  if (threadIdx.x == 0) ties[(size_t)t.g * k.tiles_g + t.tile] = total;
}

// one workgroup per group: the tie counts become their exclusive prefix along the group's tiles, state[g] = {threshold key, r}
__global__ __launch_bounds__(256) void pc_tie_scan_kernel(PcCall k, int* __restrict__ hist, int* __restrict__ ties, unsigned* __restrict__ state) {
  __shared__ int shs[4], shp[2];
  const int g = blockIdx.x;
  int rem;
  const unsigned thr = pc_threshold(k, hist, g, PC_PASSES, rem, shs, shp);
  if (threadIdx.x == 0) state[2 * g] = thr, state[2 * g + 1] = (unsigned)rem;
  int* p = ties + (size_t)g * k.tiles_g;
  int carry = 0;
  for (int base = 0; base < k.tiles_g; base += 256) {   // uniform trip count: the scan's barriers are met by every thread
    const int j = base + threadIdx.x, v = j < k.tiles_g ? p[j] : 0;
    int total;
    const int ex = block_exclusive_scan(v, shs, &total);
    if (j < k.tiles_g) p[j] = carry + ex;
    carry += total;
  }
}

// ---- sums, finish, gradient ---------------------------------------------------------------------------------------------------------
// part[2 * (g * tiles_g + tile)] = sum of the kept losses of the tile, [+ 1] = sum of their w_y (double).  With the select the kept
// test reads the plane and marks the dropped pixels in it; without it the losses are formed here and every counted pixel is kept.
template <int NC, bool SELECT, bool MAP>
__global__ __launch_bounds__(256) void pc_sum_kernel(PcCall k, unsigned* __restrict__ plane, const int* __restrict__ ties,
                                                     const unsigned* __restrict__ state, double* __restrict__ part,
                                                     float* __restrict__ pixel_loss, int* __restrict__ kept, int* __restrict__ err_word) {
  __shared__ int shw[4];
  __shared__ double shd[8];
  const LossTile t = loss_tile(k);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc[2] = {0.0, 0.0};
  bool bad = false;
  if (SELECT) {
    const unsigned thr = state[2 * t.g];
    const int r = (int)state[2 * t.g + 1];
    unsigned key[LOSS_ITEMS];
    int rank[LOSS_ITEMS], mine = 0;   // rank among the wave's pixels with key == thr; mine: how many the wave holds
#pragma unroll
    for (int i = 0; i < LOSS_ITEMS; ++i) {
      const int j = loss_item(i);
      key[i] = j < t.n ? plane[t.first + j] : PC_IGNORED;
      const unsigned long long m = __ballot(key[i] == thr && thr != PC_IGNORED);
      rank[i] = mine + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
      mine += __popcll(m);
    }
    if (lane == 0) shw[wave] = mine;
    __syncthreads();
    int before = ties[(size_t)t.g * k.tiles_g + t.tile];
    for (int w = 0; w < wave; ++w) before += shw[w];
#pragma unroll
    for (int i = 0; i < LOSS_ITEMS; ++i) {
      const int j = loss_item(i);
      if (j >= t.n) continue;
      const int q = t.first + j;
      const long long y = k.labels[q];
      if (key[i] == PC_IGNORED) {
        if (y != k.ignore) acc[0] += (double)NAN;   // a label outside [0, C): the loss comes out NaN
        if (kept) kept[q] = -1;
        continue;
      }
      const bool keep = thr != PC_IGNORED && (key[i] > thr || (key[i] == thr && before + rank[i] < r));
      if (keep) {
        acc[0] += (double)__uint_as_float(key[i]);
        acc[1] += pc_den<MAP>(k, q, (int)y);
      } else {
        plane[q] = key[i] | PC_DROPPED;
      }
      if (kept) kept[q] = keep;
    }
  } else {
    PcPixel<NC> x;
    pc_weights(k, x.w);
#pragma unroll 2
    for (int i = 0; i < LOSS_ITEMS; ++i) {
      const int j = loss_item(i);
      if (j >= t.n) continue;
      const int q = t.first + j;
      const long long y = k.labels[q];
      const bool counted = y != k.ignore && y >= 0 && y < k.C;
      float v = 0.f;
      if (counted) {
        pc_pixel<NC, MAP>(k, q, (int)y, x);
        v = x.loss;
        acc[0] += (double)v;
        acc[1] += pc_den<MAP>(k, q, (int)y);
      } else if (y != k.ignore) {
        bad = true;
        acc[0] += (double)NAN;
      }
      if (pixel_loss) pixel_loss[q] = v;
      if (kept) kept[q] = counted ? 1 : -1;
    }
    if (bad && err_word) atomicOr(err_word, 1);
  }
  block_fold<2>(acc, shd);
  if (threadIdx.x == 0) {
    const size_t at = 2 * ((size_t)t.g * k.tiles_g + t.tile);
    part[at] = acc[0], part[at + 1] = acc[1];
  }
}

// the partial sums in a fixed order: thread i takes tiles i, i + 256, ..., thread 0 adds the 256 results in index order.
// fin[0] = the numerator, fin[1] = the denominator; loss = their quotient (0 / 0 = NaN, as torch's mean over no pixel)
__global__ __launch_bounds__(256) void pc_finish_kernel(const double* __restrict__ part, int tiles, double* __restrict__ fin,
                                                        float* __restrict__ loss) {
  __shared__ double sh[2][256];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < tiles; i += 256) a += part[2 * (size_t)i], b += part[2 * (size_t)i + 1];
  sh[0][threadIdx.x] = a, sh[1][threadIdx.x] = b;
  __syncthreads();
  if (threadIdx.x != 0) return;
  a = 0.0, b = 0.0;
  for (int i = 0; i < 256; ++i) a += sh[0][i], b += sh[1][i];
  fin[0] = a, fin[1] = b;
  if (loss) *loss = (float)(a / b);
}

// the gradient rows: kept pixels d l / d logits * grad_scale / denominator, every other pixel zeros (accumulate: left as they are);
// classes [C, zero_to) of every pixel are written 0 when the call does not accumulate
template <int NC, bool SELECT, bool MAP>
__global__ __launch_bounds__(256) void pc_grad_kernel(PcCall k, const unsigned* __restrict__ plane, const double* __restrict__ fin, float gs,
                                                      const float* __restrict__ gs_dev, float* __restrict__ dlogits, int64_t ds_n,
                                                      int64_t ds_c, int64_t ds_p, int accumulate, int zero_to) {
#pragma clang fp contract(off)   // with and without the select the rows come out bit for bit the same
  const LossTile t = loss_tile(k);
  const float up = (float)((double)gs * (gs_dev ? (double)*gs_dev : 1.0) / fin[1]);
  PcPixel<NC> x;
  pc_weights(k, x.w);
#pragma unroll 2
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const int j = i * 256 + threadIdx.x;
    if (j >= t.n) continue;
    const int q = t.first + j, b = q / k.HW;
    float* d = dlogits + b * ds_n + (int64_t)(q - b * k.HW) * ds_p;
    const long long y = k.labels[q];
    bool keep = y != k.ignore && y >= 0 && y < k.C;
    if (SELECT) keep = keep && !(plane[q] & PC_DROPPED);
    float row[NC] = {};
    if (keep) {
      pc_pixel<NC, MAP>(k, q, (int)y, x);
      pc_row(k, (int)y, x, row);
      if (MAP) {   // m is held fixed: the row of m * l
        const float m = k.pmap[q];
#pragma unroll
        for (int c = 0; c < NC; ++c) row[c] *= m;
      }
    }
    if (!accumulate) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < k.C) d[c * ds_c] = keep ? up * row[c] : 0.f;
      for (int c = k.C; c < zero_to; ++c) d[c * ds_c] = 0.f;
    } else if (keep) {
#pragma unroll
      for (int c = 0; c < NC; ++c)
        if (c < k.C) d[c * ds_c] += up * row[c];
    }
  }
}

}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

struct PcScratch {
  size_t part, fin, plane, hist, ties, state, bytes;
};
PcScratch pc_scratch(int64_t P, int G, int tiles_g, bool select) {
  Carve k;
  PcScratch s{};
  const size_t tiles = (size_t)G * tiles_g;
  s.part = k.take(tiles * 16);
  s.fin = k.take(16);
  if (select) {
    s.plane = k.take((size_t)P * 4);
    s.hist = k.take((size_t)PC_PASSES * G * 256 * 4);
    s.ties = k.take(tiles * 4);
    s.state = k.take((size_t)G * 8);
  }
  s.bytes = k.off;
  return s;
}

const char* const PC_HINT = "1 <= num_classes <= 8, a shape without pixels";

int pixel_ce_run(mgu_ctx* c, const char* fn, const void* logits, const int64_t* labels, int B, int64_t HW, int C, int64_t ls_n, int64_t ls_c,
                 int64_t ls_p, const float* weight, const float* pmap, bool map_entry, float eps, float gamma, double keep, int64_t min_kept,
                 int per_image, int64_t ignore_index, float* loss, float* pixel_loss, int32_t* kept, const LossGrad* grad, hipStream_t s) {
  // the profile's kernel families: the _map entries report under names of their own
  static const char* const NAMES[2][3] = {{"pixel_ce select", "pixel_ce sums", "pixel_ce gradient"},
                                          {"pixel_ce_map select", "pixel_ce_map sums", "pixel_ce_map gradient"}};
  const char* const* names = NAMES[map_entry ? 1 : 0];
  PcCall k;
  int* err_dev = nullptr;
  int rc = loss_call(c, fn, PC_HINT, logits, labels, B, HW, C, ls_n, ls_c, ls_p, per_image, ignore_index, &k, &err_dev);
  if (rc) return rc;
  if (!(eps >= 0.f && eps < 1.f)) return fail(c, MGU_ERR_INVALID, "%s: label_smoothing must lie in [0, 1)", fn);
  if (!(gamma == 0.f || gamma >= 1.f)) return fail(c, MGU_ERR_INVALID, "%s: focal_gamma must be 0 or >= 1", fn);
  if (gamma > 0.f && eps > 0.f) return fail(c, MGU_ERR_INVALID, "%s: focal_gamma > 0 takes no label_smoothing", fn);
  if (!(keep > 0.0 && keep <= 1.0)) return fail(c, MGU_ERR_INVALID, "%s: keep_fraction must lie in (0, 1]", fn);
  if (min_kept < 0) return fail(c, MGU_ERR_INVALID, "%s: min_kept must be >= 0", fn);
  const bool select = keep < 1.0;
  k.weight = weight, k.pmap = pmap, k.min_kept = min_kept, k.keep = keep, k.eps = eps, k.gamma = gamma;
  const PcScratch w = pc_scratch(k.P, k.G, k.tiles_g, select);
  if ((rc = ensure(c, &c->lossws, &c->lossws_bytes, w.bytes))) return rc;
  char* ws = (char*)c->lossws;
  double *part = (double*)(ws + w.part), *fin = (double*)(ws + w.fin);
  unsigned *plane = (unsigned*)(ws + w.plane), *state = (unsigned*)(ws + w.state);
  int *hist = (int*)(ws + w.hist), *ties = (int*)(ws + w.ties);
  const int tiles = k.G * k.tiles_g;
  const dim3 grid(tiles);
  if (select) HIPCHK(c, hipMemsetAsync(hist, 0, (size_t)PC_PASSES * k.G * 256 * 4, s));
  // MAP, then the padded class count and SELECT where a kernel has them, become template arguments; the selecting sums read the plane
  // and exist for <4> only.
  with_flag(pmap != nullptr, [&](auto map) {
    constexpr bool MAP = decltype(map)::value;
    if (select) {
      {
        ProfScope ps(c, s, names[0]);
        with_nc(C, [&](auto nc) {
          hipLaunchKernelGGL((pc_loss_kernel<decltype(nc)::value, MAP>), grid, dim3(256), 0, s, k, plane, hist, pixel_loss, err_dev);
        });
      }
      for (int pass = 1; pass < PC_PASSES; ++pass) {
        ProfScope ps(c, s, names[0]);
        hipLaunchKernelGGL(pc_count_kernel, grid, dim3(256), 0, s, k, plane, hist, pass);
      }
      {
        ProfScope ps(c, s, names[0]);
        hipLaunchKernelGGL(pc_tie_count_kernel, grid, dim3(256), 0, s, k, plane, hist, ties);
      }
      {
        ProfScope ps(c, s, names[0]);
        hipLaunchKernelGGL(pc_tie_scan_kernel, dim3(k.G), dim3(256), 0, s, k, hist, ties, state);
      }
      {
        ProfScope ps(c, s, names[1]);
        hipLaunchKernelGGL((pc_sum_kernel<4, true, MAP>), grid, dim3(256), 0, s, k, plane, ties, state, part, pixel_loss, kept, err_dev);
      }
    } else {
      ProfScope ps(c, s, names[1]);
      with_nc(C, [&](auto nc) {
        hipLaunchKernelGGL((pc_sum_kernel<decltype(nc)::value, false, MAP>), grid, dim3(256), 0, s, k, plane, ties, state, part, pixel_loss,
                           kept, err_dev);
      });
    }
    {
      ProfScope ps(c, s, names[1]);
      hipLaunchKernelGGL(pc_finish_kernel, dim3(1), dim3(256), 0, s, part, tiles, fin, loss);
    }
    if (grad) {
      ProfScope ps(c, s, names[2]);
      with_flag(select, [&](auto sel) {
        with_nc(C, [&](auto nc) {
          hipLaunchKernelGGL((pc_grad_kernel<decltype(nc)::value, decltype(sel)::value, MAP>), grid, dim3(256), 0, s, k, plane, fin,
                             grad->scale, grad->scale_dev, grad->dlogits, grad->ds_n, grad->ds_c, grad->ds_p, grad->accumulate, grad->zero_to);
        });
      });
    }
  });
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_pixel_ce_tile(void) { return LOSS_TILE; }

int mgu_pixel_ce(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n, int64_t ls_c,
                 int64_t ls_p, const float* class_weight_dev, float label_smoothing, float focal_gamma, double keep_fraction,
                 int64_t min_kept, int per_image, int64_t ignore_index, float* loss_dev, float* pixel_loss_dev, int32_t* kept_dev,
                 void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!loss_dev) return fail(c, MGU_ERR_INVALID, "bad pixel_ce args (loss_dev is NULL)");
  return pixel_ce_run(c, "pixel_ce", logits_dev, labels_dev, B, HW, num_classes, ls_n, ls_c, ls_p, class_weight_dev, nullptr, false,
                      label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, ignore_index, loss_dev, pixel_loss_dev, kept_dev, nullptr,
                      (hipStream_t)hip_stream);
}

int mgu_pixel_ce_backward(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                          int64_t ls_c, int64_t ls_p, const float* class_weight_dev, float label_smoothing, float focal_gamma,
                          double keep_fraction, int64_t min_kept, int per_image, int64_t ignore_index, float grad_scale,
                          const float* grad_scale_dev, void* dlogits_dev, int64_t ds_n, int64_t ds_c, int64_t ds_p, int accumulate,
                          int zero_to, float* loss_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!dlogits_dev) return fail(c, MGU_ERR_INVALID, "bad pixel_ce_backward args (dlogits_dev is NULL)");
  const LossGrad g{grad_scale, grad_scale_dev, (float*)dlogits_dev, ds_n, ds_c, ds_p, accumulate, zero_to};
  return pixel_ce_run(c, "pixel_ce_backward", logits_dev, labels_dev, B, HW, num_classes, ls_n, ls_c, ls_p, class_weight_dev, nullptr,
                      false, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, ignore_index, loss_dev, nullptr, nullptr, &g,
                      (hipStream_t)hip_stream);
}

// the same two entries with a per-pixel weight map m (fp32 (B, HW), dense, >= 0; nullptr: the entries above, bit for bit)
int mgu_pixel_ce_map(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                     int64_t ls_c, int64_t ls_p, const float* class_weight_dev, const float* pixel_weight_dev, float label_smoothing,
                     float focal_gamma, double keep_fraction, int64_t min_kept, int per_image, int64_t ignore_index, float* loss_dev,
                     float* pixel_loss_dev, int32_t* kept_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!loss_dev) return fail(c, MGU_ERR_INVALID, "bad pixel_ce_map args (loss_dev is NULL)");
  return pixel_ce_run(c, "pixel_ce_map", logits_dev, labels_dev, B, HW, num_classes, ls_n, ls_c, ls_p, class_weight_dev, pixel_weight_dev,
                      true, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, ignore_index, loss_dev, pixel_loss_dev,
                      kept_dev, nullptr, (hipStream_t)hip_stream);
}

int mgu_pixel_ce_map_backward(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                              int64_t ls_c, int64_t ls_p, const float* class_weight_dev, const float* pixel_weight_dev,
                              float label_smoothing, float focal_gamma, double keep_fraction, int64_t min_kept, int per_image,
                              int64_t ignore_index, float grad_scale, const float* grad_scale_dev, void* dlogits_dev, int64_t ds_n,
                              int64_t ds_c, int64_t ds_p, int accumulate, int zero_to, float* loss_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!dlogits_dev) return fail(c, MGU_ERR_INVALID, "bad pixel_ce_map_backward args (dlogits_dev is NULL)");
  const LossGrad g{grad_scale, grad_scale_dev, (float*)dlogits_dev, ds_n, ds_c, ds_p, accumulate, zero_to};
  return pixel_ce_run(c, "pixel_ce_map_backward", logits_dev, labels_dev, B, HW, num_classes, ls_n, ls_c, ls_p, class_weight_dev,
                      pixel_weight_dev, true, label_smoothing, focal_gamma, keep_fraction, min_kept, per_image, ignore_index, loss_dev,
                      nullptr, nullptr, &g, (hipStream_t)hip_stream);
}

}  // extern "C"
