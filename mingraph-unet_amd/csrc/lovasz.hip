// Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018: the Lovasz extension of the Jaccard loss), value and gradient on the device:
//   mgu_lovasz_softmax            loss value (+ the test hooks: per-class errors and ranks)
//   mgu_lovasz_softmax_backward   d loss / d logits through the softmax (+ the value of the same pass)
// The reference has no such loss; the definition is INTEGRATION.md section Q.  Per class every pixel's error e = |[y == c] - p_c| is
// ranked in descending order inside its segment (the class over the batch, or over one image), ties in pixel order; the gradient of
// the Jaccard loss along that order comes from exact integer counts in closed form (no differencing of neighbouring quotients, which
// cancels in fp32), the value is sum e * g in double in a fixed order.
//
// The sort is the cost.  Key = ~bits(e) & 0x3FFFFFFF (e in [0, 1]: 30 bits, ascending key = descending error), bit 30 set for an
// ignored pixel so that it lands behind the segment's ranked pixels; payload = pixel index with the foreground flag in bit 31 and the
// bad-label flag in bit 30.  A stable LSD radix sort over 31 bits: per pass a digit histogram per workgroup tile (LDS counters; a
// count does not depend on arrival order), an exclusive scan along the tiles of every (segment, digit) row, and a scatter whose position inside the
// tile comes from wave ballots per digit bit + mbcnt lane counts and a fixed (wave, item, lane) order -- no atomic decides a position,
// so the order is stable, which IS the tie rule, and the result is bitwise reproducible.  The first pass forms its keys from the
// logits; no error tensor exists outside the test hook.  Segments are a dimension of the grid (a tile never straddles two).
// Launches: 3 per sort pass, foreground count, its scan, the closed-form pass, the finishing kernel, and with the gradient the
// per-pixel softmax backward -- 16 / 17 with the four passes of 8 + 8 + 8 + 7 bits, whatever C, per_image and B are.  Three passes
// of 10 + 10 + 11 (MGU_LOVASZ_PASSES=3: 13 / 14 launches) move a quarter less but count into four to sixteen times the bins: value + gradient
// at 8 x 512 x 512, C = 2 take 486.7 us with four passes and 498.4 us with three (C = 4: 843.3 / 851.4 us; every row of
// profiles/lovasz_bench.txt goes the same way, spread 0.2 %), so four it is.
#include <algorithm>

#include "loss_common.h"
#include "objects_common.h"

namespace mgu {

// A workgroup ranks the LOSS_TILE keys of one tile (loss_common.h) per pass; segment (c, g) of a LossCall is plane c, positions
// [g * Ng, (g + 1) * Ng).
constexpr unsigned LV_KEY_MASK = 0x3FFFFFFFu, LV_KEY_IGNORED = 0x40000000u;
constexpr unsigned LV_PAY_FG = 0x80000000u, LV_PAY_BAD = 0x40000000u, LV_PAY_PIX = 0x3FFFFFFFu;

// Key and payload of pixel q for class c.  The softmax is the dice kernels' (softmax_front, one reciprocal); the error is ONE
// subtraction, so a saturated softmax gives exactly 0.0f or 1.0f.  Contraction is off: the histogram and the scatter of the first
// pass both come through here and must see the same bits.
__device__ __forceinline__ void lv_key(const LossCall& k, int q, int c, unsigned& key, unsigned& pay, float& err, bool& bad) {
#pragma clang fp contract(off)
  const long long y = k.labels[q];
  if (y == k.ignore) {
    key = LV_KEY_IGNORED, pay = (unsigned)q, err = 0.f;
    return;
  }
  const int b = q / k.HW;
  const float* p = k.logits + b * k.ls_n + (int64_t)(q - b * k.HW) * k.ls_p;
  float e[8], mx, lc = 0.f;
  const float se = softmax_front(p, k.ls_c, k.C, e, mx);
#pragma unroll
  for (int j = 0; j < 8; ++j)
    if (j == c) lc = e[j];   // a select per class: e stays in registers
  const float inv = 1.f / se, pc = lc * inv;
  const bool fg = y == c, wrong = y < 0 || y >= k.C;
  err = fminf(fmaxf(fg ? 1.f - pc : pc, 0.f), 1.f);   // the clamp moves nothing on finite logits: it keeps the key inside 30 bits
  key = ~__float_as_uint(err) & LV_KEY_MASK;
  pay = (unsigned)q | (fg ? LV_PAY_FG : 0u) | (wrong ? LV_PAY_BAD : 0u);
  bad |= wrong;
}

// ---- one sort pass: histogram, scan, scatter ------------------------------------------------------------------------------------
// hist[(seg * BINS + digit) * tiles_g + tile]: keys of the tile with that digit
template <int BITS, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void lv_hist_kernel(LossCall k, const unsigned* __restrict__ keys_in, int shift, int* __restrict__ hist,
                                                      int* __restrict__ err_word) {
  constexpr int BINS = 1 << BITS;
  __shared__ int cnt[BINS];
  for (int d = threadIdx.x; d < BINS; d += 256) cnt[d] = 0;
  __syncthreads();
  const LossTile t = loss_tile(k);
  bool bad = false;
#pragma unroll 4
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const int j = i * 256 + threadIdx.x;
    if (j < t.n) {
      unsigned key, pay;
      float err;
      if (FROM_LOGITS) lv_key(k, t.first + j, t.c, key, pay, err, bad);
      else key = keys_in[t.pfirst + j];
      atomicAdd(&cnt[(key >> shift) & (BINS - 1)], 1);
    }
  }
  if (FROM_LOGITS && bad && t.c == 0 && err_word) atomicOr(err_word, 1);
  __syncthreads();
  for (int d = threadIdx.x; d < BINS; d += 256) hist[((size_t)t.seg * BINS + d) * k.tiles_g + t.tile] = cnt[d];
}

// One wave per row: a[row][0 .. n) becomes its exclusive prefix sums and tot[row] its sum.  The rows of a pass are its (segment, digit)
// pairs, n the tiles of a segment: thousands of independent rows, where one scan per segment over (digit, tile) left the whole device
// waiting for as many workgroups as there are segments (3.6 ms instead of 0.5 ms at 8 x 512 x 512, C = 2 over the batch).  The
// scatter adds the digits' own prefix (lv_scatter_kernel).
__global__ __launch_bounds__(256) void lv_rowscan_kernel(int* __restrict__ a, int rows, int n, int* __restrict__ tot) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;   // a whole wave: no workgroup barrier below
  int* p = a + (size_t)row * n;
  int carry = 0;
  for (int base = 0; base < n; base += 64) {
    const int j = base + lane, v = j < n ? p[j] : 0;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(inc, off);
      if (lane >= off) inc += u;
    }
    if (j < n) p[j] = carry + inc - v;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) tot[row] = carry;
}

// offs: the histogram scanned along the tiles of every digit, dtot: the keys of the segment per digit, whose exclusive prefix (every
// workgroup forms it again: at most 8 entries per thread) is where a digit starts in the segment.  Order of the keys of a tile: wave,
// item, lane -- their order in the input.
template <int BITS, bool FROM_LOGITS>
__global__ __launch_bounds__(256) void lv_scatter_kernel(LossCall k, const unsigned* __restrict__ keys_in, const unsigned* __restrict__ pay_in,
                                                         int shift, const int* __restrict__ offs, const int* __restrict__ dtot,
                                                         unsigned* __restrict__ keys_out, unsigned* __restrict__ pay_out,
                                                         float* __restrict__ errors) {
  constexpr int BINS = 1 << BITS, PER = BINS >= 256 ? BINS / 256 : 1;
  __shared__ int cnt[4 * BINS];
  __shared__ int dbase[BINS];
  __shared__ int shs[4];
  const LossTile t = loss_tile(k);
  {
    int mine_tot[PER], sum = 0;
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int d = threadIdx.x * PER + r;
      mine_tot[r] = d < BINS ? dtot[(size_t)t.seg * BINS + d] : 0;
      sum += mine_tot[r];
    }
    int total;
    int at = block_exclusive_scan(sum, shs, &total) + t.g * k.Ng;   // the segment's first position in the class plane
#pragma unroll
    for (int r = 0; r < PER; ++r) {
      const int d = threadIdx.x * PER + r;
      if (d < BINS) dbase[d] = at;
      at += mine_tot[r];
    }
  }
  for (int d = threadIdx.x; d < 4 * BINS; d += 256) cnt[d] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int* mine = cnt + wave * BINS;
  unsigned key[LOSS_ITEMS], pay[LOSS_ITEMS];
  int rank[LOSS_ITEMS];
  bool bad = false;
#pragma unroll
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const int j = loss_item(i);
    const bool valid = j < t.n;
    key[i] = 0, pay[i] = 0;
    if (valid) {
      if (FROM_LOGITS) {
        const int q = t.first + j;
        float err;
        lv_key(k, q, t.c, key[i], pay[i], err, bad);
        if (errors) errors[(size_t)t.c * k.P + q] = err;
      } else {
        key[i] = keys_in[t.pfirst + j], pay[i] = pay_in[t.pfirst + j];
      }
    }
    const unsigned d = (key[i] >> shift) & (BINS - 1);
    // the lanes of this item that hold the same digit: one ballot per digit bit
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < BITS; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long s = __ballot(bit);
      m &= bit ? s : ~s;
    }
    const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    int old = 0;
    if (valid && below == 0) {   // the first of them takes the digit's next positions of this wave for all of them
      old = mine[d];
      mine[d] = old + __popcll(m);
    }
    old = __shfl(old, valid ? __ffsll((long long)m) - 1 : lane);
    rank[i] = old + below;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // per digit: where the digit starts, the keys of the tiles before this one, then the waves in order
  for (int d = threadIdx.x; d < BINS; d += 256) {
    int o = dbase[d] + offs[((size_t)t.seg * BINS + d) * k.tiles_g + t.tile];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int v = cnt[w * BINS + d];
      cnt[w * BINS + d] = o;
      o += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const int j = loss_item(i);
    if (j < t.n) {
      const int pos = mine[(key[i] >> shift) & (BINS - 1)] + rank[i];
      if ((unsigned)pos < (unsigned)k.P) {   // always, for a histogram of these very keys
        keys_out[(size_t)t.c * k.P + pos] = key[i];
        pay_out[(size_t)t.c * k.P + pos] = pay[i];
      }
    }
  }
}

// ---- over the sorted order ------------------------------------------------------------------------------------------------------
// foreground pixels per tile
__global__ __launch_bounds__(256) void lv_count_kernel(LossCall k, const unsigned* __restrict__ pay, int* __restrict__ fgc) {
  __shared__ int sh[4];
  const LossTile t = loss_tile(k);
  int s = 0;
#pragma unroll 4
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const int j = i * 256 + threadIdx.x;
    if (j < t.n) s += pay[t.pfirst + j] >> 31;
  }
  int total;
  block_exclusive_scan(s, sh, &total);
  if (threadIdx.x == 0) fgc[(size_t)t.seg * k.tiles_g + t.tile] = total;
}

// The Jaccard gradient at every rank from the exact counts: G = foreground pixels of the segment, k = rank (from 1), F = foreground
// pixels among ranks 1 .. k, U = G + k - F (the union), I = G - F (what is left of the intersection):
//   foreground pixel 1 / U;  background pixel I / (U (U - 1));  G == 0: 1 at rank 1, else 0
// in double, rounded once into gbuf[c][pixel]; an ignored pixel gets 0 and rank -1.  part[seg][tile] = sum e * g over the tile.
__global__ __launch_bounds__(256) void lv_apply_kernel(LossCall k, const unsigned* __restrict__ keys, const unsigned* __restrict__ pay,
                                                       const int* __restrict__ fgoff, const int* __restrict__ seg_fg,
                                                       float* __restrict__ gbuf, int* __restrict__ ranks, double* __restrict__ part) {
  __shared__ int shs[4];
  __shared__ double shd[4];
  const LossTile t = loss_tile(k);
  const int j0 = threadIdx.x * LOSS_ITEMS;   // a thread owns consecutive ranks
  unsigned key[LOSS_ITEMS], py[LOSS_ITEMS];
  int s = 0;
#pragma unroll
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    const bool valid = j0 + i < t.n;
    key[i] = valid ? keys[t.pfirst + j0 + i] : LV_KEY_IGNORED;
    py[i] = valid ? pay[t.pfirst + j0 + i] : 0u;
    s += py[i] >> 31;
  }
  int total;
  int F = block_exclusive_scan(s, shs, &total) + fgoff[(size_t)t.seg * k.tiles_g + t.tile];
  const int G = seg_fg[t.seg];
  double acc[1] = {0.0};
#pragma unroll
  for (int i = 0; i < LOSS_ITEMS; ++i) {
    if (j0 + i >= t.n) continue;
    const unsigned pix = py[i] & LV_PAY_PIX;
    if (pix >= (unsigned)k.P) continue;   // never: payloads are pixel indices
    const size_t at = (size_t)t.c * k.P + pix;
    if (key[i] & LV_KEY_IGNORED) {
      gbuf[at] = 0.f;
      if (ranks) ranks[at] = -1;
      continue;
    }
    const int fg = py[i] >> 31, rk = t.lo + j0 + i + 1;
    F += fg;
    double g;
    if (G == 0) {
      g = rk == 1 ? 1.0 : 0.0;
    } else {
      const double U = (double)(G + rk - F);
      g = fg ? 1.0 / U : (double)(G - F) / (U * (U - 1.0));
    }
    acc[0] += (double)__uint_as_float(~key[i] & LV_KEY_MASK) * g;
    if (py[i] & LV_PAY_BAD) acc[0] += (double)NAN;   // a label outside [0, C): the loss comes out NaN
    gbuf[at] = (float)g;
    if (ranks) ranks[at] = rk - 1;
  }
  block_fold<1>(acc, shd);
  if (threadIdx.x == 0) part[(size_t)t.seg * k.tiles_g + t.tile] = acc[0];
}

// Segment losses (tiles in order), the mean over the counted segments of a group and over the groups, and the factor of every
// segment's gradient: wtab[seg] = 1 / (counted segments of its group * groups), 0 for a segment that is not counted.
__global__ __launch_bounds__(64) void lv_finish_kernel(const double* __restrict__ part, const int* __restrict__ seg_fg, int C, int G,
                                                       int tiles_g, int classes_all, double* __restrict__ seg_loss,
                                                       float* __restrict__ wtab, float* __restrict__ loss) {
  for (int seg = threadIdx.x; seg < C * G; seg += 64) {
    double s = 0.0;
    for (int j = 0; j < tiles_g; ++j) s += part[(size_t)seg * tiles_g + j];
    seg_loss[seg] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int seg = 0; seg < C * G; ++seg) total += seg_loss[seg] * 0.0;   // NaN (a bad label) reaches the loss from any segment
  for (int g = 0; g < G; ++g) {
    int counted = 0;
    double sum = 0.0;
    for (int c = 0; c < C; ++c)
      if (classes_all || seg_fg[c * G + g] > 0) ++counted, sum += seg_loss[c * G + g];
    if (counted) total += sum / counted;
    for (int c = 0; c < C; ++c)
      wtab[c * G + g] = (classes_all || seg_fg[c * G + g] > 0) ? (float)(1.0 / ((double)counted * G)) : 0.f;
  }
  if (loss) *loss = (float)(total / G);
}

// dL/dp_c = d_c = -+ g * wtab (foreground -, background +), then the softmax backward dlogit_j = p_j (d_j - sum_c p_c d_c), formed as
// p_j sum_{c != j} p_c (d_j - d_c): the segment's first rank carries a g of order 1 on a pixel whose p_j is close to 1 (a class the
// image lacks, under "all"), and d_j (1 - p_j) as a difference loses ulp(1) / (1 - p_j) there -- 6e-6 of the LARGEST gradient element
// at p_j = 0.99, which is what torch's own fp32 softmax backward loses.  C terms more per class; the pass stays bound by its loads.
template <int NC>
__global__ __launch_bounds__(256) void lv_bwd_kernel(LossCall k, const float* __restrict__ gbuf, const float* __restrict__ wtab, float gs,
                                                     const float* __restrict__ gs_dev, float* __restrict__ dlogits, int64_t ds_n,
                                                     int64_t ds_c, int64_t ds_p, int accumulate) {
  const int b = blockIdx.y, grp = k.G > 1 ? b : 0;
  const float up = up_scale(gs, gs_dev);
  float w[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) w[c] = c < k.C ? wtab[c * k.G + grp] : 0.f;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < k.HW; i += gridDim.x * 256) {
    const int q = b * k.HW + i;
    const long long y = k.labels[q];
    float* d = dlogits + b * ds_n + i * ds_p;
    if (y == k.ignore) {
      if (!accumulate)
#pragma unroll
        for (int c = 0; c < NC; ++c)
          if (c < k.C) d[c * ds_c] = 0.f;
      continue;
    }
    const float* p = k.logits + b * k.ls_n + i * k.ls_p;
    float l[NC], mx;
    const float inv = 1.f / softmax_front(p, k.ls_c, k.C, l, mx);
    float dp[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      l[c] *= inv;
      const float g = c < k.C ? gbuf[(size_t)c * k.P + q] * w[c] : 0.f;
      dp[c] = y == c ? -g : g;
    }
#pragma unroll
    for (int j = 0; j < NC; ++j)
      if (j < k.C) {
        float rest = 0.f;   // d_j - sum_c p_c d_c with sum_c p_c = 1; a padded class has p = 0
#pragma unroll
        for (int c = 0; c < NC; ++c) rest += l[c] * (dp[j] - dp[c]);
        const float v = up * l[j] * rest;
        d[j * ds_c] = accumulate ? d[j * ds_c] + v : v;
      }
  }
}

}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

// digit widths of the LSD passes over the 31 key bits (the choice: the head of this file)
struct LvSplit {
  int passes;
  int bits[4];
};
const LvSplit LV_SPLIT3 = {3, {10, 10, 11, 0}}, LV_SPLIT4 = {4, {8, 8, 8, 7}};

struct LvScratch {
  size_t keys[2], pay[2], hist, dtot, fgc, seg_fg, part, seg_loss, wtab, bytes;
};
// scratch of a call: two key and two payload planes per class (the free key plane holds g after the sort), the (digit, tile) table
// and the digit totals of one pass (max_bits: its widest digit), and per-tile / per-segment records
LvScratch lv_scratch(int64_t P, int C, int G, int tiles_g, int max_bits) {
  Carve k;
  LvScratch s;
  const size_t plane = (size_t)C * P * 4, segs = (size_t)C * G, tiles = segs * tiles_g;
  for (int i = 0; i < 2; ++i) s.keys[i] = k.take(plane), s.pay[i] = k.take(plane);
  s.hist = k.take(tiles * ((size_t)4 << max_bits));
  s.dtot = k.take(segs * ((size_t)4 << max_bits));
  s.fgc = k.take(tiles * 4);
  s.seg_fg = k.take(segs * 4);
  s.part = k.take(tiles * 8);
  s.seg_loss = k.take(segs * 8);
  s.wtab = k.take(segs * 4);
  s.bytes = k.off;
  return s;
}

template <bool FROM_LOGITS>
void lv_pass(int bits, const LossCall& k, dim3 grid, hipStream_t s, const unsigned* kin, const unsigned* pin, int shift, int* hist, int* dtot,
             int* err_dev, unsigned* kout, unsigned* pout, float* errors) {
  const auto pass = [&](auto width) {
    constexpr int BITS = decltype(width)::value;
    hipLaunchKernelGGL((lv_hist_kernel<BITS, FROM_LOGITS>), grid, dim3(256), 0, s, k, kin, shift, hist, err_dev);
    hipLaunchKernelGGL(lv_rowscan_kernel, dim3((k.C * k.G << BITS) / 4), dim3(256), 0, s, hist, k.C * k.G << BITS, k.tiles_g, dtot);
    hipLaunchKernelGGL((lv_scatter_kernel<BITS, FROM_LOGITS>), grid, dim3(256), 0, s, k, kin, pin, shift, hist, dtot, kout, pout, errors);
  };
  if (bits == 7) pass(int_c<7>{});
  else if (bits == 8) pass(int_c<8>{});
  else if (bits == 10) pass(int_c<10>{});
  else pass(int_c<11>{});
}

const char* const LV_HINT = "1 <= num_classes <= 8, classes_mode 0 = present / 1 = all";

int lovasz_run(mgu_ctx* c, const char* fn, const void* logits, const int64_t* labels, int B, int64_t HW, int C, int64_t ls_n, int64_t ls_c,
               int64_t ls_p, int classes_mode, int per_image, int64_t ignore_index, float* loss, float* errors, int32_t* ranks,
               const LossGrad* grad, hipStream_t s) {
  if (classes_mode < 0 || classes_mode > 1) return fail(c, MGU_ERR_INVALID, "bad %s args (%s)", fn, LV_HINT);
  LossCall k;
  int* err_dev = nullptr;
  int rc = loss_call(c, fn, LV_HINT, logits, labels, B, HW, C, ls_n, ls_c, ls_p, per_image, ignore_index, &k, &err_dev);
  if (rc) return rc;
  const LvSplit& split = c->tn.lovasz_passes == 3 ? LV_SPLIT3 : LV_SPLIT4;
  const LvScratch w = lv_scratch(k.P, C, k.G, k.tiles_g, *std::max_element(split.bits, split.bits + split.passes));
  if ((rc = ensure(c, &c->lossws, &c->lossws_bytes, w.bytes))) return rc;
  char* ws = (char*)c->lossws;
  unsigned *keys[2] = {(unsigned*)(ws + w.keys[0]), (unsigned*)(ws + w.keys[1])}, *pay[2] = {(unsigned*)(ws + w.pay[0]), (unsigned*)(ws + w.pay[1])};
  int *hist = (int*)(ws + w.hist), *dtot = (int*)(ws + w.dtot), *fgc = (int*)(ws + w.fgc), *seg_fg = (int*)(ws + w.seg_fg);
  double *part = (double*)(ws + w.part), *seg_loss = (double*)(ws + w.seg_loss);
  float* wtab = (float*)(ws + w.wtab);
  const dim3 grid(k.G * k.tiles_g, C);
  int cur = 1, shift = 0;   // the pass writes buffer 1 - cur
  {
    ProfScope ps(c, s, "lovasz sort");
    for (int p = 0; p < split.passes; ++p) {
      if (p == 0) lv_pass<true>(split.bits[p], k, grid, s, nullptr, nullptr, shift, hist, dtot, err_dev, keys[1 - cur], pay[1 - cur], errors);
      else lv_pass<false>(split.bits[p], k, grid, s, keys[cur], pay[cur], shift, hist, dtot, err_dev, keys[1 - cur], pay[1 - cur], nullptr);
      cur = 1 - cur, shift += split.bits[p];
    }
  }
  float* gbuf = (float*)keys[1 - cur];
  {
    ProfScope ps(c, s, "lovasz scan");
    hipLaunchKernelGGL(lv_count_kernel, grid, dim3(256), 0, s, k, pay[cur], fgc);
    hipLaunchKernelGGL(lv_rowscan_kernel, dim3((C * k.G + 3) / 4), dim3(256), 0, s, fgc, C * k.G, k.tiles_g, seg_fg);
    hipLaunchKernelGGL(lv_apply_kernel, grid, dim3(256), 0, s, k, keys[cur], pay[cur], fgc, seg_fg, gbuf, ranks, part);
    hipLaunchKernelGGL(lv_finish_kernel, dim3(1), dim3(64), 0, s, part, seg_fg, C, k.G, k.tiles_g, classes_mode, seg_loss, wtab, loss);
  }
  if (grad) {
    ProfScope ps(c, s, "lovasz final");
    const dim3 pg(std::min(128, grid_for(HW, 1024, 1024)), B);
    with_nc(C, [&](auto nc) {
      hipLaunchKernelGGL(lv_bwd_kernel<decltype(nc)::value>, pg, dim3(256), 0, s, k, gbuf, wtab, grad->scale, grad->scale_dev, grad->dlogits,
                         grad->ds_n, grad->ds_c, grad->ds_p, grad->accumulate);
    });
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_lovasz_tile(void) { return LOSS_TILE; }

int mgu_lovasz_softmax(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                       int64_t ls_c, int64_t ls_p, int classes_mode, int per_image, int64_t ignore_index, float* loss_dev,
                       float* errors_dev, int32_t* ranks_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!loss_dev) return fail(c, MGU_ERR_INVALID, "bad lovasz_softmax args (loss_dev is NULL)");
  return lovasz_run(c, "lovasz_softmax", logits_dev, labels_dev, B, HW, num_classes, ls_n, ls_c, ls_p, classes_mode, per_image, ignore_index,
                    loss_dev, errors_dev, ranks_dev, nullptr, (hipStream_t)hip_stream);
}

int mgu_lovasz_softmax_backward(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                                int64_t ls_n, int64_t ls_c, int64_t ls_p, int classes_mode, int per_image, int64_t ignore_index,
                                float grad_scale, const float* grad_scale_dev, void* dlogits_dev, int64_t ds_n, int64_t ds_c, int64_t ds_p,
                                int accumulate, float* loss_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!dlogits_dev) return fail(c, MGU_ERR_INVALID, "bad lovasz_softmax_backward args (dlogits_dev is NULL)");
  const LossGrad g{grad_scale, grad_scale_dev, (float*)dlogits_dev, ds_n, ds_c, ds_p, accumulate, 0};
  return lovasz_run(c, "lovasz_softmax_backward", logits_dev, labels_dev, B, HW, num_classes, ls_n, ls_c, ls_p, classes_mode, per_image,
                    ignore_index, loss_dev, nullptr, nullptr, &g, (hipStream_t)hip_stream);
}

}  // extern "C"
