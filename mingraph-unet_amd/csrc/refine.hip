// Edge-aware refinement of class probabilities on the device: every class plane is filtered with a joint bilateral kernel guided by
// the photograph, `iterations` times, then argmax (cost-volume filtering, Hosni et al., PAMI 2013; structurally the message passing
// step of a dense CRF).
//   mgu_refine_probs   NHWC fp32 probabilities (or logits) + uint8 guide -> refined probabilities, first maximal class, its value and
//                      the number of pixels per image whose class moved
// The reference has no such stage.  The arithmetic is THIS BUILD'S DEFINITION (include/mgunet.h spells it out): probabilities
// quantised to 16 bits once, integer weights w = (space[|dy|][|dx|] * range[min(d2 >> shift, 1023)] + 128) >> 8 <= 256 from two host
// tables, d2 the squared guide distance, uint32 sums (225 taps * 256 * 65535 < 2^32), one rounded integer division per pixel, class and
// iteration.  Taps outside the image are skipped.  No floating point after the quantisation: bitwise equal to tests/refine_oracle.py
// and from run to run.
//
// One launch per iteration, one workgroup per tile of one image (32 x 64 pixels up to 4 classes, 16 x 32 beyond).  The tile with its
// halo of `radius` pixels is staged in LDS: a 32-bit word per pixel for the guide (bytes 0..2 the channels, byte 3 = 1 marks a pixel
// outside the image), the range table with a second, all-zero half behind it, and one plane of 32-bit words per PAIR of classes.  The
// first launch quantises (softmax first, for logits) while it stages -- a halo pixel is formed by the expression its owner uses -- later
// launches read the previous launch's 16-bit NHWC planes from the context's scratch, the last one writes the outputs.
//   pairs   a thread filters two vertically adjacent pixels: they share every guide word and plane word they read, and a wave's LDS
//           accesses are runs of consecutive words
//   d2      |p|^2 + |q|^2 - 2 p.q with v_dot4_u32_u8 (|q|^2 once per pair, p.q once per pixel) instead of three subtract-multiply pairs
//   border  a tile that touches the border adds (byte 3) << 10 to the table index: an outside pixel lands in the zero half, weight 0,
//           so it leaves numerator and denominator alone; interior tiles run without those two instructions
//   taps    rows by a loop, the 15 columns of a row unrolled under a uniform |dx| <= radius test: the row's space weights sit in scalar
//           registers at compile-time indices
// Both tables travel in the kernel arguments.  Products are __umul24 (both factors fit 24 bits, see gaussian.hip).
#include <limits.h>

#include "ctx.h"

namespace mgu {
namespace {

constexpr int RF_THREADS = 256;
constexpr int RF_MAX_R = 7;          // 225 taps * 256 * 65535 < 2^32: the uint32 numerator is exact up to here and no further
constexpr int RF_MAX_C = 16;
constexpr int RF_MAX_T = 16;
constexpr int RF_MAX_SHIFT = 18;     // 3 * 255^2 < 2^18
constexpr int RF_RANGE = 1024;       // range table entries
constexpr int RF_SP = RF_MAX_R + 1;  // row pitch of the space table in the kernel arguments

// NC > 0: C == NC (1..4); NC == 0: C <= RF_MAX_C at run time
__host__ __device__ constexpr int rf_tile_h(int NC) { return NC > 0 ? 32 : 16; }
__host__ __device__ constexpr int rf_tile_w(int NC) { return NC > 0 ? 64 : 32; }
// LDS, all 32-bit words (16-bit planes and a 16-bit table, read with ds_read_u16, measured 4 % slower at C = 2 and 20 % at C = 4): the
// guide words of the (TH + 2r) x (TW + 2r) window, the doubled range table, and one plane of the window per class PAIR, class 2j in the
// low half, 2j + 1 in the high half
__host__ __device__ constexpr int rf_window(int NC, int r) { return (rf_tile_h(NC) + 2 * r) * (rf_tile_w(NC) + 2 * r); }
__host__ __device__ constexpr int rf_lds_bytes(int NC, int C, int r) { return rf_window(NC, r) * 4 * (1 + (C + 1) / 2) + 2 * RF_RANGE * 4; }
static_assert(rf_lds_bytes(4, 4, RF_MAX_R) <= 65536 && rf_lds_bytes(0, RF_MAX_C, RF_MAX_R) <= 65536,
              "a tile with a halo of 7 must fit the 64 KiB of LDS a workgroup can have");
static_assert(rf_tile_h(1) % 2 == 0 && rf_tile_h(0) % 2 == 0, "a thread owns vertical pixel pairs");

struct RefineTables {
  int space[RF_SP * RF_SP];          // [|dy|][|dx|], rows of RF_SP, 0 past the radius
  uint16_t range[RF_RANGE];
};
struct RefineOut {
  float* probs;
  long long* labels;
  float* conf;
  unsigned long long* changed;
};

// q0 of one value: rint(clamp(x, 0, 1) * 65535), NaN -> 0
__device__ __forceinline__ unsigned rf_quantise(float x) {
  x = x > 0.f ? x : 0.f;             // false for NaN
  x = x < 1.f ? x : 1.f;
  return (unsigned)__float2int_rn(x * 65535.f);
}
// q0 of the C classes of the pixel at p (probabilities, or logits through the softmax mgu_tta_merge takes)
template <int CM>
__device__ __forceinline__ void rf_quantise_pixel(const float* p, int is_prob, int C, unsigned (&q)[CM]) {
  float e[CM];
  if (is_prob) {
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) e[c] = p[c];
  } else {
    const float sum = pixel_softmax<CM>(p, C, e);
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) e[c] = e[c] / sum;
  }
#pragma unroll
  for (int c = 0; c < CM; ++c) q[c] = c < C ? rf_quantise(e[c]) : 0u;
}
template <int CM>
__device__ __forceinline__ int rf_first_max(const unsigned (&q)[CM], int C) {
  unsigned best = q[0];
  int bi = 0;
#pragma unroll
  for (int c = 1; c < CM; ++c)
    if (c < C && q[c] > best) best = q[c], bi = c;
  return bi;
}

// what the threads of a workgroup share while they filter: the staged window and the call's parameters
struct RefineWindow {
  const unsigned* Gd;    // guide words
  const unsigned* L;     // range table, then RF_RANGE zeros
  const unsigned* Q;     // (C + 1) / 2 planes of `win` words: classes 2j | 2j + 1 in the low | high half
  int win, P, r, shift, C;
};

// One window row of a pixel pair: the pixels A = (x, y) and B = (x, y + 1) share every guide word and plane value of the row, which is
// row dy of A (weights spa) and row dy - 1 of B (weights spb).  UA / UB: the row lies within the radius of A / B.
template <int CM, bool EDGE, bool UA, bool UB>
__device__ __forceinline__ void rf_row(const RefineWindow& w, int row, const int (&spa)[RF_SP], const int (&spb)[RF_SP], unsigned gpa, unsigned n2a,
                                       unsigned gpb, unsigned n2b, unsigned (&acca)[CM], unsigned& dena, unsigned (&accb)[CM], unsigned& denb) {
#pragma unroll
  for (int k = 0; k < 2 * RF_MAX_R + 1; ++k) {
    const int dx = k - RF_MAX_R, adx = dx < 0 ? -dx : dx;
    if (adx <= w.r) {                                        // uniform: a scalar branch, and spa[adx] is a scalar register
      const unsigned gq = w.Gd[row + dx], n2q = __builtin_amdgcn_udot4(gq, gq, 0u, false);
      unsigned flag = 0, qv[CM + 1];
      if constexpr (EDGE) flag = (gq >> 24) << 10;           // outside the image: the zero half (d2 is then off by the flag's square: unused)
#pragma unroll
      for (int j = 0; j < (CM + 1) / 2; ++j)
        if (2 * j < w.C) {
          const unsigned u = w.Q[j * w.win + row + dx];
          qv[2 * j] = u & 0xffffu, qv[2 * j + 1] = u >> 16;
        }
      if constexpr (UA) {
        const unsigned d2 = n2a + n2q - 2u * __builtin_amdgcn_udot4(gpa, gq, 0u, false);
        const unsigned wt = (__umul24((unsigned)spa[adx], w.L[min(d2 >> w.shift, (unsigned)(RF_RANGE - 1)) + flag]) + 128u) >> 8;
        dena += wt;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < w.C) acca[c] += __umul24(wt, qv[c]);
      }
      if constexpr (UB) {
        const unsigned d2 = n2b + n2q - 2u * __builtin_amdgcn_udot4(gpb, gq, 0u, false);
        const unsigned wt = (__umul24((unsigned)spb[adx], w.L[min(d2 >> w.shift, (unsigned)(RF_RANGE - 1)) + flag]) + 128u) >> 8;
        denb += wt;
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < w.C) accb[c] += __umul24(wt, qv[c]);
      }
    }
  }
}

// q' = (num + (den >> 1)) / den of one pixel, to the next plane set (qout) or, in the last iteration, to the outputs; returns 1 when
// the pixel's class moved and that is counted
template <int NC>
__device__ __forceinline__ unsigned rf_finish(const RefineWindow& w, const unsigned (&acc)[NC > 0 ? NC : RF_MAX_C], unsigned den, int64_t pix, int centre,
                                              const float* src, int is_prob, int first, uint16_t* __restrict__ qout, const RefineOut& o) {
  constexpr int CM = NC > 0 ? NC : RF_MAX_C;
  const int C = w.C;
  unsigned q[CM];
  const unsigned half = den >> 1;                            // den >= the centre's weight >= 1
#pragma unroll
  for (int c = 0; c < CM; ++c) q[c] = c < C ? (acc[c] + half) / den : 0u;
  if (qout) {
    if constexpr (NC == 2) {
      reinterpret_cast<unsigned*>(qout)[pix] = q[0] | q[1] << 16;
    } else if constexpr (NC == 4) {
      reinterpret_cast<uint2*>(qout)[pix] = make_uint2(q[0] | q[1] << 16, q[2] | q[3] << 16);
    } else {
#pragma unroll
      for (int c = 0; c < CM; ++c)
        if (c < C) qout[pix * C + c] = (uint16_t)q[c];
    }
    return 0;
  }
  const int bi = rf_first_max<CM>(q, C);
  o.labels[pix] = bi;
  if (o.probs) {
#pragma unroll
    for (int c = 0; c < CM; ++c)
      if (c < C) o.probs[pix * C + c] = (float)q[c] / 65535.0f;
  }
  if (o.conf) {
    unsigned qb = q[0];
#pragma unroll
    for (int c = 1; c < CM; ++c) qb = c == bi ? q[c] : qb;
    o.conf[pix] = (float)qb / 65535.0f;
  }
  if (!o.changed) return 0;
  unsigned q0[CM];
  if (first) {
#pragma unroll
    for (int c = 0; c < CM; ++c) q0[c] = c < C ? (w.Q[(c >> 1) * w.win + centre] >> (16 * (c & 1))) & 0xffffu : 0u;
  } else {
    rf_quantise_pixel<CM>(src + pix * C, is_prob, C, q0);
  }
  return rf_first_max<CM>(q0, C) != bi;
}

// the filter at the tile's pixels, from the staged window; returns the thread's count of pixels whose class moved.  A thread owns
// vertical pixel pairs, a wave 64 neighbouring columns of two rows: every LDS access of a wave is a run of consecutive addresses.
// A pair whose lower pixel lies below an odd tile height computes that pixel from the staged row under the tile and drops it.
template <int NC, bool EDGE>
__device__ __forceinline__ unsigned rf_filter(const RefineWindow& w, const RefineTables& tb, int th, int tw, int64_t pix0, int W, const float* src,
                                              int is_prob, int first, uint16_t* __restrict__ qout, const RefineOut& o) {
  constexpr int TH = rf_tile_h(NC), TW = rf_tile_w(NC), CM = NC > 0 ? NC : RF_MAX_C;
  const int r = w.r, P = w.P;
  unsigned moved = 0;
  for (int i = threadIdx.x; i < TH / 2 * TW; i += RF_THREADS) {
    const int ly = i / TW * 2, lx = i % TW;
    if (ly >= th || lx >= tw) continue;
    const int ca = (ly + r) * P + lx + r, cb = ca + P;
    const unsigned gpa = w.Gd[ca], gpb = w.Gd[cb];
    const unsigned n2a = __builtin_amdgcn_udot4(gpa, gpa, 0u, false), n2b = __builtin_amdgcn_udot4(gpb, gpb, 0u, false);
    unsigned acca[CM], accb[CM], dena = 0, denb = 0;
#pragma unroll
    for (int c = 0; c < CM; ++c) acca[c] = accb[c] = 0;
    int spa[RF_SP], spb[RF_SP];
#pragma unroll
    for (int k = 0; k < RF_SP; ++k) spa[k] = spb[k] = tb.space[r * RF_SP + k];
    rf_row<CM, EDGE, true, false>(w, ca - r * P, spa, spb, gpa, n2a, gpb, n2b, acca, dena, accb, denb);          // row -r of A
    for (int dy = 1 - r; dy <= r; ++dy) {                                                                        // row dy of A, dy - 1 of B
#pragma unroll
      for (int k = 0; k < RF_SP; ++k) spa[k] = tb.space[(dy < 0 ? -dy : dy) * RF_SP + k], spb[k] = tb.space[(dy < 1 ? 1 - dy : dy - 1) * RF_SP + k];
      rf_row<CM, EDGE, true, true>(w, ca + dy * P, spa, spb, gpa, n2a, gpb, n2b, acca, dena, accb, denb);
    }
#pragma unroll
    for (int k = 0; k < RF_SP; ++k) spb[k] = tb.space[r * RF_SP + k];
    rf_row<CM, EDGE, false, true>(w, ca + (r + 1) * P, spa, spb, gpa, n2a, gpb, n2b, acca, dena, accb, denb);    // row r of B
    const int64_t pix = pix0 + (int64_t)ly * W + lx;
    moved += rf_finish<NC>(w, acca, dena, pix, ca, src, is_prob, first, qout, o);
    if (ly + 1 < th) moved += rf_finish<NC>(w, accb, denb, pix + W, cb, src, is_prob, first, qout, o);
  }
  return moved;
}

// One iteration on one tile.  first: the planes come from src (quantised here), else from qin (NHWC uint16).  qout != NULL: the
// filtered planes go there; NULL (the last iteration): the outputs of o are written, and src is read again at the tile's own pixels
// when the class before the first iteration is wanted and is not in LDS.
template <int NC>
__global__ __launch_bounds__(RF_THREADS) void refine_kernel(const float* __restrict__ src, int is_prob, int first, const uint16_t* __restrict__ qin,
                                                            const uint8_t* __restrict__ guide, int H, int W, int Crt, int G, int r, int shift,
                                                            int tiles_x, const RefineTables tb, uint16_t* __restrict__ qout, const RefineOut o) {
  constexpr int TH = rf_tile_h(NC), TW = rf_tile_w(NC), CM = NC > 0 ? NC : RF_MAX_C;
  extern __shared__ __attribute__((aligned(16))) uint8_t rf_lds[];
  const int C = NC > 0 ? NC : Crt;
  const int b = blockIdx.y, ty = blockIdx.x / tiles_x, y0 = ty * TH, x0 = (blockIdx.x - ty * tiles_x) * TW;
  const int th = min(TH, H - y0), tw = min(TW, W - x0);
  const int P = TW + 2 * r, win = (TH + 2 * r) * P;
  unsigned* Gd = reinterpret_cast<unsigned*>(rf_lds);
  unsigned* L = Gd + win;
  unsigned* Q = L + 2 * RF_RANGE;
  for (int i = threadIdx.x; i < RF_RANGE; i += RF_THREADS) L[i] = tb.range[i], L[RF_RANGE + i] = 0u;
  const int64_t img = (int64_t)b * H * W;
  // an odd tile height is rounded up: the row under the tile is then outside the image, and the lower pixel of the last pair reads it
  const int rows = th + (th & 1) + 2 * r, cols = tw + 2 * r;
  const float rcols = 1.0f / (float)cols;                    // i / cols below: i < 2^12, so (i + 0.5) / cols is at least 2^-8 away from an integer
#pragma unroll 4
  for (int i = threadIdx.x; i < rows * cols; i += RF_THREADS) {
    const int ry = (int)(((float)i + 0.5f) * rcols), rx = i - ry * cols, gy = y0 - r + ry, gx = x0 - r + rx;
    unsigned g = 1u << 24, q[CM];
#pragma unroll
    for (int c = 0; c < CM; ++c) q[c] = 0;
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
      const int64_t pix = img + (int64_t)gy * W + gx;
      const uint8_t* gs = guide + pix * G;
      g = gs[0];
      if (G == 3) g |= (unsigned)gs[1] << 8 | (unsigned)gs[2] << 16;
      if (first) {
        rf_quantise_pixel<CM>(src + pix * C, is_prob, C, q);
      } else if constexpr (NC == 2) {
        const unsigned u = reinterpret_cast<const unsigned*>(qin)[pix];
        q[0] = u & 0xffffu, q[1] = u >> 16;
      } else if constexpr (NC == 4) {
        const uint2 u = reinterpret_cast<const uint2*>(qin)[pix];
        q[0] = u.x & 0xffffu, q[1] = u.x >> 16, q[2] = u.y & 0xffffu, q[3] = u.y >> 16;
      } else {
#pragma unroll
        for (int c = 0; c < CM; ++c)
          if (c < C) q[c] = qin[pix * C + c];
      }
    }
    const int at = ry * P + rx;
    Gd[at] = g;
#pragma unroll
    for (int j = 0; j < (CM + 1) / 2; ++j)
      if (2 * j < C) Q[j * win + at] = q[2 * j] | (2 * j + 1 < CM ? q[2 * j + 1] : 0u) << 16;       // q is 0 from class C on
  }
  __syncthreads();
  const int64_t pix0 = img + (int64_t)y0 * W + x0;
  const bool interior = y0 >= r && x0 >= r && y0 + th + r <= H && x0 + tw + r <= W;
  const RefineWindow w{Gd, L, Q, win, P, r, shift, C};
  unsigned moved;
  if (interior) moved = rf_filter<NC, false>(w, tb, th, tw, pix0, W, src, is_prob, first, qout, o);
  else moved = rf_filter<NC, true>(w, tb, th, tw, pix0, W, src, is_prob, first, qout, o);
  if (!qout && o.changed) {
    moved = wave_sum(moved);
    if ((threadIdx.x & 63) == 0 && moved) atomicAdd(o.changed + b, (unsigned long long)moved);
  }
}

bool rf_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const char *pa = (const char*)a, *pb = (const char*)b;
  return a && b && pa < pb + nb && pb < pa + na;
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_refine_probs(mgu_ctx* c, const float* src_dev, int is_prob, const uint8_t* guide_dev, int B, int H, int W, int C, int G, int radius,
                     const int32_t* space_lut, const int32_t* range_lut, int shift, int iterations, float* probs_dev, int64_t* labels_dev,
                     float* conf_dev, int64_t* changed_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!src_dev || !guide_dev || !labels_dev || !space_lut || !range_lut)
    return fail(c, MGU_ERR_INVALID, "bad refine_probs args (null source, guide, labels or table)");
  if (B < 0 || H < 0 || W < 0 || B > 65535 || (B > 0 && ((int64_t)H * W > INT_MAX || (int64_t)B * ((int64_t)H * W) > INT_MAX)))
    return fail(c, MGU_ERR_INVALID, "refine_probs: B, H, W >= 0, B <= 65535 and B * H * W below 2^31");
  if (C < 1 || C > RF_MAX_C || (G != 1 && G != 3)) return fail(c, MGU_ERR_INVALID, "refine_probs: %d classes (1..%d), %d guide channels (1 or 3)", C, RF_MAX_C, G);
  if (radius < 1 || radius > RF_MAX_R || iterations < 1 || iterations > RF_MAX_T || shift < 0 || shift > RF_MAX_SHIFT)
    return fail(c, MGU_ERR_INVALID, "refine_probs: radius %d (1..%d: 225 taps keep the uint32 sums exact), iterations %d (1..%d), shift %d (0..%d)",
                radius, RF_MAX_R, iterations, RF_MAX_T, shift, RF_MAX_SHIFT);
  RefineTables tb;
  memset(&tb, 0, sizeof tb);
  const int n1 = radius + 1;
  for (int a = 0; a < n1; ++a)
    for (int d = 0; d < n1; ++d) {
      const int v = space_lut[a * n1 + d];
      if (v < 0 || v > 256) return fail(c, MGU_ERR_INVALID, "refine_probs: space_lut[%d][%d] is %d (0..256)", a, d, v);
      tb.space[a * RF_SP + d] = v;
    }
  for (int k = 0; k < RF_RANGE; ++k) {
    const int v = range_lut[k];
    if (v < 0 || v > 256) return fail(c, MGU_ERR_INVALID, "refine_probs: range_lut[%d] is %d (0..256)", k, v);
    tb.range[k] = (uint16_t)v;
  }
  if (space_lut[0] * range_lut[0] < 128)
    return fail(c, MGU_ERR_INVALID, "refine_probs: space_lut[0][0] * range_lut[0] = %d: the centre weight must be at least 1 (>= 128)",
                space_lut[0] * range_lut[0]);
  const int64_t npix = (int64_t)B * H * W;
  if (npix == 0) return MGU_OK;
  const size_t src_bytes = (size_t)npix * C * 4, guide_bytes = (size_t)npix * G;
  const struct {
    const void* p;
    size_t n;
  } outs[4] = {{probs_dev, src_bytes}, {labels_dev, (size_t)npix * 8}, {conf_dev, (size_t)npix * 4}, {changed_dev, (size_t)B * 8}};
  for (const auto& o : outs)
    if (rf_overlap(o.p, o.n, src_dev, src_bytes) || rf_overlap(o.p, o.n, guide_dev, guide_bytes))
      return fail(c, MGU_ERR_INVALID, "refine_probs: an output must not alias the source or the guide");
  const int NC = C <= 4 ? C : 0, TH = rf_tile_h(NC), TW = rf_tile_w(NC);
  const int tiles_x = (W + TW - 1) / TW;
  const int64_t tiles = (int64_t)tiles_x * ((H + TH - 1) / TH);
  if (tiles > INT_MAX) return fail(c, MGU_ERR_INVALID, "refine_probs: more than 2^31 tiles per image");
  HIPCHK(c, hipSetDevice(c->device));
  // iteration t writes plane set t & 1 and reads the other: one set for two iterations, two beyond
  uint16_t* planes[2] = {nullptr, nullptr};
  if (iterations >= 2) {
    Carve cv;
    const size_t set_bytes = (size_t)npix * C * 2;
    const size_t o0 = cv.take(set_bytes), o1 = iterations >= 3 ? cv.take(set_bytes) : 0;
    if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
    planes[0] = (uint16_t*)((char*)c->objws + o0);
    planes[1] = (uint16_t*)((char*)c->objws + o1);
  }
  hipStream_t s = (hipStream_t)hip_stream;
  if (changed_dev) HIPCHK(c, hipMemsetAsync(changed_dev, 0, (size_t)B * 8, s));
  const dim3 grid((unsigned)tiles, (unsigned)B), block(RF_THREADS);
  const size_t lds = (size_t)rf_lds_bytes(NC, C, radius);
  const RefineOut out{probs_dev, (long long*)labels_dev, conf_dev, (unsigned long long*)changed_dev};
  for (int t = 0; t < iterations; ++t) {
    const int first = t == 0;
    const uint16_t* qin = first ? nullptr : planes[(t - 1) & 1];
    uint16_t* qout = t == iterations - 1 ? nullptr : planes[t & 1];
    ProfScope ps(c, s, "refine_kernel");
#define MGU_RF(N)                                                                                                                          \
  hipLaunchKernelGGL(refine_kernel<N>, grid, block, lds, s, src_dev, is_prob ? 1 : 0, first, qin, guide_dev, H, W, C, G, radius, shift, tiles_x, \
                     tb, qout, out)
    switch (NC) {
      case 1: MGU_RF(1); break;
      case 2: MGU_RF(2); break;
      case 3: MGU_RF(3); break;
      case 4: MGU_RF(4); break;
      default: MGU_RF(0); break;
    }
#undef MGU_RF
    HIPCHK(c, hipGetLastError());
  }
  return MGU_OK;
}

}  // extern "C"
