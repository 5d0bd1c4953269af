// Boundary evaluation on the device: how far the outline of every class in a predicted map lies from the outline of the same class in
// the target map (include/mgunet.h states the definitions).  All integer: bitwise repeatable whatever order the atomics land in.
//   mgu_boundary_tables   prediction (int64 class map or NHWC fp32 logits, argmax fused) + int64 target -> per (image, class):
//                         histograms of the squared surface distances in both directions, their count / unmatched / max / fixed-point
//                         sum of roots, and the band counts of Boundary IoU
// (1) both sides become int32 class planes (2B, H, W): planes 0..B-1 the prediction, B..2B-1 the target.  (2) split.hip's exact
// squared distance transform runs on them: a foreground pixel is a boundary pixel exactly where D2 == 1, and it lies in the band
// where D2 <= band_r2.  (3) site columns: per (plane, class, column) the vertical distance to the nearest boundary pixel of that
// class in the column (uint16, 65535 = none), scanned down and up by 16 threads, a row segment each, that exchange their first and last site.  (4) site rows: a workgroup per (row, class, source
// plane) looks for the row's query pixels -- the source plane's boundary pixels of the class -- and leaves when there are none; else
// it squares the other side's column distances of the row into LDS and every query pixel walks outward over x' for
// min (x - x')^2 + g^2(x') until (x - x')^2 reaches the best value (exact: the nearest site of column x' lies g(x') away, the argument
// of dt_row_kernel).  A row whose columns hold no site at all has only unmatched pixels and nobody walks.  The workgroup histograms
// into LDS and flushes its non-zero bins, the max and the 64-bit sum with integer atomics.  (5) band counts per workgroup in LDS,
// then one integer atomic per non-zero counter.  LDS of (4): 4 bytes per pixel of the row + 4 per bin, at most 80 KiB.
// 6 kernel launches and 3 fills whatever the sizes, the classes and the boundaries; no host synchronisation.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_MAX_D2 = 4096;              // largest histogram: 4098 bins of LDS next to the row
constexpr int BD_MAX_DIM = 16384;            // H, W, as the distance transform's
constexpr int BD_SEGS = 16;                   // row segments of a column in the site column pass: a wave each
constexpr int BD_SITE_NONE = 65535;          // column distance "no boundary pixel of the class in this column" (a real one is < 16384)

typedef unsigned long long u64;

// (1) planes: pixel g of the prediction (pix_key's KIND) and of the target as foreground classes
template <int KIN>
__global__ __launch_bounds__(BD_THREADS) void planes_kernel(const void* __restrict__ pred, const long long* __restrict__ target, int64_t n, int C,
                                                             int ncls, int* __restrict__ cls) {
  const int64_t g = (int64_t)blockIdx.x * BD_THREADS + threadIdx.x;
  if (g >= n) return;
  cls[g] = foreground_class(pix_key<KIN>(pred, g, C), ncls);
  cls[n + g] = foreground_class(target[g], ncls);
}

// a boundary pixel of class c: of that class, and its nearest pixel holding another value is a 4-neighbour
__device__ __forceinline__ bool is_site(const int* __restrict__ cls, const int* __restrict__ d2, int64_t i, int c) { return cls[i] == c && d2[i] == 1; }

// (3) site columns: workgroup = 64 columns of plane blockIdx.z, class blockIdx.y + 1; lane = column, wave = one of BD_SEGS row segments,
// so that a column is scanned by BD_SEGS threads at once.  Down sweep: the distance to the nearest site at or above inside the segment,
// and the segment's first and last site row into LDS.  Up sweep: the nearest site at or below, carried in from the first site of the
// segments below; a row above its segment's first site takes the distance to the last site of the segments above.  gs = the smaller.
__global__ __launch_bounds__(64 * BD_SEGS) void site_col_kernel(const int* __restrict__ cls, const int* __restrict__ d2, int H, int W,
                                                                unsigned short* __restrict__ gs) {
  __shared__ int sfirst[BD_SEGS][64], slast[BD_SEGS][64];
  const int lane = threadIdx.x & 63, seg = threadIdx.x >> 6, x = blockIdx.x * 64 + lane, c = blockIdx.y + 1;
  const int S = (H + BD_SEGS - 1) / BD_SEGS, y0 = min(H, seg * S), y1 = min(H, y0 + S);
  const bool col = x < W;
  const int64_t in = (int64_t)blockIdx.z * H * W + x, out = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * H * W + x;
  int first = -1, last = -1, d = BD_SITE_NONE;
  if (col)
    for (int y = y0; y < y1; ++y) {
      if (is_site(cls, d2, in + (int64_t)y * W, c)) {
        d = 0, last = y;
        if (first < 0) first = y;
      } else if (d < BD_SITE_NONE) {
        ++d;
      }
      gs[out + (int64_t)y * W] = (unsigned short)d;
    }
  sfirst[seg][lane] = first;
  slast[seg][lane] = last;
  __syncthreads();
  if (!col) return;
  int above = -1, below = -1;   // the nearest site row of the column outside the segment
  for (int t = seg - 1; t >= 0 && above < 0; --t) above = slast[t][lane];
  for (int t = seg + 1; t < BD_SEGS && below < 0; ++t) below = sfirst[t][lane];
  d = below >= 0 ? below - y1 : BD_SITE_NONE;   // at the virtual row y1
  for (int y = y1 - 1; y >= y0; --y) {
    if (is_site(cls, d2, in + (int64_t)y * W, c)) d = 0;
    else if (d < BD_SITE_NONE) ++d;
    const int64_t o = out + (int64_t)y * W;
    const int dn = first >= 0 && y >= first ? (int)gs[o] : above >= 0 ? y - above : BD_SITE_NONE;
    gs[o] = (unsigned short)min(dn, d);
  }
}

// floor(sqrt(d2 * 2^32)) = floor(2^16 sqrt(d2)): the fp64 root is a first guess, integer comparisons decide
__device__ __forceinline__ u64 root_q16(int d2) {
  const u64 v = (u64)d2 << 32;
  u64 r = (u64)(sqrt((double)d2) * 65536.0);
  while (r * r > v) --r;
  while ((r + 1) * (r + 1) <= v) ++r;
  return r;
}

// (4) site rows: workgroup = row blockIdx.x, class blockIdx.y + 1, source plane blockIdx.z (< B: prediction -> target, direction 0;
// else target -> prediction, direction 1).  LDS: squared site column distances [W], histogram [max_d2 + 2]
__global__ __launch_bounds__(BD_THREADS) void site_row_kernel(const int* __restrict__ cls, const int* __restrict__ d2,
                                                              const unsigned short* __restrict__ gs, int B, int W, int max_d2,
                                                              u64* __restrict__ hist, u64* __restrict__ stats) {
  extern __shared__ int bd_row[];
  __shared__ u64 st[4];   // the workgroup's n, unmatched, max, sum
  int* sc = bd_row;
  int* sh = bd_row + W;
  const int tid = threadIdx.x, y = blockIdx.x, H = gridDim.x, k = blockIdx.y, K = gridDim.y, c = k + 1, src = blockIdx.z;
  const int dir = src >= B, b = src - dir * B, dst = (1 - dir) * B + b;
  const int64_t qrow = ((int64_t)src * H + y) * W;
  bool any = false;
  for (int x = tid; x < W; x += BD_THREADS) any |= is_site(cls, d2, qrow + x, c);
  if (!__syncthreads_or(any)) return;   // uniform: no query pixel in this row
  const int64_t srow = (((int64_t)dst * K + k) * H + y) * W;
  const int bins = max_d2 + 2;
  bool sites = false;
  for (int x = tid; x < W; x += BD_THREADS) {
    const int v = gs[srow + x];
    sc[x] = v == BD_SITE_NONE ? MGU_D2_NONE : v * v;
    sites |= v != BD_SITE_NONE;
  }
  for (int i = tid; i < bins; i += BD_THREADS) sh[i] = 0;
  if (tid < 4) st[tid] = 0;
  sites = __syncthreads_or(sites);   // also the barrier behind sc and sh; no site in any column: the class has no boundary over there
  unsigned n = 0, unmatched = 0;
  int mx = 0;
  u64 sum = 0;
  for (int x = tid; x < W; x += BD_THREADS) {
    if (!is_site(cls, d2, qrow + x, c)) continue;
    ++n;
    if (!sites) {
      ++unmatched;
      continue;
    }
    int best = sc[x];
    for (int dx = 1;; ++dx) {   // outward from x; no x' farther than sqrt(best) can improve it
      const int dd = dx * dx, xl = x - dx, xr = x + dx;
      if (dd >= best || (xl < 0 && xr >= W)) break;
      if (xl >= 0) best = min(best, dd + sc[xl]);
      if (xr < W) best = min(best, dd + sc[xr]);
    }
    atomicAdd(&sh[min(best, max_d2 + 1)], 1);
    mx = max(mx, best);
    sum += root_q16(best);
  }
  if (unmatched) atomicAdd(&sh[max_d2 + 1], (int)unmatched);
  n = wave_sum(n);
  unmatched = wave_sum(unmatched);
  mx = wave_max(mx);
  sum = wave_sum(sum);
  if ((tid & 63) == 0 && n) {   // the waves of the workgroup first: the rows of an image all add to the same four words
    atomicAdd(&st[0], (u64)n);
    atomicAdd(&st[1], (u64)unmatched);
    atomicMax(&st[2], (u64)mx);
    atomicAdd(&st[3], sum);
  }
  __syncthreads();
  const int64_t slot = ((int64_t)b * K + k) * 2 + dir;
  if (tid < 4 && st[tid]) {
    if (tid == 2) atomicMax(&stats[slot * 4 + 2], st[2]);
    else atomicAdd(&stats[slot * 4 + tid], st[tid]);
  }
  for (int i = tid; i < bins; i += BD_THREADS)
    if (sh[i]) atomicAdd(&hist[slot * bins + i], (u64)sh[i]);
}

// (5) bands: workgroup = 256 consecutive pixels of image blockIdx.y; counters [class][inter, pred, target] in LDS.  A wave counts the
// classes it holds with ballots: a wide band puts most lanes on the same counter
__global__ __launch_bounds__(BD_THREADS) void band_kernel(const int* __restrict__ cls, const int* __restrict__ d2, int64_t HW, int64_t n, int K,
                                                          int band_r2, u64* __restrict__ band) {
  __shared__ unsigned cnt[3 * 31];
  const int tid = threadIdx.x;
  if (tid < 3 * K) cnt[tid] = 0;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * BD_THREADS + tid;
  int cp = 0, ct = 0;   // the pixel's class where it lies in the band, else 0
  if (i < HW) {
    const int64_t gp = (int64_t)blockIdx.y * HW + i, gt = n + gp;
    cp = cls[gp], ct = cls[gt];
    if (cp != 0 && d2[gp] > band_r2) cp = 0;
    if (ct != 0 && d2[gt] > band_r2) ct = 0;
  }
  unsigned present = wave_or((1u << cp) | (1u << ct)) & ~1u;   // reached by the whole wave
  while (present) {
    const int c = __ffs((int)present) - 1;
    present &= present - 1;
    const unsigned np = (unsigned)__popcll(__ballot(cp == c)), ng = (unsigned)__popcll(__ballot(ct == c));
    const unsigned ni = (unsigned)__popcll(__ballot(cp == c && ct == c));
    if ((tid & 63) == 0) {
      if (ni) atomicAdd(&cnt[3 * (c - 1)], ni);
      if (np) atomicAdd(&cnt[3 * (c - 1) + 1], np);
      if (ng) atomicAdd(&cnt[3 * (c - 1) + 2], ng);
    }
  }
  __syncthreads();
  if (tid < 3 * K && cnt[tid]) atomicAdd(&band[(int64_t)blockIdx.y * 3 * K + tid], (u64)cnt[tid]);
}

bool g_site_row_lds[64];

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_boundary_tables(mgu_ctx* c, const void* pred_dev, int pred_kind, const int64_t* target_dev, int B, int H, int W, int C,
                        int64_t num_classes, int max_d2, int band_r2, int64_t* hist_dev, int64_t* stats_dev, int64_t* band_dev,
                        void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!pred_dev || !target_dev || !hist_dev || !stats_dev || !band_dev || B < 0 || H < 0 || W < 0)
    return fail(c, MGU_ERR_INVALID, "bad boundary_tables args (null pointer or negative size)");
  if (pred_kind != 0 && pred_kind != 1) return fail(c, MGU_ERR_INVALID, "boundary_tables: pred_kind %d (0 int64 class map, 1 fp32 logits)", pred_kind);
  if (num_classes < 2 || num_classes > 32) return fail(c, MGU_ERR_INVALID, "boundary_tables: num_classes %lld (2..32)", (long long)num_classes);
  if (pred_kind == 1 && C != num_classes)
    return fail(c, MGU_ERR_INVALID, "boundary_tables: logits of %d channels for num_classes %lld", C, (long long)num_classes);
  if (max_d2 < 1 || max_d2 > BD_MAX_D2) return fail(c, MGU_ERR_INVALID, "boundary_tables: max_d2 %d (1..%d)", max_d2, BD_MAX_D2);
  if (band_r2 < 1) return fail(c, MGU_ERR_INVALID, "boundary_tables: band_r2 %d (>= 1)", band_r2);
  if (B > 32767) return fail(c, MGU_ERR_INVALID, "boundary_tables: at most 32767 images per call");
  if (int rc = distance_transform_dims(c, "boundary_tables (2B planes)", 2 * B, H, W)) return rc;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  if (n == 0) return MGU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int ncls = (int)num_classes, K = ncls - 1, bins = max_d2 + 2;
  Carve cv;
  const size_t oC = cv.take((size_t)n * 8);          // int32 class planes (2B, H, W)
  const size_t oG = cv.take((size_t)n * 8);          // the distance transform's column distances
  const size_t oD = cv.take((size_t)n * 8);          // D2 of the planes
  const size_t oS = cv.take((size_t)n * 4 * K);      // uint16 site column distances (2B, K, H, W)
  int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off);
  if (rc) return rc;
  char* ws = (char*)c->objws;
  int* cls = (int*)(ws + oC);
  int* d2 = (int*)(ws + oD);
  unsigned short* gs = (unsigned short*)(ws + oS);
  u64 *hist = (u64*)hist_dev, *stats = (u64*)stats_dev, *band = (u64*)band_dev;
  const size_t lds = ((size_t)W + bins) * 4;
  if (lds > 65536) {   // the opt-in is set once per device: for the widest row and the largest histogram
    int budget = 0;
    HIPCHK(c, hipDeviceGetAttribute(&budget, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    if (lds > (size_t)budget) return fail(c, MGU_ERR_INVALID, "boundary_tables: a row of %d pixels and %d bins need %zu bytes of LDS, the device gives one workgroup %d", W, bins, lds, budget);
    HIPCHK(c, ensure_dyn_lds((const void*)site_row_kernel, std::min((size_t)(BD_MAX_DIM + BD_MAX_D2 + 2) * 4, (size_t)budget), g_site_row_lds));
  }
  HIPCHK(c, hipMemsetAsync(hist, 0, (size_t)B * K * 2 * bins * sizeof(u64), s));
  HIPCHK(c, hipMemsetAsync(stats, 0, (size_t)B * K * 2 * 4 * sizeof(u64), s));
  HIPCHK(c, hipMemsetAsync(band, 0, (size_t)B * K * 3 * sizeof(u64), s));

  const unsigned pixblocks = grid_for(n, BD_THREADS, INT_MAX);
  if (pred_kind == 0) hipLaunchKernelGGL(planes_kernel<0>, dim3(pixblocks), dim3(BD_THREADS), 0, s, pred_dev, (const long long*)target_dev, n, C, ncls, cls);
  else hipLaunchKernelGGL(planes_kernel<1>, dim3(pixblocks), dim3(BD_THREADS), 0, s, pred_dev, (const long long*)target_dev, n, C, ncls, cls);
  rc = distance_transform(c, cls, 2 * B, H, W, -1, (int*)(ws + oG), d2, s);
  if (rc) return rc;
  hipLaunchKernelGGL(site_col_kernel, dim3((W + 63) / 64, K, 2 * B), dim3(64 * BD_SEGS), 0, s, cls, d2, H, W, gs);
  hipLaunchKernelGGL(site_row_kernel, dim3(H, K, 2 * B), dim3(BD_THREADS), lds, s, cls, d2, gs, B, W, max_d2, hist, stats);
  hipLaunchKernelGGL(band_kernel, dim3(grid_for(HW, BD_THREADS, INT_MAX), B), dim3(BD_THREADS), 0, s, cls, d2, HW, n, K, band_r2, band);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
