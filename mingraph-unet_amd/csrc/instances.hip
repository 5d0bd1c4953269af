// Instance evaluation on the device: the overlap of every (GT object, predicted object) pair of two label maps, and what sits on it.
//   mgu_object_overlaps   two int32 label maps (B, H, W) -> the pairs that share a pixel, CSR by predicted object: pair_ptr, pair_gt
//                         (ascending inside a row), pair_inter (pixels carrying both labels)
//   mgu_match_masks       the confidence-ordered greedy matching of metrics.py:215-240 on mask IoU, for T thresholds at once
//   mgu_panoptic_totals   the strict-majority matching of panoptic quality: per class [TP, FP, FN, sum of IoU in 2^-32 fixed point]
// The overlap table is an open-addressing hash table in global scratch keyed by (pred index << 32 | gt index), both batch-wide:
// (1) every pixel group looks its pair up (64-bit compare-and-swap inserts it, the winner bumps the row's degree) and adds its pixel
// count with an integer atomic, (2) the degrees are scanned into pair_ptr, (3) the occupied slots are poured into their rows in
// whatever order the atomics land in, (4) every entry finds its rank inside its row by counting the smaller GT indices and is stored
// there.  The slot a pair lands in varies from run to run; the outputs do not: counts are integer sums and the in-row order is the
// rank.  Step (4) is one thread per entry, so a long row (one predicted object over thousands of GT objects) is ranked by as many
// threads as it has entries.
// Contention.  One full-image object on both sides sends every pixel to one counter, so pixels are combined before the atomic: a lane
// holds 4 consecutive pixels (one 16-byte load per map) and folds equal neighbours in registers; lanes whose 4 pixels all carry one
// pair form runs inside the wave (ballot arithmetic) and only a run's first lane issues one add of the run's pixel count.  The keys
// are batch-wide object indices, which differ between images, so a run never joins pixels of two images.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int IN_THREADS = 256;
constexpr int PIXG = 4;                         // pixels per lane in the counting pass
constexpr int ROWCHUNK = PAIR_ROWCHUNK;         // the pair table, its probing and its degree / pour / place kernels: objects_common.h
constexpr unsigned long long EMPTY = PAIR_EMPTY;

// (1) one lane per PIXG consecutive pixels of the flat (B, H*W) maps
template <bool VEC>
__global__ __launch_bounds__(IN_THREADS) void overlap_count_kernel(const int* __restrict__ glab, const int* __restrict__ plab, int64_t n, int64_t HW,
                                                                   const long long* __restrict__ goff, const long long* __restrict__ poff,
                                                                   int64_t gcap, int64_t pcap, PairTable t) {
  const int lane = threadIdx.x & 63;
  const int64_t i0 = ((int64_t)blockIdx.x * IN_THREADS + threadIdx.x) * PIXG;
  const bool whole = i0 + PIXG <= n;
  int a[PIXG] = {0, 0, 0, 0}, c[PIXG] = {0, 0, 0, 0};
  if (whole && VEC) {
    const int4 va = *reinterpret_cast<const int4*>(glab + i0), vc = *reinterpret_cast<const int4*>(plab + i0);
    a[0] = va.x, a[1] = va.y, a[2] = va.z, a[3] = va.w;
    c[0] = vc.x, c[1] = vc.y, c[2] = vc.z, c[3] = vc.w;
  } else {
#pragma unroll
    for (int j = 0; j < PIXG; ++j)
      if (i0 + j < n) a[j] = glab[i0 + j], c[j] = plab[i0 + j];
  }
  unsigned long long k[PIXG];
  int64_t b = -1;
  long long g0 = 0, p0 = 0, G = 0, NP = 0;
#pragma unroll
  for (int j = 0; j < PIXG; ++j) {
    k[j] = EMPTY;
    if (a[j] <= 0 || c[j] <= 0) continue;
    const int64_t bj = (i0 + j) / HW;
    if (bj != b) {   // an image whose objects pass a capacity contributes no pairs (G = NP = 0 rejects every label)
      b = bj;
      g0 = goff[b], p0 = poff[b];
      G = goff[b + 1] - g0, NP = poff[b + 1] - p0;
      if (g0 + G > gcap || p0 + NP > pcap || p0 + NP > t.rows) G = NP = 0;
    }
    if (a[j] <= G && c[j] <= NP) k[j] = ((unsigned long long)(p0 + c[j] - 1) << 32) | (unsigned long long)(g0 + a[j] - 1);
  }
  const bool uniform = whole && k[0] == k[1] && k[1] == k[2] && k[2] == k[3];
  if (!uniform) {   // a lane on an object's border: its own runs, folded in registers
    int j = 0;
    while (j < PIXG) {
      int m = 1;
      while (j + m < PIXG && k[j + m] == k[j]) ++m;
      if (k[j] != EMPTY) pair_add(t, k[j], (unsigned)m);
      j += m;
    }
  }
  // runs of uniform lanes holding one pair: the first lane of a run adds PIXG pixels for every lane of it
  const unsigned long long K = k[0], prevK = __shfl_up(K, 1);
  const int prevU = __shfl_up((int)uniform, 1);
  const bool start = uniform && (lane == 0 || !prevU || prevK != K);
  const unsigned long long S = __ballot(start), U = __ballot(uniform);
  if (start && K != EMPTY) {
    const unsigned long long above = lane == 63 ? 0ull : (~0ull << (lane + 1));
    const unsigned long long stop = (S | ~U) & above;
    const int end = stop ? __ffsll((long long)stop) - 1 : 64;
    pair_add(t, K, (unsigned)(PIXG * (end - lane)));
  }
}

// (2b) one workgroup: exclusive scan of the chunk sums; the number of pairs; the status bits
__global__ __launch_bounds__(SCAN_THREADS) void degree_scan_kernel(const int* __restrict__ csum, int64_t nch, long long* __restrict__ choff,
                                                                   long long* __restrict__ total_out, int64_t pair_cap, int B,
                                                                   const long long* __restrict__ goff, const long long* __restrict__ poff,
                                                                   int64_t gcap, int64_t pcap, int* __restrict__ status) {
  const int tid = threadIdx.x;
  const long long pairs = chunk_sum_scan(csum, nch, choff);
  int bits = 0;
  for (int b = tid; b < B; b += SCAN_THREADS)
    if (goff[b + 1] > gcap || poff[b + 1] > pcap) bits |= 2;
  if (tid == SCAN_THREADS - 1) {
    *total_out = pairs;
    if (pairs > pair_cap) bits |= 1;
  }
  if (bits) atomicOr(status, bits);
}

// ---- confidence-ordered greedy matching on mask IoU ------------------------------------------------------------------------------
// descending-score sort key: larger first; NaN last; -0 = +0 (they tie, and a tie goes to the smaller index)
__device__ __forceinline__ unsigned score_key(float s) {
  if (s != s) return 0u;
  if (s == 0.f) s = 0.f;
  const unsigned u = __float_as_uint(s);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// order[p0 + r] = the local index of the image's r-th prediction: r = the number of predictions that come before it
__global__ __launch_bounds__(IN_THREADS) void score_rank_kernel(const long long* __restrict__ poff, int64_t pcap, const float* __restrict__ scores,
                                                                int* __restrict__ order) {
  const int b = blockIdx.y;
  const long long p0 = poff[b], NP = poff[b + 1] - p0;
  if (p0 + NP > pcap) return;
  for (long long i = (long long)blockIdx.x * IN_THREADS + threadIdx.x; i < NP; i += (long long)gridDim.x * IN_THREADS) {
    const unsigned ki = score_key(scores[p0 + i]);
    long long r = 0;
    for (long long j = 0; j < NP; ++j) {
      const unsigned kj = score_key(scores[p0 + j]);
      r += (kj > ki) || (kj == ki && j < i);
    }
    order[p0 + r] = (int)i;
  }
}

// One wave per image, lane t = threshold t with its own used flags (used + t * gcap, touched by that lane alone after the clearing).
// Predictions in score order; each scans its row: unused GT objects of its class, IoU in fp64 = inter / (a_p + a_g - inter) (Python's
// int / int); the strictly larger IoU wins, and as a row ascends in GT index an equal IoU leaves the smaller index in place.
__global__ __launch_bounds__(64) void mask_match_kernel(const long long* __restrict__ pair_ptr, const long long* __restrict__ pair_gt,
                                                        const long long* __restrict__ pair_inter, int64_t pair_cap,
                                                        const long long* __restrict__ goff, const long long* __restrict__ gcls,
                                                        const long long* __restrict__ garea, int64_t gcap, const long long* __restrict__ poff,
                                                        const long long* __restrict__ pcls, const long long* __restrict__ parea, int64_t pcap,
                                                        const int* __restrict__ order, const double* __restrict__ thr, int T,
                                                        unsigned char* __restrict__ used, long long* __restrict__ match_gt,
                                                        double* __restrict__ match_iou, unsigned long long* __restrict__ totals) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const long long g0 = goff[b], G = goff[b + 1] - g0, p0 = poff[b], NP = poff[b + 1] - p0;
  if (g0 + G > gcap || p0 + NP > pcap) return;   // objects past the arrays' capacity were not recorded
  for (int t = 0; t < T; ++t)
    for (long long j = lane; j < G; j += 64) used[(int64_t)t * gcap + g0 + j] = 0;
  __syncthreads();
  if (lane >= T) return;
  const double th = thr[lane];
  unsigned char* u = used + (int64_t)lane * gcap;
  long long* mg = match_gt + (int64_t)lane * pcap;
  double* mi = match_iou + (int64_t)lane * pcap;
  unsigned long long matched = 0;
  for (long long i = 0; i < NP; ++i) {
    const long long p = p0 + (order ? order[p0 + i] : i);
    const long long pc = pcls[p], ap = parea[p];
    const long long r0 = pair_ptr[p], r1 = min(pair_ptr[p + 1], (long long)pair_cap);
    double best = 0.0;
    long long bj = -1;
    for (long long e = r0; e < r1; ++e) {
      const long long g = pair_gt[e];
      if (gcls[g] != pc || u[g]) continue;
      const long long inter = pair_inter[e];
      const double iou = (double)inter / (double)(ap + garea[g] - inter);
      if (iou > best) best = iou, bj = g;
    }
    const bool hit = bj >= 0 && best >= th;
    if (hit) u[bj] = 1, ++matched;
    mg[p] = hit ? bj : -1;
    mi[p] = hit ? best : 0.0;
  }
  atomicAdd(&totals[3 * lane], (unsigned long long)G);
  atomicAdd(&totals[3 * lane + 1], (unsigned long long)NP);
  atomicAdd(&totals[3 * lane + 2], matched);
}

// ---- panoptic quality ------------------------------------------------------------------------------------------------------------
// add one record per lane to pq[cls] (cls < 0: none): the lanes of one class are summed inside the wave (wave_by_key)
__device__ __forceinline__ void class_add(unsigned long long* pq, long long cls, unsigned long long v0, unsigned long long v1,
                                          unsigned long long v2, unsigned long long v3) {
  auto add = [=](long long k, unsigned long long s0, unsigned long long s1, unsigned long long s2, unsigned long long s3) {
    if (s0) atomicAdd(&pq[4 * k], s0);
    if (s1) atomicAdd(&pq[4 * k + 1], s1);
    if (s2) atomicAdd(&pq[4 * k + 2], s2);
    if (s3) atomicAdd(&pq[4 * k + 3], s3);
  };
  wave_by_key(
      cls,
      [=](long long lc, bool mine, bool lead) {
        const unsigned long long s0 = wave_sum<unsigned long long>(mine ? v0 : 0ull), s1 = wave_sum<unsigned long long>(mine ? v1 : 0ull);
        const unsigned long long s2 = wave_sum<unsigned long long>(mine ? v2 : 0ull), s3 = wave_sum<unsigned long long>(mine ? v3 : 0ull);
        if (lead) add(lc, s0, s1, s2, s3);
      },
      [=] { add(cls, v0, v1, v2, v3); });
}

// grid (x, images): thread i of an image takes its i-th predicted object (TP with its IoU, or FP) and its i-th GT object (one FN;
// every TP takes one FN back: the sums are modulo 2^64 and end at GT objects - TP).  2 inter > a_p + a_g - inter holds for at most
// one GT object per prediction and one prediction per GT object, so there is no order to respect.
__global__ __launch_bounds__(IN_THREADS) void panoptic_kernel(const long long* __restrict__ pair_ptr, const long long* __restrict__ pair_gt,
                                                              const long long* __restrict__ pair_inter, int64_t pair_cap,
                                                              const long long* __restrict__ goff, const long long* __restrict__ gcls,
                                                              const long long* __restrict__ garea, int64_t gcap, const long long* __restrict__ poff,
                                                              const long long* __restrict__ pcls, const long long* __restrict__ parea, int64_t pcap,
                                                              int ncls, unsigned long long* __restrict__ pq) {
  const int b = blockIdx.y;
  const long long g0 = goff[b], G = goff[b + 1] - g0, p0 = poff[b], NP = poff[b + 1] - p0;
  if (g0 + G > gcap || p0 + NP > pcap) return;
  const long long most = G > NP ? G : NP;
  for (long long base = (long long)blockIdx.x * IN_THREADS; base < most; base += (long long)gridDim.x * IN_THREADS) {
    const long long i = base + threadIdx.x;
    long long pc = -1;
    unsigned long long tp = 0, fix = 0;
    if (i < NP) {
      const long long p = p0 + i, ap = parea[p];
      pc = pcls[p];
      if (pc < 0 || pc >= ncls) pc = -1;
      const long long r0 = pair_ptr[p], r1 = min(pair_ptr[p + 1], (long long)pair_cap);
      for (long long e = r0; pc >= 0 && e < r1; ++e) {
        const long long g = pair_gt[e], inter = pair_inter[e], uni = ap + garea[g] - inter;
        if (gcls[g] == pc && 2 * inter > uni) {
          tp = 1;
          fix = __double2ull_rn((double)inter / (double)uni * 4294967296.0);
          break;
        }
      }
    }
    class_add(pq, pc, tp, 1 - tp, 0ull - tp, fix);
    long long gc = i < G ? gcls[g0 + i] : -1;
    if (gc >= ncls) gc = -1;
    class_add(pq, gc, 0, 0, 1, 0);
  }
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_object_overlaps(mgu_ctx* c, const int32_t* gt_labels_dev, const int64_t* gt_offsets_dev, int64_t gt_capacity,
                        const int32_t* pred_labels_dev, const int64_t* pred_offsets_dev, int64_t pred_capacity, int B, int H, int W,
                        int64_t pair_capacity, int64_t* pair_ptr_dev, int64_t* pair_gt_dev, int64_t* pair_inter_dev, int32_t* status_dev,
                        void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!gt_labels_dev || !gt_offsets_dev || !pred_labels_dev || !pred_offsets_dev || !pair_ptr_dev || !status_dev || B < 0 || H < 0 || W < 0 ||
      gt_capacity < 0 || pred_capacity < 0 || pair_capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad object_overlaps args (null pointer or negative size)");
  if (pair_capacity > 0 && (!pair_gt_dev || !pair_inter_dev)) return fail(c, MGU_ERR_INVALID, "object_overlaps: pair arrays are needed for a nonzero pair_capacity");
  if (int rc = check_pixel_count(c, "object_overlaps", B, H, W)) return rc;
  if (pred_capacity >= 2147483647ll || gt_capacity >= 2147483647ll) return fail(c, MGU_ERR_INVALID, "object_overlaps: capacities must stay below 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const int64_t nptr = pred_capacity + 1;
  PairTable t;
  t.rows = std::min<int64_t>(pred_capacity, n);       // an image has at most H*W objects: no row past n can be an object's
  t.slots = (unsigned)std::min<int64_t>(2 * n + 64, 0xFFFFFFFFll);   // pairs <= pixels: the table stays about half full at most
  const int64_t nch = (nptr + ROWCHUNK - 1) / ROWCHUNK;
  Carve cv;
  const size_t oK = cv.take((size_t)t.slots * 8), oZ = cv.take((size_t)t.slots * 4), oD = cv.take((size_t)(t.rows + 1) * 4);
  const size_t zero_bytes = cv.off - oZ;               // counters and degrees are cleared together
  const size_t oP = cv.take((size_t)(n + 1) * 4), oG = cv.take((size_t)(n + 1) * 4), oC = cv.take((size_t)(n + 1) * 4);
  const size_t oS = cv.take((size_t)nch * 4), oO = cv.take((size_t)nch * 8), oT = cv.take(8);
  int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off);
  if (rc) return rc;
  char* ws = (char*)c->objws;
  t.keys = (unsigned long long*)(ws + oK), t.cnt = (unsigned*)(ws + oZ), t.deg = (int*)(ws + oD);
  int *tp = (int*)(ws + oP), *csum = (int*)(ws + oS);
  unsigned *tg = (unsigned*)(ws + oG), *tc = (unsigned*)(ws + oC);
  long long *choff = (long long*)(ws + oO), *total = (long long*)(ws + oT);
  const long long *goff = (const long long*)gt_offsets_dev, *poff = (const long long*)pred_offsets_dev;
  HIPCHK(c, hipMemsetAsync(t.keys, 0xFF, (size_t)t.slots * 8, s));
  HIPCHK(c, hipMemsetAsync(t.cnt, 0, zero_bytes, s));
  if (n > 0) {
    const unsigned blocks = grid_for(n, IN_THREADS * PIXG, INT_MAX);
    const bool vec = (((uintptr_t)gt_labels_dev | (uintptr_t)pred_labels_dev) & 15) == 0;
    if (vec)
      hipLaunchKernelGGL(overlap_count_kernel<true>, dim3(blocks), dim3(IN_THREADS), 0, s, gt_labels_dev, pred_labels_dev, n, HW, goff, poff,
                         gt_capacity, pred_capacity, t);
    else
      hipLaunchKernelGGL(overlap_count_kernel<false>, dim3(blocks), dim3(IN_THREADS), 0, s, gt_labels_dev, pred_labels_dev, n, HW, goff, poff,
                         gt_capacity, pred_capacity, t);
  }
  hipLaunchKernelGGL(degree_count_kernel<0>, dim3((unsigned)nch), dim3(IN_THREADS), 0, s, t.deg, t.rows, csum);
  hipLaunchKernelGGL(degree_scan_kernel, dim3(1), dim3(SCAN_THREADS), 0, s, csum, nch, choff, total, pair_capacity, B, goff, poff, gt_capacity,
                     pred_capacity, (int*)status_dev);
  hipLaunchKernelGGL(degree_write_kernel<long long>, dim3((unsigned)nch), dim3(IN_THREADS), 0, s, t.deg, t.rows, nptr, choff, (long long*)pair_ptr_dev);
  const unsigned slotblocks = grid_for(t.slots, IN_THREADS, 4096);
  hipLaunchKernelGGL(pair_pour_kernel<long long>, dim3(slotblocks), dim3(IN_THREADS), 0, s, t, (const long long*)pair_ptr_dev, tp, tg, tc);
  const unsigned pairblocks = grid_for(n + 1, IN_THREADS, 4096);   // the pairs are counted on the device: at most n
  hipLaunchKernelGGL((pair_place_kernel<long long, long long>), dim3(pairblocks), dim3(IN_THREADS), 0, s, total, (const long long*)pair_ptr_dev, tp, tg, tc, pair_capacity,
                     (long long*)pair_gt_dev, (long long*)pair_inter_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

static int check_sides(mgu_ctx* c, const char* fn, int B, const void* pair_ptr, const void* pair_gt, const void* pair_inter, int64_t pair_capacity,
                       const void* goff, const void* gcls, const void* garea, int64_t gcap, const void* poff, const void* pcls, const void* parea,
                       int64_t pcap) {
  if (!pair_ptr || !goff || !poff || B < 0 || pair_capacity < 0 || gcap < 0 || pcap < 0)
    return fail(c, MGU_ERR_INVALID, "bad %s args (null pointer or negative size)", fn);
  if ((pair_capacity > 0 && (!pair_gt || !pair_inter)) || (gcap > 0 && (!gcls || !garea)) || (pcap > 0 && (!pcls || !parea)))
    return fail(c, MGU_ERR_INVALID, "%s: the pair, class and area arrays are needed for a nonzero capacity", fn);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "%s: at most 65535 images per call", fn);
  return MGU_OK;
}

int mgu_match_masks(mgu_ctx* c, int B, const int64_t* pair_ptr_dev, const int64_t* pair_gt_dev, const int64_t* pair_inter_dev, int64_t pair_capacity,
                    const int64_t* gt_offsets_dev, const int64_t* gt_class_dev, const int64_t* gt_area_dev, int64_t gt_capacity,
                    const int64_t* pred_offsets_dev, const int64_t* pred_class_dev, const int64_t* pred_area_dev, int64_t pred_capacity,
                    const float* scores_dev, const double* thresholds_dev, int T, int64_t* match_gt_dev, double* match_iou_dev,
                    int64_t* totals_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  int rc = check_sides(c, "match_masks", B, pair_ptr_dev, pair_gt_dev, pair_inter_dev, pair_capacity, gt_offsets_dev, gt_class_dev, gt_area_dev,
                       gt_capacity, pred_offsets_dev, pred_class_dev, pred_area_dev, pred_capacity);
  if (rc) return rc;
  if (T < 1 || T > 16 || !thresholds_dev || !totals_dev) return fail(c, MGU_ERR_INVALID, "match_masks: 1 <= T <= 16 thresholds and totals are needed");
  if (pred_capacity > 0 && (!match_gt_dev || !match_iou_dev)) return fail(c, MGU_ERR_INVALID, "match_masks: match arrays are needed for a nonzero capacity");
  HIPCHK(c, hipSetDevice(c->device));
  if (B == 0) return MGU_OK;
  hipStream_t s = (hipStream_t)hip_stream;
  Carve cv;
  const size_t oU = cv.take((size_t)T * std::max<int64_t>(gt_capacity, 1)), oO = cv.take((size_t)std::max<int64_t>(pred_capacity, 1) * 4);
  rc = ensure(c, &c->objws, &c->objws_bytes, cv.off);
  if (rc) return rc;
  char* ws = (char*)c->objws;
  int* order = scores_dev ? (int*)(ws + oO) : nullptr;
  const long long *goff = (const long long*)gt_offsets_dev, *poff = (const long long*)pred_offsets_dev;
  if (scores_dev) hipLaunchKernelGGL(score_rank_kernel, dim3(64, B), dim3(IN_THREADS), 0, s, poff, pred_capacity, scores_dev, order);
  hipLaunchKernelGGL(mask_match_kernel, dim3(B), dim3(64), 0, s, (const long long*)pair_ptr_dev, (const long long*)pair_gt_dev,
                     (const long long*)pair_inter_dev, pair_capacity, goff, (const long long*)gt_class_dev, (const long long*)gt_area_dev, gt_capacity,
                     poff, (const long long*)pred_class_dev, (const long long*)pred_area_dev, pred_capacity, order, thresholds_dev, T,
                     (unsigned char*)(ws + oU), (long long*)match_gt_dev, match_iou_dev, (unsigned long long*)totals_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_panoptic_totals(mgu_ctx* c, int B, const int64_t* pair_ptr_dev, const int64_t* pair_gt_dev, const int64_t* pair_inter_dev,
                        int64_t pair_capacity, const int64_t* gt_offsets_dev, const int64_t* gt_class_dev, const int64_t* gt_area_dev,
                        int64_t gt_capacity, const int64_t* pred_offsets_dev, const int64_t* pred_class_dev, const int64_t* pred_area_dev,
                        int64_t pred_capacity, int num_classes, uint64_t* pq_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  int rc = check_sides(c, "panoptic_totals", B, pair_ptr_dev, pair_gt_dev, pair_inter_dev, pair_capacity, gt_offsets_dev, gt_class_dev, gt_area_dev,
                       gt_capacity, pred_offsets_dev, pred_class_dev, pred_area_dev, pred_capacity);
  if (rc) return rc;
  if (num_classes < 1 || !pq_dev) return fail(c, MGU_ERR_INVALID, "panoptic_totals: num_classes >= 1 and pq are needed");
  HIPCHK(c, hipSetDevice(c->device));
  if (B == 0) return MGU_OK;
  hipLaunchKernelGGL(panoptic_kernel, dim3(16, B), dim3(IN_THREADS), 0, (hipStream_t)hip_stream, (const long long*)pair_ptr_dev,
                     (const long long*)pair_gt_dev, (const long long*)pair_inter_dev, pair_capacity, (const long long*)gt_offsets_dev,
                     (const long long*)gt_class_dev, (const long long*)gt_area_dev, gt_capacity, (const long long*)pred_offsets_dev,
                     (const long long*)pred_class_dev, (const long long*)pred_area_dev, pred_capacity, num_classes,
                     (unsigned long long*)pq_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
