// Splitting touching objects on the device: the exact squared Euclidean distance transform of a label map, one seed per inscribed
// disc and the power diagram of those discs (include/mgunet.h states the definitions).  All integer: bitwise repeatable.
//   mgu_distance_transform   int32 labels (B, H, W) -> int32 D2: squared distance to the nearest pixel holding another label
//   mgu_split_objects        labels -> labels of the split objects, counts, offsets (and, on request, D2 and the seed mask)
// D2 in two passes: (1) a lane per column scans down and up for the vertical distance g to the nearest other label; (2) a
// workgroup per row keeps the row's labels and g^2 in LDS, and every pixel walks outward over x' for min (x - x')^2 + c(x'),
// c = 0 where the label differs and g^2 where it does not, until (x - x')^2 reaches the best value: exact, because the nearest
// other-label pixel of a same-label column x' lies g(x') away.  The row buffer is 8 bytes per pixel of LDS: W <= 16384 (128 KiB).
// Split: (3) seed test in a tile with an r-pixel apron, (4) zone map in a tile with an h-pixel apron, labelled by objects.hip's
// union-find (cc_roots_i32), (5) seeds bucketed per component (count, bucket start, scatter), (6) every foreground pixel scans its
// component's bucket, staged through LDS, (7) the first pixel of every new object by atomicMin, then objects.hip's numbering tail.
// The launch count is fixed: it depends on no size, object count or seed count.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int SP_THREADS = 256;
constexpr int SP_TILE = 32;                  // seed / zone tile: SP_TILE x SP_TILE pixels, 4 per thread
constexpr int SP_MAX_R = 16;                 // largest min_distance: the seed tile's apron
constexpr int SP_MAX_DIM = 16384;            // H, W: coordinates pack into 16 bits, D2 stays below MGU_D2_NONE
constexpr int G_NONE = 32768;                // column distance "no other label in this column"; G_NONE^2 = MGU_D2_NONE
static_assert((long long)G_NONE * G_NONE == MGU_D2_NONE, "the sentinel is the square of the column sentinel");

// the label of a pixel: maxlab >= 0 (the split, whose tables are indexed by label) reads a label outside [0, maxlab] as background
__device__ __forceinline__ int lab_in(int l, int maxlab) { return (maxlab >= 0 && (unsigned)l > (unsigned)maxlab) ? 0 : l; }

// (1) columns: lane = column x of image blockIdx.y; g = vertical distance to the nearest pixel of the column with another label
__global__ __launch_bounds__(64) void dt_col_kernel(const int* __restrict__ labels, int H, int W, int maxlab, int* __restrict__ g) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= W) return;
  const int64_t base = (int64_t)blockIdx.y * H * W + x;
  int prev = 0, d = G_NONE;
  for (int y = 0; y < H; ++y) {   // down: the nearest other label above
    const int l = lab_in(labels[base + (int64_t)y * W], maxlab);
    if (y > 0 && l != prev) d = 1;
    else if (d < G_NONE) ++d;
    g[base + (int64_t)y * W] = d;
    prev = l;
  }
  d = G_NONE;
  for (int y = H - 1; y >= 0; --y) {   // up: the nearest other label below; keep the smaller
    const int l = lab_in(labels[base + (int64_t)y * W], maxlab);
    if (y < H - 1 && l != prev) d = 1;
    else if (d < G_NONE) ++d;
    const int64_t i = base + (int64_t)y * W;
    if (d < g[i]) g[i] = d;
    prev = l;
  }
}

// (2) rows: workgroup = row blockIdx.x of image blockIdx.y; LDS: labels [W], g^2 [W]
__global__ __launch_bounds__(SP_THREADS) void dt_row_kernel(const int* __restrict__ labels, const int* __restrict__ g, int W, int maxlab,
                                                            int* __restrict__ d2) {
  extern __shared__ int sp_row[];
  int* sl = sp_row;
  int* sc = sp_row + W;
  const int64_t row = ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * W;
  for (int x = threadIdx.x; x < W; x += SP_THREADS) {
    const int v = g[row + x];
    sl[x] = lab_in(labels[row + x], maxlab);
    sc[x] = v * v;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += SP_THREADS) {
    const int L = sl[x];
    int best = 0;
    if (L != 0) {
      best = sc[x];
      for (int dx = 1;; ++dx) {   // outward from x; no x' farther than sqrt(best) can improve it
        const int dd = dx * dx, xl = x - dx, xr = x + dx;
        if (dd >= best || (xl < 0 && xr >= W)) break;
        if (xl >= 0) best = min(best, sl[xl] != L ? dd : dd + sc[xl]);
        if (xr < W) best = min(best, sl[xr] != L ? dd : dd + sc[xr]);
      }
    }
    d2[row + x] = best;
  }
}

// (3) seeds: D2 >= minr2 and no pixel of the same label within Chebyshev distance r has a larger D2 (brute force over the window: the
// label restriction rules a separable max filter out).  Counts the seeds of every (image, label) slot.
__global__ __launch_bounds__(SP_THREADS) void seed_kernel(const int* __restrict__ labels, const int* __restrict__ d2, int H, int W, int maxlab,
                                                          int r, int minr2, unsigned char* __restrict__ seeds, int* __restrict__ cnt) {
  constexpr int MAXP = SP_TILE + 2 * SP_MAX_R;
  __shared__ int sl[MAXP * MAXP];
  __shared__ int sd[MAXP * MAXP];
  const int TP = SP_TILE + 2 * r, tx0 = blockIdx.x * SP_TILE - r, ty0 = blockIdx.y * SP_TILE - r;
  const int64_t HW = (int64_t)H * W, base = (int64_t)blockIdx.z * HW;
  for (int i = threadIdx.x; i < TP * TP; i += SP_THREADS) {
    const int y = ty0 + i / TP, x = tx0 + i % TP;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    sl[i] = in ? lab_in(labels[base + (int64_t)y * W + x], maxlab) : 0;
    sd[i] = in ? d2[base + (int64_t)y * W + x] : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = threadIdx.x + k * SP_THREADS, cy = li / SP_TILE, cx = li % SP_TILE;
    const int y = ty0 + r + cy, x = tx0 + r + cx;
    if (y >= H || x >= W) continue;
    const int ctr = (cy + r) * TP + cx + r, L = sl[ctr], D = sd[ctr];
    bool seed = L != 0 && D >= minr2;
    for (int dy = -r; seed && dy <= r; ++dy)
      for (int dx = -r; dx <= r; ++dx) {
        const int q = ctr + dy * TP + dx;
        if (sl[q] == L && sd[q] > D) {
          seed = false;
          break;
        }
      }
    seeds[base + (int64_t)y * W + x] = seed;
    if (seed) atomicAdd(&cnt[(int64_t)blockIdx.z * (HW + 1) + L], 1);
  }
}

// (4) zone map: Z = the pixel's label when a seed of that label lies within Chebyshev distance h, else 0
__global__ __launch_bounds__(SP_THREADS) void zone_kernel(const int* __restrict__ labels, const unsigned char* __restrict__ seeds, int H, int W,
                                                          int maxlab, int h, int* __restrict__ zone) {
  constexpr int MAXP = SP_TILE + SP_MAX_R;   // h <= SP_MAX_R / 2
  __shared__ int sl[MAXP * MAXP];            // the label of a seed pixel, 0 elsewhere
  const int TP = SP_TILE + 2 * h, tx0 = blockIdx.x * SP_TILE - h, ty0 = blockIdx.y * SP_TILE - h;
  const int64_t HW = (int64_t)H * W, base = (int64_t)blockIdx.z * HW;
  for (int i = threadIdx.x; i < TP * TP; i += SP_THREADS) {
    const int y = ty0 + i / TP, x = tx0 + i % TP;
    const bool in = y >= 0 && y < H && x >= 0 && x < W;
    sl[i] = in && seeds[base + (int64_t)y * W + x] ? lab_in(labels[base + (int64_t)y * W + x], maxlab) : 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int li = threadIdx.x + k * SP_THREADS, cy = li / SP_TILE, cx = li % SP_TILE;
    const int y = ty0 + h + cy, x = tx0 + h + cx;
    if (y >= H || x >= W) continue;
    const int64_t gi = base + (int64_t)y * W + x;
    const int L = lab_in(labels[gi], maxlab), ctr = (cy + h) * TP + cx + h;
    bool near = false;
    for (int dy = -h; L != 0 && !near && dy <= h; ++dy)
      for (int dx = -h; dx <= h; ++dx)
        if (sl[ctr + dy * TP + dx] == L) {
          near = true;
          break;
        }
    zone[gi] = near ? L : 0;
  }
}

// (5a) bucket starts: every slot with seeds takes its run of the seed list (the order of the runs is free); cursor = the run's start
__global__ __launch_bounds__(SP_THREADS) void bucket_kernel(const int* __restrict__ cnt, int64_t nslots, int* __restrict__ total,
                                                            int* __restrict__ cursor) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= nslots) return;
  const int c = cnt[i];
  if (c > 0) cursor[i] = atomicAdd(total, c);
}

// (5b) scatter: a seed pixel appends ((y << 16) | x, D2) to its slot's run (any order: the assignment's tie rule is order-free);
// afterwards cursor = the run's end
__global__ __launch_bounds__(SP_THREADS) void scatter_kernel(const int* __restrict__ labels, const int* __restrict__ d2,
                                                             const unsigned char* __restrict__ seeds, int W, int64_t HW, int maxlab,
                                                             int* __restrict__ cursor, int2* __restrict__ list) {
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (i >= HW) return;
  const int64_t gi = (int64_t)blockIdx.y * HW + i;
  if (!seeds[gi]) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  const int pos = atomicAdd(&cursor[(int64_t)blockIdx.y * (HW + 1) + lab_in(labels[gi], maxlab)], 1);
  list[pos] = make_int2((y << 16) | x, d2[gi]);
}

// index of a provisional object in the first-pixel table: a zone root (a pixel index < n) or, for a component without seeds
// (prov = -2 - slot), n + slot
__device__ __forceinline__ int64_t prov_index(int prov, int64_t n) { return prov >= 0 ? (int64_t)prov : n + (-2 - (int64_t)prov); }

// (6) assignment: workgroup = 256 consecutive pixels of image blockIdx.y.  The labels present are served one at a time (smallest
// first): the label's seeds pass through LDS in chunks of 256 and its pixels keep the seed with the smallest (|p - s|^2 - D2(s),
// (y, x) of s).  prov = the zone root of that seed; a pixel of a seedless component gets -2 - slot, background -1.  Every foreground
// pixel then lowers its provisional object's entry of `first` to its own index.
__global__ __launch_bounds__(SP_THREADS) void assign_kernel(const int* __restrict__ labels, int W, int64_t HW, int64_t n, int maxlab,
                                                            const int* __restrict__ cnt, const int* __restrict__ cursor,
                                                            const int2* __restrict__ list, const int* __restrict__ zroot,
                                                            int* __restrict__ prov, unsigned* __restrict__ first) {
  __shared__ int2 sh[SP_THREADS];
  __shared__ int cur;
  const int tid = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * SP_THREADS + tid, base = (int64_t)blockIdx.y * HW, slot0 = (int64_t)blockIdx.y * (HW + 1);
  const bool in = i < HW;
  const int L = in ? lab_in(labels[base + i], maxlab) : 0;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  bool pending = L != 0 && cnt[slot0 + L] > 0;
  int out = L == 0 ? -1 : (int)(-2 - (slot0 + L));
  while (true) {
    if (tid == 0) cur = INT_MAX;
    __syncthreads();
    if (pending) atomicMin(&cur, L);
    __syncthreads();
    const int l = cur;
    if (l == INT_MAX) break;   // uniform: every thread read the same value
    const int c = cnt[slot0 + l], start = cursor[slot0 + l] - c;
    const bool mine = pending && L == l;
    long long bc = LLONG_MAX;
    int bxy = INT_MAX;
    for (int k0 = 0; k0 < c; k0 += SP_THREADS) {
      __syncthreads();   // the previous chunk, and `cur`, have been read
      if (k0 + tid < c) sh[tid] = list[start + k0 + tid];
      __syncthreads();
      if (mine) {
        const int m = min(SP_THREADS, c - k0);
        for (int j = 0; j < m; ++j) {
          const int2 s = sh[j];
          const long long dy = y - (s.x >> 16), dx = x - (s.x & 0xffff), cost = dy * dy + dx * dx - s.y;
          if (cost < bc || (cost == bc && s.x < bxy)) bc = cost, bxy = s.x;
        }
      }
    }
    if (mine) {
      out = zroot[base + (int64_t)(bxy >> 16) * W + (bxy & 0xffff)];
      pending = false;
    }
  }
  if (!in) return;
  prov[base + i] = out;
  if (out != -1) atomicMin(&first[prov_index(out, n)], (unsigned)(base + i));
}

// (7) every foreground pixel points at the first pixel of its provisional object: the form objects.hip numbers
__global__ __launch_bounds__(SP_THREADS) void point_kernel(const int* __restrict__ prov, const unsigned* __restrict__ first, int64_t n,
                                                           int* __restrict__ P) {
  const int64_t gi = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
  if (gi >= n) return;
  const int p = prov[gi];
  P[gi] = p == -1 ? -1 : (int)first[prov_index(p, n)];
}

bool g_row_lds[64];

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

// D2 of labels into d2 with the column distances in g (n ints of scratch): two launches (declared in objects_common.h: boundary.hip
// runs it on its class planes)
int mgud::distance_transform(mgu_ctx* c, const int32_t* labels, int B, int H, int W, int maxlab, int* g, int32_t* d2, hipStream_t s) {
  const size_t lds = (size_t)W * 8;
  if (lds > 65536) {   // the opt-in is set once per device: for the widest row, not for this call's
    int budget = 0;
    HIPCHK(c, hipDeviceGetAttribute(&budget, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    if (lds > (size_t)budget) return fail(c, MGU_ERR_INVALID, "a row of %d pixels needs %zu bytes of LDS, the device gives one workgroup %d", W, lds, budget);
    HIPCHK(c, ensure_dyn_lds((const void*)dt_row_kernel, std::min((size_t)SP_MAX_DIM * 8, (size_t)budget), g_row_lds));
  }
  hipLaunchKernelGGL(dt_col_kernel, dim3((W + 63) / 64, B), dim3(64), 0, s, labels, H, W, maxlab, g);
  hipLaunchKernelGGL(dt_row_kernel, dim3(H, B), dim3(SP_THREADS), lds, s, labels, g, W, maxlab, d2);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgud::distance_transform_dims(mgu_ctx* c, const char* fn, int B, int H, int W) {
  if (B < 0 || H < 0 || W < 0) return fail(c, MGU_ERR_INVALID, "%s: negative size", fn);
  if (H > SP_MAX_DIM || W > SP_MAX_DIM) return fail(c, MGU_ERR_INVALID, "%s: H and W at most %d", fn, SP_MAX_DIM);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "%s: at most 65535 images per call", fn);
  if ((double)B * ((double)H * W + 1) >= (double)(INT_MAX - 2)) return fail(c, MGU_ERR_INVALID, "%s: B*(H*W+1) must stay below 2^31", fn);
  return MGU_OK;
}

extern "C" {

int mgu_distance_transform(mgu_ctx* c, const int32_t* labels_dev, int B, int H, int W, int32_t* d2_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !d2_dev) return fail(c, MGU_ERR_INVALID, "bad distance_transform args (null pointer)");
  int rc = distance_transform_dims(c, "distance_transform", B, H, W);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const int64_t n = (int64_t)B * H * W;
  if (n == 0) return MGU_OK;
  rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)n * 4);
  if (rc) return rc;
  return distance_transform(c, labels_dev, B, H, W, -1, (int*)c->objws, d2_dev, (hipStream_t)hip_stream);
}

int mgu_split_objects(mgu_ctx* c, const int32_t* labels_dev, int B, int H, int W, int min_distance, int64_t min_radius_sq, int min_area,
                      int32_t* labels_out_dev, int64_t* counts_dev, int64_t* offsets_dev, int32_t* d2_out_dev, uint8_t* seeds_out_dev,
                      void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !labels_out_dev || !counts_dev || !offsets_dev) return fail(c, MGU_ERR_INVALID, "bad split_objects args (null pointer)");
  int rc = distance_transform_dims(c, "split_objects", B, H, W);
  if (rc) return rc;
  if (min_distance < 1 || min_distance > SP_MAX_R) return fail(c, MGU_ERR_INVALID, "split_objects: min_distance %d (1..%d)", min_distance, SP_MAX_R);
  if (min_radius_sq < 1 || min_area < 0) return fail(c, MGU_ERR_INVALID, "split_objects: min_radius_sq must be >= 1 and min_area >= 0");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW, nslots = n + B, nch = cc_chunks(HW);
  if (n == 0) return clear_counts(c, B, counts_dev, offsets_dev, s);
  Carve cv;
  const size_t oG = cv.take((size_t)n * 4);                          // column distances, then the provisional objects
  const size_t oD = d2_out_dev ? 0 : cv.take((size_t)n * 4);
  const size_t oS = seeds_out_dev ? 0 : cv.take((size_t)n);
  const size_t oZ = cv.take((size_t)n * 4);                          // zone map, then the first-pixel pointers
  const size_t oR = cv.take((size_t)n * 4);                          // zone roots
  const size_t oN = cv.take((size_t)(nslots + 1) * 4);               // seeds per slot; the last word is the bucket allocator
  const size_t oU = cv.take((size_t)nslots * 4);                     // bucket cursors
  const size_t oL = cv.take((size_t)n * 8);                          // seed list
  const size_t oF = cv.take((size_t)(n + nslots) * 4);               // first pixel per provisional object
  const size_t oA = min_area > 0 ? cv.take((size_t)n * 4) : 0;
  const size_t oC = cv.take((size_t)nch * B * 4);
  rc = ensure(c, &c->objws, &c->objws_bytes, cv.off + (size_t)nch * B * 8);
  if (rc) return rc;
  char* ws = (char*)c->objws;
  int* g = (int*)(ws + oG);
  int* d2 = d2_out_dev ? d2_out_dev : (int*)(ws + oD);
  unsigned char* seeds = seeds_out_dev ? seeds_out_dev : (unsigned char*)(ws + oS);
  int* zone = (int*)(ws + oZ);
  int* zroot = (int*)(ws + oR);
  int* cnt = (int*)(ws + oN);
  int* cursor = (int*)(ws + oU);
  int2* list = (int2*)(ws + oL);
  unsigned* first = (unsigned*)(ws + oF);
  unsigned* area = min_area > 0 ? (unsigned*)(ws + oA) : nullptr;
  const int maxlab = (int)HW, h = (min_distance + 1) / 2;
  const int minr2 = (int)std::min<int64_t>(min_radius_sq, INT_MAX);

  rc = distance_transform(c, labels_dev, B, H, W, maxlab, g, d2, s);
  if (rc) return rc;
  HIPCHK(c, hipMemsetAsync(cnt, 0, (size_t)(nslots + 1) * 4, s));
  const dim3 tiles((W + SP_TILE - 1) / SP_TILE, (H + SP_TILE - 1) / SP_TILE, B);
  hipLaunchKernelGGL(seed_kernel, tiles, dim3(SP_THREADS), 0, s, labels_dev, d2, H, W, maxlab, min_distance, minr2, seeds, cnt);
  hipLaunchKernelGGL(zone_kernel, tiles, dim3(SP_THREADS), 0, s, labels_dev, seeds, H, W, maxlab, h, zone);
  rc = cc_roots_i32(c, zone, B, H, W, zroot, s);
  if (rc) return rc;
  hipLaunchKernelGGL(bucket_kernel, dim3(grid_for(nslots, SP_THREADS, INT_MAX)), dim3(SP_THREADS), 0, s, cnt, nslots, cnt + nslots,
                     cursor);
  const dim3 runs(grid_for(HW, SP_THREADS, INT_MAX), B);
  hipLaunchKernelGGL(scatter_kernel, runs, dim3(SP_THREADS), 0, s, labels_dev, d2, seeds, W, HW, maxlab, cursor, list);
  HIPCHK(c, hipMemsetAsync(first, 0xff, (size_t)(n + nslots) * 4, s));
  int* prov = g;
  hipLaunchKernelGGL(assign_kernel, runs, dim3(SP_THREADS), 0, s, labels_dev, W, HW, n, maxlab, cnt, cursor, list, zroot, prov, first);
  int* P = zone;
  hipLaunchKernelGGL(point_kernel, dim3(grid_for(n, SP_THREADS, INT_MAX)), dim3(SP_THREADS), 0, s, prov, first, n, P);
  HIPCHK(c, hipGetLastError());
  return cc_number_roots(c, P, area, min_area, B, HW, (int*)(ws + oC), (long long*)(ws + cv.off), labels_out_dev, counts_dev, offsets_dev, s);
}

}  // extern "C"
