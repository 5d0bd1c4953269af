// Masks in and out of the device: the dense int32 label map (B, H, W) of objects.hip / split.hip against the two forms annotations
// and result files use -- run lengths in COCO's column-major order and closed polygons on the pixel grid.
//   mgu_mask_runs            label map -> run table, CSR by object (run_ptr, run_start, run_length); position p = x * H + y
//   mgu_runs_to_labels       run table -> label map; where objects overlap the largest label wins (integer atomicMax)
//   mgu_object_outlines      label map -> the closed crack-edge loops of every object: loop_ptr, vertex_ptr, vertices, loop_area2
//   mgu_polygons_to_labels   loops (that layout, fixed-point corners) -> label map: even-odd over the loops of an object, tested at
//                            pixel centres, exact in int64; the largest label wins
// All four are integer definitions ("Masks in and out") held bitwise equal to tests/maskio_oracle.py.  No atomic
// decides a position or an order: places come from exclusive scans and from a stable radix sort; the atomics are integer add (per-row
// counts, shoelace sums) and max (painting), whose results do not depend on arrival order.  No kernel waits for another workgroup.
//
// Shared machinery of this file:
//   compaction  count per chunk -> chunk_scan_kernel (chunk_sum_scan, objects_common.h) -> write at the scanned place: 3 launches
//   counts_to_ptr  per-row counts -> int64 row pointers with the degree kernels of objects_common.h: 3 launches
//   sort_pairs  stable LSD radix sort of (64-bit key, int payload) over `nbits` key bits, 8 per pass: digit histogram per tile of 1024,
//               one wave per digit row scans along the tiles, scatter by wave ballots per digit bit + mbcnt in (wave, item, lane)
//               order (the scheme of lovasz.hip, here on 64-bit keys): 3 launches per pass, ceil(nbits / 8) passes
// Launches (kernel launches + fills), P(n) = ceil(n / 8), bits(v) = the bits that hold v, N = the object capacity:
//   mgu_mask_runs           9 + 3 P(bits(N - 1))                                   + 1 fill
//   mgu_runs_to_labels      1                                                      + 1 fill
//   mgu_object_outlines     17 + bits(4HW - 1) + 3 P(bits(N - 1) + bits(4HW - 1))  + 4 fills
//   mgu_polygons_to_labels  4 + 3 P(bits(N - 1) + bits(H - 1) + bits(W))           + 1 fill
// They depend on H, W and the arguments, never on the data or on B.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int MT = 256;            // threads of every workgroup here
constexpr int CHUNK = 4 * MT;      // compaction: 4 consecutive items per thread
constexpr int TILE = 1024;         // sort: items per workgroup, 256 consecutive ones per wave
constexpr int BINS = 256;

// the object of a pixel of image b: batch-wide row, or -1 (background, a label outside [1, n_b], a row past the capacity)
__device__ __forceinline__ int pixel_object(int lab, const long long* __restrict__ off, int64_t b, int64_t cap) {
  if (lab < 1 || lab > off[b + 1] - off[b]) return -1;
  return (int)object_index(lab, off, b, cap);
}

// the last k in [0, n) with a[k] <= v (a ascending, a[0] <= v): the row of a CSR pointer array that holds entry v
__device__ __forceinline__ long long row_of(const long long* __restrict__ a, long long n, long long v) {
  long long lo = 0, hi = n;   // a[lo] <= v < a[hi] (a[n] taken as +inf)
  while (hi - lo > 1) {
    const long long mid = lo + (hi - lo) / 2;
    if (a[mid] <= v) lo = mid;
    else hi = mid;
  }
  return lo;
}

// total of a compaction or of row counts: choff[k] = cnt[0] + ... + cnt[k - 1], *total = the sum; a sum past cap sets `bit`
__global__ __launch_bounds__(SCAN_THREADS) void chunk_scan_kernel(const int* __restrict__ cnt, int64_t nch, long long* __restrict__ choff,
                                                                  long long* __restrict__ total, int64_t cap, int* __restrict__ status, int bit) {
  const long long t = chunk_sum_scan(cnt, nch, choff);
  if (threadIdx.x == 0) {
    if (total) *total = t;
    if (bit && t > cap) atomicOr(status, bit);
  }
}

// status bit for objects past the per-object capacity
__global__ void capacity_kernel(const long long* __restrict__ off, int B, int64_t cap, int* __restrict__ status, int bit) {
  if (off[B] > cap) atomicOr(status, bit);
}

// one more row of `key` for every lane that holds one (key < 0: none): lanes of a wave that share a key add once
__device__ __forceinline__ void count_row(int key, int* __restrict__ deg) {
  wave_by_key(
      key,
      [=](int k, bool mine, bool lead) {
        const int c = __popcll(__ballot(mine));
        if (lead) atomicAdd(&deg[k], c);
      },
      [=]() { atomicAdd(&deg[key], 1); });
}

// ---- the radix sort ----------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ long long item_count(const long long* __restrict__ count, int64_t max_items) {
  const long long c = *count;
  return c < max_items ? c : max_items;
}

__global__ __launch_bounds__(MT) void sort_hist_kernel(const unsigned long long* __restrict__ keys, const long long* __restrict__ count,
                                                       int64_t max_items, int shift, int ntiles, int* __restrict__ hist) {
  __shared__ int cnt[BINS];
  cnt[threadIdx.x] = 0;
  __syncthreads();
  const long long R = item_count(count, max_items), j0 = (long long)blockIdx.x * TILE;
  for (int i = 0; i < TILE / MT; ++i) {
    const long long j = j0 + i * MT + threadIdx.x;
    if (j < R) atomicAdd(&cnt[(keys[j] >> shift) & (BINS - 1)], 1);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * ntiles + blockIdx.x] = cnt[threadIdx.x];
}

// one wave per digit: hist[d][0 .. ntiles) becomes its exclusive prefix sums, dtot[d] its sum
__global__ __launch_bounds__(MT) void sort_rowscan_kernel(int* __restrict__ hist, int ntiles, int* __restrict__ dtot) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  int* p = hist + (size_t)row * ntiles;
  int carry = 0;
  for (int base = 0; base < ntiles; base += 64) {
    const int j = base + lane, v = j < ntiles ? p[j] : 0;
    int inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int u = __shfl_up(inc, off);
      if (lane >= off) inc += u;
    }
    if (j < ntiles) p[j] = carry + inc - v;
    carry += __shfl(inc, 63);
  }
  if (lane == 0) dtot[row] = carry;
}

// an item goes to (start of its digit) + (items of the digit in the tiles before) + (those before it in this tile): the order inside
// a tile is wave, item, lane -- the order of the input, so the sort is stable
__global__ __launch_bounds__(MT) void sort_scatter_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ pay,
                                                          const long long* __restrict__ count, int64_t max_items, int shift, int ntiles,
                                                          const int* __restrict__ hist, const int* __restrict__ dtot,
                                                          unsigned long long* __restrict__ keys_out, int* __restrict__ pay_out) {
  constexpr int ITEMS = TILE / MT;
  __shared__ int cnt[4 * BINS];
  __shared__ int shs[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int total;
  const int dstart = block_exclusive_scan(dtot[threadIdx.x], shs, &total);
  for (int d = threadIdx.x; d < 4 * BINS; d += MT) cnt[d] = 0;
  __syncthreads();
  const long long R = item_count(count, max_items), j0 = (long long)blockIdx.x * TILE + wave * (ITEMS * 64);
  int* mine = cnt + wave * BINS;
  unsigned long long key[ITEMS];
  int val[ITEMS], rank[ITEMS];
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const long long j = j0 + i * 64 + lane;
    const bool valid = j < R;
    key[i] = valid ? keys[j] : 0ull;
    val[i] = valid ? pay[j] : 0;
    const unsigned d = (unsigned)(key[i] >> shift) & (BINS - 1);
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1;
      const unsigned long long s = __ballot(bit);
      m &= bit ? s : ~s;
    }
    const int below = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    int old = 0;
    if (valid && below == 0) {   // the first lane of a digit takes the digit's next places of this wave for all of them
      old = mine[d];
      mine[d] = old + __popcll(m);
    }
    old = __shfl(old, valid ? __ffsll((long long)m) - 1 : lane);
    rank[i] = old + below;
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  {
    const int d = threadIdx.x;
    int o = dstart + hist[(size_t)d * ntiles + blockIdx.x];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int v = cnt[w * BINS + d];
      cnt[w * BINS + d] = o;
      o += v;
    }
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < ITEMS; ++i) {
    const long long j = j0 + i * 64 + lane;
    if (j < R) {
      const long long pos = mine[(unsigned)(key[i] >> shift) & (BINS - 1)] + rank[i];
      if (pos >= 0 && pos < R) keys_out[pos] = key[i], pay_out[pos] = val[i];   // always, for a histogram of these very keys
    }
  }
}

// ---- painting ----------------------------------------------------------------------------------------------------------------------
// Every lane may hold one stretch of `len` pixels of image b, all taking label k: MODE 0 the column-major positions first .. (a run),
// MODE 1 the row-major ones (a span of a row).  A lane paints the first SHORT pixels itself; a longer stretch is then painted by the
// whole wave.  Reached by every lane of the wave.
template <int MODE>
__device__ __forceinline__ void paint_pixel(int* __restrict__ lab, int64_t base, int p, int H, int W, int k) {
  const int64_t at = MODE == 0 ? base + (int64_t)(p % H) * W + p / H : base + p;
  atomicMax(&lab[at], k);
}
template <int MODE>
__device__ __forceinline__ void wave_paint(int* __restrict__ lab, bool valid, int b, int first, int len, int k, int H, int W) {
  constexpr int SHORT = 4;
  const int lane = threadIdx.x & 63;
  const int64_t HW = (int64_t)H * W;
  if (valid)
    for (int q = 0; q < len && q < SHORT; ++q) paint_pixel<MODE>(lab, b * HW, first + q, H, W, k);
  unsigned long long m = __ballot(valid && len > SHORT);
  while (m) {
    const int l = __ffsll((long long)m) - 1;
    m &= m - 1;
    const int lb = __shfl(b, l), lf = __shfl(first, l), ll = __shfl(len, l), lk = __shfl(k, l);
    for (int q = SHORT + lane; q < ll; q += 64) paint_pixel<MODE>(lab, lb * HW, lf + q, H, W, lk);
  }
}

// ---- 1. runs -----------------------------------------------------------------------------------------------------------------------
// col[b * HW + x * H + y] = the object of pixel (x, y) of image b: the map in COCO's order, through a 32 x 32 tile in LDS
__global__ __launch_bounds__(MT) void columns_kernel(const int* __restrict__ lab, int H, int W, const long long* __restrict__ off, int64_t cap,
                                                     int* __restrict__ col) {
  __shared__ int tile[32][33];
  const int b = blockIdx.z, x0 = blockIdx.x * 32, y0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int64_t base = (int64_t)b * H * W;
  for (int k = ty; k < 32; k += 8) {
    const int x = x0 + tx, y = y0 + k;
    tile[k][tx] = (x < W && y < H) ? pixel_object(lab[base + (int64_t)y * W + x], off, b, cap) : -1;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int x = x0 + k, y = y0 + tx;
    if (x < W && y < H) col[base + (int64_t)x * H + y] = tile[tx][k];
  }
}

// position g of the flat column-major batch: its object, whether a run starts and whether one ends there.  Objects of two images
// differ, so a run never joins two images.
__device__ __forceinline__ void run_flags(const int* __restrict__ col, int64_t n, int64_t g, int& v, bool& st, bool& en) {
  v = g < n ? col[g] : -1;
  st = v >= 0 && (g == 0 || col[g - 1] != v);
  en = v >= 0 && (g == n - 1 || col[g + 1] != v);
}

__global__ __launch_bounds__(MT) void run_count_kernel(const int* __restrict__ col, int64_t n, int* __restrict__ cnt) {
  __shared__ int sh[4];
  const int64_t g0 = (int64_t)blockIdx.x * CHUNK + 4 * threadIdx.x;
  int c = 0;
  for (int j = 0; j < 4; ++j) {
    int v;
    bool st, en;
    run_flags(col, n, g0 + j, v, st, en);
    c += st;
  }
  int total;
  block_exclusive_scan(c, sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// the r-th run in position order: key = object << 32 | start, payload = its last position (the r-th end belongs to the r-th start)
__global__ __launch_bounds__(MT) void run_write_kernel(const int* __restrict__ col, int64_t n, int64_t HW, const long long* __restrict__ choff,
                                                       unsigned long long* __restrict__ keys, int* __restrict__ last, int* __restrict__ deg) {
  __shared__ int sh[4];
  const int64_t g0 = (int64_t)blockIdx.x * CHUNK + 4 * threadIdx.x;
  int v[4], c = 0;
  bool st[4], en[4];
  for (int j = 0; j < 4; ++j) {
    run_flags(col, n, g0 + j, v[j], st[j], en[j]);
    c += st[j];
  }
  int total;
  long long at = choff[blockIdx.x] + block_exclusive_scan(c, sh, &total);
  for (int j = 0; j < 4; ++j) {
    const int p = (int)((g0 + j) % HW);
    if (st[j]) keys[at] = ((unsigned long long)(unsigned)v[j] << 32) | (unsigned)p;
    at += st[j];
    if (en[j]) last[at - 1] = p;
    count_row(st[j] ? v[j] : -1, deg);
  }
}

__global__ __launch_bounds__(MT) void run_finish_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ last,
                                                        const long long* __restrict__ count, int64_t cap, int* __restrict__ run_start,
                                                        int* __restrict__ run_length) {
  const long long R = item_count(count, cap);
  for (long long j = (long long)blockIdx.x * MT + threadIdx.x; j < R; j += (long long)gridDim.x * MT) {
    const int start = (int)(unsigned)keys[j];
    run_start[j] = start, run_length[j] = last[j] - start + 1;
  }
}

// ---- 2. runs -> labels -------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MT) void run_paint_kernel(const long long* __restrict__ run_ptr, const int* __restrict__ run_start,
                                                       const int* __restrict__ run_length, int64_t run_cap, const long long* __restrict__ off,
                                                       int64_t N, int B, int H, int W, int* __restrict__ lab, int* __restrict__ status) {
  const int lane = threadIdx.x & 63;
  const long long HW = (long long)H * W, all = run_ptr[N], R = all < run_cap ? all : run_cap;
  const long long wave = (long long)blockIdx.x * (MT / 64) + (threadIdx.x >> 6), waves = (long long)gridDim.x * (MT / 64);
  if (all > run_cap && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, 4);
  for (long long j0 = wave * 64; j0 < R; j0 += waves * 64) {   // uniform over the wave
    const long long j = j0 + lane;
    bool valid = j < R;
    int b = 0, first = 0, len = 0, k = 0;
    if (valid) {
      const long long i = row_of(run_ptr, N, j);
      first = run_start[j], len = run_length[j];
      if (i >= off[B] || i < off[0]) {
        atomicOr(status, 2), valid = false;
      } else {
        b = (int)row_of(off, B, i);
        k = (int)(i - off[b] + 1);
        if (first < 0 || len < 1 || (long long)first + len > HW) atomicOr(status, 1), valid = false;
      }
    }
    wave_paint<0>(lab, valid, b, first, len, k, H, W);
  }
}

// ---- 3. outlines -------------------------------------------------------------------------------------------------------------------
// Sides of pixel (x, y), clockwise on the screen: 0 top, 1 right, 2 bottom, 3 left; side s travels along DX[s], DY[s] with the pixel
// on its right and the pixel across, P + (DY[s], -DX[s]), on its left.  Edge id = (y * W + x) * 4 + s.
__device__ __forceinline__ int side_dx(int s) { return s == 0 ? 1 : s == 2 ? -1 : 0; }
__device__ __forceinline__ int side_dy(int s) { return s == 1 ? 1 : s == 3 ? -1 : 0; }

struct ImageObjects {   // the objects of one image, read with the frame as "no object"
  const int* oi;
  int H, W;
  __device__ __forceinline__ bool is(int x, int y, int v) const {
    return x >= 0 && y >= 0 && x < W && y < H && oi[(int64_t)y * W + x] == v;
  }
};

__global__ __launch_bounds__(MT) void objmap_kernel(const int* __restrict__ lab, int64_t n, int64_t HW, const long long* __restrict__ off, int64_t cap,
                                                    int* __restrict__ oi) {
  const int64_t g = (int64_t)blockIdx.x * MT + threadIdx.x;
  if (g < n) oi[g] = pixel_object(lab[g], off, g / HW, cap);
}

// side s of pixel (x, y) of object v is an outline edge whose predecessor has another direction: a stored vertex.  The predecessor
// keeps the direction iff the pixel behind on the right is v's and the one behind on the left is not.
__device__ __forceinline__ bool is_corner(const ImageObjects& im, int x, int y, int s, int v) {
  const int dx = side_dx(s), dy = side_dy(s), qx = x + dy, qy = y - dx;
  if (im.is(qx, qy, v)) return false;
  return !(im.is(x - dx, y - dy, v) && !im.is(qx - dx, qy - dy, v));
}

__global__ __launch_bounds__(MT) void corner_count_kernel(const int* __restrict__ oi, int64_t n, int H, int W, int* __restrict__ cnt) {
  __shared__ int sh[4];
  const int64_t g = (int64_t)blockIdx.x * MT + threadIdx.x, HW = (int64_t)H * W;
  int c = 0;
  if (g < n && oi[g] >= 0) {
    const int64_t b = g / HW;
    const int r = (int)(g - b * HW), x = r % W, y = r / W;
    const ImageObjects im{oi + b * HW, H, W};
    for (int s = 0; s < 4; ++s) c += is_corner(im, x, y, s, oi[g]);
  }
  int total;
  block_exclusive_scan(c, sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// corner number `at` (ascending edge id over the batch): cedge[at] = its edge, slot[edge] = at
__global__ __launch_bounds__(MT) void corner_write_kernel(const int* __restrict__ oi, int64_t n, int H, int W, const long long* __restrict__ choff,
                                                          int* __restrict__ cedge, int* __restrict__ slot) {
  __shared__ int sh[4];
  const int64_t g = (int64_t)blockIdx.x * MT + threadIdx.x, HW = (int64_t)H * W;
  bool f[4] = {false, false, false, false};
  int c = 0;
  if (g < n && oi[g] >= 0) {
    const int64_t b = g / HW;
    const int r = (int)(g - b * HW), x = r % W, y = r / W;
    const ImageObjects im{oi + b * HW, H, W};
    for (int s = 0; s < 4; ++s) f[s] = is_corner(im, x, y, s, oi[g]), c += f[s];
  }
  int total;
  long long at = choff[blockIdx.x] + block_exclusive_scan(c, sh, &total);
  for (int s = 0; s < 4; ++s)
    if (f[s]) {
      cedge[at] = (int)(g * 4 + s);
      slot[g * 4 + s] = (int)at;
      ++at;
    }
}

// A corner walks its straight segment: at the end point of an edge, with AR / AL the pixels ahead on the right / left,
//   AR not v's: turn right (the next side of the same pixel) -- unless AL is v's and connectivity = 2, which crosses to AL (left turn)
//   AR v's, AL not: straight on (the same side of AR);  both v's: turn left (the previous side of AL)
// nxt = the corner that starts the next segment, seg = the smallest edge id (inside the image) of this segment.
__global__ __launch_bounds__(MT) void corner_walk_kernel(const int* __restrict__ oi, int H, int W, int conn, const long long* __restrict__ ncorn,
                                                         int64_t max_corners, const int* __restrict__ cedge, const int* __restrict__ slot,
                                                         int* __restrict__ nxt, int* __restrict__ seg, int* __restrict__ dist, int* __restrict__ jump) {
  const long long NC = item_count(ncorn, max_corners), c = (long long)blockIdx.x * MT + threadIdx.x;
  if (c >= NC) return;
  const int64_t HW = (int64_t)H * W;
  const int ge = cedge[c], s = ge & 3;
  const int64_t g = ge >> 2, b = g / HW;
  const int r = (int)(g - b * HW), v = oi[g], dx = side_dx(s), dy = side_dy(s);
  const ImageObjects im{oi + b * HW, H, W};
  int x = r % W, y = r / W, lo = r * 4 + s, to;
  for (;;) {
    const int e = (y * W + x) * 4 + s;
    lo = e < lo ? e : lo;
    const bool ar = im.is(x + dx, y + dy, v), al = im.is(x + dx + dy, y + dy - dx, v);
    if (ar && !al) {
      x += dx, y += dy;
      continue;
    }
    if (ar || (al && conn == 2)) to = ((y + dy - dx) * W + x + dx + dy) * 4 + ((s + 3) & 3);
    else to = (y * W + x) * 4 + ((s + 1) & 3);
    break;
  }
  int t = slot[b * HW * 4 + to];
  if (t < 0 || t >= NC) t = (int)c;   // never, for a corner rule that matches the turn rule: the rounds below must stay inside the arrays
  nxt[c] = t, jump[c] = t, seg[c] = lo, dist[c] = 0;
}

// One round of pointer jumping on the corner cycles: (m, d) = the smallest edge id among the segments of the next 2^r corners and
// the distance in corners to the segment that holds it; j = the corner 2^r further.  Ids are unique inside a loop, and a window that
// already covers its loop cannot be improved, so d stays below the loop's length.
__global__ __launch_bounds__(MT) void corner_round_kernel(const long long* __restrict__ ncorn, int64_t max_corners, int step,
                                                          const int* __restrict__ m0, const int* __restrict__ d0, const int* __restrict__ j0,
                                                          int* __restrict__ m1, int* __restrict__ d1, int* __restrict__ j1) {
  const long long NC = item_count(ncorn, max_corners), c = (long long)blockIdx.x * MT + threadIdx.x;
  if (c >= NC) return;
  const int j = j0[c];
  int m = m0[c], d = d0[c];
  if (m0[j] < m) m = m0[j], d = step + d0[j];
  m1[c] = m, d1[c] = d, j1[c] = j0[j];
}

// the loops: one record per corner at distance 0 of its loop's leader (the corner whose segment holds it)
__global__ __launch_bounds__(MT) void loop_count_kernel(const long long* __restrict__ ncorn, int64_t max_corners, const int* __restrict__ dist,
                                                        int* __restrict__ cnt) {
  __shared__ int sh[4];
  const long long NC = item_count(ncorn, max_corners), c0 = (long long)blockIdx.x * CHUNK + 4 * threadIdx.x;
  int c = 0;
  for (int j = 0; j < 4; ++j) c += c0 + j < NC && dist[c0 + j] == 0;
  int total;
  block_exclusive_scan(c, sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}
// key = object << ebits | leader (image-local edge id), payload = that corner
__global__ __launch_bounds__(MT) void loop_write_kernel(const long long* __restrict__ ncorn, int64_t max_corners, const int* __restrict__ dist,
                                                        const int* __restrict__ lead, const int* __restrict__ cedge, const int* __restrict__ oi,
                                                        int ebits, const long long* __restrict__ choff, int64_t max_loops,
                                                        unsigned long long* __restrict__ keys, int* __restrict__ pay) {
  __shared__ int sh[4];
  const long long NC = item_count(ncorn, max_corners), c0 = (long long)blockIdx.x * CHUNK + 4 * threadIdx.x;
  bool f[4];
  int c = 0;
  for (int j = 0; j < 4; ++j) f[j] = c0 + j < NC && dist[c0 + j] == 0, c += f[j];
  int total;
  long long at = choff[blockIdx.x] + block_exclusive_scan(c, sh, &total);
  for (int j = 0; j < 4; ++j)
    if (f[j] && at < max_loops) {   // always: a loop has 4 corners at least
      const unsigned long long v = (unsigned)oi[cedge[c0 + j] >> 2];
      keys[at] = (v << ebits) | (unsigned)lead[c0 + j];
      pay[at] = (int)(c0 + j);
      ++at;
    }
}

// loop l of the sorted list: its corner count, whether its first vertex is the corner after the leader's segment start (the leader
// edge is no corner), and one more loop for its object
__global__ __launch_bounds__(MT) void loop_info_kernel(const long long* __restrict__ nloops, int64_t max_loops, const unsigned long long* __restrict__ keys,
                                                       const int* __restrict__ pay, int ebits, int64_t HW4, const int* __restrict__ cedge,
                                                       const int* __restrict__ nxt, const int* __restrict__ dist, int* __restrict__ len,
                                                       int* __restrict__ later, int* __restrict__ deg) {
  const long long L = item_count(nloops, max_loops), l = (long long)blockIdx.x * MT + threadIdx.x;
  int obj = -1;
  if (l < L) {
    const int c = pay[l];
    len[l] = dist[nxt[c]] + 1;
    later[l] = (int)(keys[l] & ((1ull << ebits) - 1)) != (int)(cedge[c] % HW4);
    obj = (int)(keys[l] >> ebits);
  }
  count_row(obj, deg);
}

// every corner finds its loop (binary search of its key in the sorted list), its place in it, stores its vertex and adds its term of
// the shoelace sum
__global__ __launch_bounds__(MT) void vertex_write_kernel(const long long* __restrict__ ncorn, int64_t max_corners, const long long* __restrict__ nloops,
                                                          int64_t max_loops, const unsigned long long* __restrict__ keys, int ebits, int H, int W,
                                                          const int* __restrict__ oi, const int* __restrict__ cedge, const int* __restrict__ nxt,
                                                          const int* __restrict__ lead, const int* __restrict__ dist, const int* __restrict__ len,
                                                          const int* __restrict__ later, int64_t loop_cap, int64_t vertex_cap,
                                                          const long long* __restrict__ vertex_ptr, int* __restrict__ vertices,
                                                          unsigned long long* __restrict__ area2) {
  const long long NC = item_count(ncorn, max_corners), L = item_count(nloops, max_loops), c = (long long)blockIdx.x * MT + threadIdx.x;
  if (c >= NC || L < 1) return;
  const int64_t HW4 = (int64_t)H * W * 4;
  const unsigned long long key = ((unsigned long long)(unsigned)oi[cedge[c] >> 2] << ebits) | (unsigned)lead[c];
  long long lo = 0, hi = L - 1;   // the first l with keys[l] >= key
  while (lo < hi) {
    const long long mid = lo + (hi - lo) / 2;
    if (keys[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  if (keys[lo] != key || lo >= loop_cap) return;
  const int n = len[lo];
  int r = (n - dist[c]) % n;
  if (later[lo]) r = (r + n - 1) % n;
  int xy[2][2];
  for (int k = 0; k < 2; ++k) {
    const int e = (int)((k ? cedge[nxt[c]] : cedge[c]) % HW4), s = e & 3, p = e >> 2;
    xy[k][0] = p % W + (s == 1 || s == 2), xy[k][1] = p / W + (s == 2 || s == 3);
  }
  atomicAdd(&area2[lo], (unsigned long long)((long long)xy[0][0] * xy[1][1] - (long long)xy[1][0] * xy[0][1]));
  const long long at = vertex_ptr[lo] + r;
  if (at < vertex_cap) vertices[2 * at] = xy[0][0], vertices[2 * at + 1] = xy[0][1];
}

// ---- 4. polygons -> labels ---------------------------------------------------------------------------------------------------------
struct Polygons {
  const long long *loop_ptr, *vertex_ptr, *off;
  const int* vertices;
  int64_t N, loop_cap, vertex_cap;
  int B, H, W, fbits;
};
struct PolyEdge {   // an edge in doubled units, ordered y0 < y1, with the scanlines [ya, yb) it counts for
  long long x0, y0, x1, y1;
  int obj, ya, yb;
};

// the edge that leaves vertex v, or yb = ya = 0: no such vertex, a horizontal or zero-length edge, a loop of no image (bit 2), a
// coordinate out of range (bit 4)
__device__ __forceinline__ PolyEdge poly_edge(const Polygons& P, long long v, int* __restrict__ status) {
  PolyEdge e{0, 0, 0, 0, -1, 0, 0};
  const long long loops = P.loop_ptr[P.N], L = loops < P.loop_cap ? loops : P.loop_cap;
  if (L < 1) return e;
  const long long verts = P.vertex_ptr[L], V = verts < P.vertex_cap ? verts : P.vertex_cap;
  if (v == 0 && (loops > P.loop_cap || verts > P.vertex_cap)) atomicOr(status, 2);
  if (v >= V) return e;
  const long long l = row_of(P.vertex_ptr, L, v), i = row_of(P.loop_ptr, P.N, l);
  if (i >= P.off[P.B] || i < P.off[0]) {
    atomicOr(status, 2);
    return e;
  }
  const long long end = P.vertex_ptr[l + 1] < V ? P.vertex_ptr[l + 1] : V, w0 = v + 1 < end ? v + 1 : P.vertex_ptr[l], w = w0 < 0 || w0 >= V ? v : w0;
  const int ax = P.vertices[2 * v], ay = P.vertices[2 * v + 1], bx = P.vertices[2 * w], by = P.vertices[2 * w + 1];
  constexpr int LIM = 1 << 24;
  if (ax <= -LIM || ax >= LIM || ay <= -LIM || ay >= LIM || bx <= -LIM || bx >= LIM || by <= -LIM || by >= LIM) {
    atomicOr(status, 4);
    return e;
  }
  if (ay == by) return e;
  const bool up = ay < by;
  e.x0 = 2ll * (up ? ax : bx), e.y0 = 2ll * (up ? ay : by), e.x1 = 2ll * (up ? bx : ax), e.y1 = 2ll * (up ? by : ay);
  e.obj = (int)i;
  // scanline y counts iff y0 <= (2y + 1) S < y1, S = 2^fbits: y >= ceil((y0 - S) / 2S), and the same bound of y1 ends the range
  const long long S = 1ll << P.fbits;
  const long long ya = (e.y0 + S - 1) >> (P.fbits + 1), yb = (e.y1 + S - 1) >> (P.fbits + 1);
  e.ya = (int)(ya < 0 ? 0 : ya > P.H ? P.H : ya), e.yb = (int)(yb < 0 ? 0 : yb > P.H ? P.H : yb);
  return e;
}

__global__ __launch_bounds__(MT) void cross_count_kernel(Polygons P, int* __restrict__ cnt, int* __restrict__ status) {
  __shared__ int sh[4];
  const PolyEdge e = poly_edge(P, (long long)blockIdx.x * MT + threadIdx.x, status);
  int total;
  block_exclusive_scan(e.yb - e.ya, sh, &total);
  if (threadIdx.x == 0) cnt[blockIdx.x] = total;
}

// a crossing: key = object << (ybits + xbits) | y << xbits | the first pixel whose centre lies right of the crossing, clamped to
// [0, W]: A = x0 dy + (x1 - x0)(Yc - y0) < (2x + 1) S dy  <=>  x >= ceil(floor(A / (S dy)) / 2)
__global__ __launch_bounds__(MT) void cross_write_kernel(Polygons P, const long long* __restrict__ choff, int64_t cross_cap, int xbits, int ybits,
                                                         unsigned long long* __restrict__ keys, int* __restrict__ status) {
  __shared__ int sh[4];
  const PolyEdge e = poly_edge(P, (long long)blockIdx.x * MT + threadIdx.x, status);
  int total;
  long long at = choff[blockIdx.x] + block_exclusive_scan(e.yb - e.ya, sh, &total);
  const long long S = 1ll << P.fbits, dy = e.y1 - e.y0, D = S * dy;
  for (int y = e.ya; y < e.yb; ++y, ++at) {
    if (at >= cross_cap) break;
    const long long A = e.x0 * dy + (e.x1 - e.x0) * ((2ll * y + 1) * S - e.y0);
    long long fl = A / D;
    if (A % D != 0 && A < 0) --fl;
    long long x = (fl + 1) >> 1;
    x = x < 0 ? 0 : x > P.W ? P.W : x;
    keys[at] = ((unsigned long long)(unsigned)e.obj << (ybits + xbits)) | ((unsigned long long)y << xbits) | (unsigned long long)x;
  }
}

// the crossings of an (object, scanline) are an even number and lie together in the sorted list: every pair (2m, 2m + 1) is a span
__global__ __launch_bounds__(MT) void span_paint_kernel(const unsigned long long* __restrict__ keys, const long long* __restrict__ count, int64_t cross_cap,
                                                        int xbits, int ybits, const long long* __restrict__ off, int B, int H, int W,
                                                        int* __restrict__ lab) {
  const int lane = threadIdx.x & 63;
  const long long E = item_count(count, cross_cap), pairs = E / 2;
  const long long wave = (long long)blockIdx.x * (MT / 64) + (threadIdx.x >> 6), waves = (long long)gridDim.x * (MT / 64);
  for (long long m0 = wave * 64; m0 < pairs; m0 += waves * 64) {   // uniform over the wave
    const long long m = m0 + lane;
    bool valid = m < pairs;
    int b = 0, first = 0, len = 0, k = 0;
    if (valid) {
      const unsigned long long k0 = keys[2 * m], k1 = keys[2 * m + 1];
      const int x0 = (int)(k0 & ((1ull << xbits) - 1)), x1 = (int)(k1 & ((1ull << xbits) - 1));
      const int y = (int)((k0 >> xbits) & ((1ull << ybits) - 1));
      const long long i = (long long)(k0 >> (xbits + ybits));
      valid = (k0 >> xbits) == (k1 >> xbits) && x1 > x0 && x1 <= W && y < H && i < off[B] && i >= off[0];
      if (valid) {
        b = (int)row_of(off, B, i);
        k = (int)(i - off[b] + 1), first = y * W + x0, len = x1 - x0;
      }
    }
    wave_paint<1>(lab, valid, b, first, len, k, H, W);
  }
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

int bits_of(unsigned long long v) {   // the bits that hold v: 0 for 0
  int b = 0;
  while (v) ++b, v >>= 1;
  return b;
}

template <typename... KA, typename... A>
void go(mgu_ctx* c, hipStream_t s, const char* name, void (*kernel)(KA...), dim3 grid, dim3 block, A... args) {
  ProfScope ps(c, s, name);
  hipLaunchKernelGGL(kernel, grid, block, 0, s, (KA)args...);
}

// per-row counts deg[0 .. rows) -> ptr[0 .. nptr) (rows past `rows` are empty); csum / choff: scratch of ceil(nptr / PAIR_ROWCHUNK)
void counts_to_ptr(mgu_ctx* c, hipStream_t s, const char* name, const int* deg, int64_t rows, int64_t nptr, int* csum, long long* choff,
                   long long* ptr) {
  const unsigned nch = (unsigned)((nptr + PAIR_ROWCHUNK - 1) / PAIR_ROWCHUNK);
  go(c, s, name, degree_count_kernel<0>, dim3(nch), dim3(PAIR_THREADS), deg, rows, csum);
  go(c, s, name, chunk_scan_kernel, dim3(1), dim3(SCAN_THREADS), (const int*)csum, (int64_t)nch, choff, (long long*)nullptr, (int64_t)0,
     (int*)nullptr, 0);
  go(c, s, name, degree_write_kernel<long long>, dim3(nch), dim3(PAIR_THREADS), deg, rows, nptr, (const long long*)choff, ptr);
}

struct SortBuf {
  unsigned long long* k[2];
  int* p[2];
  int *hist, *dtot;
};
size_t sort_tiles(int64_t max_items) { return (size_t)std::max<int64_t>(1, (max_items + TILE - 1) / TILE); }
// sorts the *count (at most max_items) pairs of buffer 0 by the nbits key bits from bit lo up; returns the buffer that holds the result
int sort_pairs(mgu_ctx* c, hipStream_t s, const char* name, const SortBuf& sb, const long long* count, int64_t max_items, int lo, int nbits) {
  const int ntiles = (int)sort_tiles(max_items);
  int cur = 0;
  for (int shift = lo; shift < lo + nbits; shift += 8, cur ^= 1) {
    go(c, s, name, sort_hist_kernel, dim3(ntiles), dim3(MT), (const unsigned long long*)sb.k[cur], count, max_items, shift, ntiles, sb.hist);
    go(c, s, name, sort_rowscan_kernel, dim3(BINS / 4), dim3(MT), sb.hist, ntiles, sb.dtot);
    go(c, s, name, sort_scatter_kernel, dim3(ntiles), dim3(MT), (const unsigned long long*)sb.k[cur], (const int*)sb.p[cur], count, max_items,
       shift, ntiles, (const int*)sb.hist, (const int*)sb.dtot, sb.k[cur ^ 1], sb.p[cur ^ 1]);
  }
  return cur;
}
void carve_sort(Carve& cv, int64_t max_items, size_t (&o)[6]) {
  const size_t m = (size_t)std::max<int64_t>(1, max_items);
  o[0] = cv.take(m * 8), o[1] = cv.take(m * 8), o[2] = cv.take(m * 4), o[3] = cv.take(m * 4);
  o[4] = cv.take(sort_tiles(max_items) * BINS * 4), o[5] = cv.take(BINS * 4);
}
SortBuf sort_buf(char* ws, const size_t (&o)[6]) {
  return SortBuf{{(unsigned long long*)(ws + o[0]), (unsigned long long*)(ws + o[1])}, {(int*)(ws + o[2]), (int*)(ws + o[3])}, (int*)(ws + o[4]),
                 (int*)(ws + o[5])};
}

// what all four entry points ask of the sizes; limit: the largest B*H*W (the outlines index 4 edges per pixel with 32 bits)
int check_sizes(mgu_ctx* c, const char* fn, int B, int H, int W, int64_t capacity, double limit) {
  if (B < 0 || H < 0 || W < 0 || capacity < 0) return fail(c, MGU_ERR_INVALID, "bad %s args (negative size)", fn);
  if (int rc = check_pixel_count(c, fn, B, H, W)) return rc;
  if ((double)B * H * W >= limit) return fail(c, MGU_ERR_INVALID, "%s: 4*B*H*W must stay below 2^31", fn);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "%s: at most 65535 images per call", fn);
  if (H > 32768 || W > 32768) return fail(c, MGU_ERR_INVALID, "%s: H and W at most 32768", fn);
  if (capacity >= 2147483647ll) return fail(c, MGU_ERR_INVALID, "%s: capacities must stay below 2^31", fn);
  return MGU_OK;
}

}  // namespace

extern "C" {

int mgu_mask_runs(mgu_ctx* c, const int32_t* labels_dev, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W, int64_t run_capacity,
                  int64_t* run_ptr_dev, int32_t* run_start_dev, int32_t* run_length_dev, int32_t* status_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !offsets_dev || !run_ptr_dev || !status_dev || run_capacity < 0 || (run_capacity > 0 && (!run_start_dev || !run_length_dev)))
    return fail(c, MGU_ERR_INVALID, "bad mask_runs args (null pointer or negative capacity)");
  if (int rc = check_sizes(c, "mask_runs", B, H, W, capacity, 2147483647.0)) return rc;
  if (run_capacity >= 2147483647ll) return fail(c, MGU_ERR_INVALID, "mask_runs: capacities must stay below 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW, nptr = capacity + 1;
  if (n == 0) {
    HIPCHK(c, hipMemsetAsync(run_ptr_dev, 0, (size_t)nptr * 8, s));
    return MGU_OK;
  }
  const int64_t rows = capacity, nch = (n + CHUNK - 1) / CHUNK, dch = (nptr + PAIR_ROWCHUNK - 1) / PAIR_ROWCHUNK;
  Carve cv;
  size_t so[6];
  const size_t oCol = cv.take((size_t)n * 4), oCnt = cv.take((size_t)nch * 4), oOff = cv.take((size_t)nch * 8), oTot = cv.take(8);
  const size_t oDeg = cv.take((size_t)(rows + 1) * 4), oDs = cv.take((size_t)dch * 4), oDo = cv.take((size_t)dch * 8);
  carve_sort(cv, n, so);
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
  char* ws = (char*)c->objws;
  int *col = (int*)(ws + oCol), *cnt = (int*)(ws + oCnt), *deg = (int*)(ws + oDeg), *dsum = (int*)(ws + oDs);
  long long *choff = (long long*)(ws + oOff), *total = (long long*)(ws + oTot), *doff = (long long*)(ws + oDo);
  const SortBuf sb = sort_buf(ws, so);
  const long long* off = (const long long*)offsets_dev;
  HIPCHK(c, hipMemsetAsync(deg, 0, (size_t)(rows + 1) * 4, s));
  go(c, s, "mask_runs columns", columns_kernel, dim3((W + 31) / 32, (H + 31) / 32, B), dim3(MT), labels_dev, H, W, off, capacity, col);
  go(c, s, "mask_runs count", run_count_kernel, dim3((unsigned)nch), dim3(MT), (const int*)col, n, cnt);
  go(c, s, "mask_runs scan", chunk_scan_kernel, dim3(1), dim3(SCAN_THREADS), (const int*)cnt, nch, choff, total, run_capacity, (int*)status_dev, 1);
  go(c, s, "mask_runs write", run_write_kernel, dim3((unsigned)nch), dim3(MT), (const int*)col, n, HW, (const long long*)choff, sb.k[0], sb.p[0], deg);
  counts_to_ptr(c, s, "mask_runs rows", deg, rows, nptr, dsum, doff, (long long*)run_ptr_dev);
  const int at = sort_pairs(c, s, "mask_runs sort", sb, total, n, 32, bits_of(capacity > 0 ? capacity - 1 : 0));
  go(c, s, "mask_runs finish", run_finish_kernel, dim3(grid_for(std::max<int64_t>(run_capacity, 1), MT, 4096)), dim3(MT),
     (const unsigned long long*)sb.k[at], (const int*)sb.p[at], (const long long*)total, run_capacity, run_start_dev, run_length_dev);
  go(c, s, "mask_runs capacity", capacity_kernel, dim3(1), dim3(1), off, B, capacity, (int*)status_dev, 2);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_runs_to_labels(mgu_ctx* c, const int64_t* run_ptr_dev, const int32_t* run_start_dev, const int32_t* run_length_dev, int64_t run_capacity,
                       const int64_t* offsets_dev, int64_t capacity, int B, int H, int W, int32_t* labels_dev, int32_t* status_dev,
                       void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!run_ptr_dev || !offsets_dev || !status_dev || run_capacity < 0 || (run_capacity > 0 && (!run_start_dev || !run_length_dev)))
    return fail(c, MGU_ERR_INVALID, "bad runs_to_labels args (null pointer or negative capacity)");
  if (int rc = check_sizes(c, "runs_to_labels", B, H, W, capacity, 2147483647.0)) return rc;
  const int64_t n = (int64_t)B * H * W;
  if (n > 0 && !labels_dev) return fail(c, MGU_ERR_INVALID, "bad runs_to_labels args (null pointer or negative capacity)");
  if (n == 0) return MGU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  HIPCHK(c, hipMemsetAsync(labels_dev, 0, (size_t)n * 4, s));
  go(c, s, "runs_to_labels paint", run_paint_kernel, dim3(grid_for(std::max<int64_t>(run_capacity, 1), MT, 4096)), dim3(MT),
     (const long long*)run_ptr_dev, run_start_dev, run_length_dev, run_capacity, (const long long*)offsets_dev, capacity, B, H, W, labels_dev,
     (int*)status_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_object_outlines(mgu_ctx* c, const int32_t* labels_dev, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W, int connectivity,
                        int64_t loop_capacity, int64_t vertex_capacity, int64_t* loop_ptr_dev, int64_t* vertex_ptr_dev, int32_t* vertices_dev,
                        int64_t* loop_area2_dev, int32_t* status_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !offsets_dev || !loop_ptr_dev || !vertex_ptr_dev || !status_dev || loop_capacity < 0 || vertex_capacity < 0 ||
      (loop_capacity > 0 && !loop_area2_dev) || (vertex_capacity > 0 && !vertices_dev))
    return fail(c, MGU_ERR_INVALID, "bad object_outlines args (null pointer or negative capacity)");
  if (connectivity != 1 && connectivity != 2) return fail(c, MGU_ERR_INVALID, "object_outlines: connectivity must be 1 or 2");
  if (int rc = check_sizes(c, "object_outlines", B, H, W, capacity, 536870912.0)) return rc;
  if (loop_capacity >= 2147483647ll || vertex_capacity >= 2147483647ll)
    return fail(c, MGU_ERR_INVALID, "object_outlines: capacities must stay below 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW, nptr = capacity + 1, lptr = loop_capacity + 1;
  if (n == 0) {
    HIPCHK(c, hipMemsetAsync(loop_ptr_dev, 0, (size_t)nptr * 8, s));
    HIPCHK(c, hipMemsetAsync(vertex_ptr_dev, 0, (size_t)lptr * 8, s));
    return MGU_OK;
  }
  // at most 4 corners per pixel and 4 corners at least per loop: 4n corners, n loops
  const int64_t maxc = 4 * n, maxl = n, rows = capacity;
  const int64_t pch = (n + MT - 1) / MT, cch = (maxc + CHUNK - 1) / CHUNK, nch = std::max(pch, cch);
  const int64_t dch = (std::max(nptr, lptr) + PAIR_ROWCHUNK - 1) / PAIR_ROWCHUNK;
  const int ebits = bits_of((unsigned long long)(4 * HW - 1)), obits = bits_of(capacity > 0 ? capacity - 1 : 0);
  Carve cv;
  size_t so[6], oR[8];
  const size_t oOi = cv.take((size_t)n * 4), oCnt = cv.take((size_t)nch * 4), oOff = cv.take((size_t)nch * 8), oNc = cv.take(8), oNl = cv.take(8);
  for (size_t& o : oR) o = cv.take((size_t)maxc * 4);   // cedge, nxt, (m, d, j) x 2; the second j starts as the edge -> corner table
  const size_t oLen = cv.take((size_t)maxl * 4), oLat = cv.take((size_t)maxl * 4), oDeg = cv.take((size_t)(rows + 1) * 4);
  const size_t oDs = cv.take((size_t)dch * 4), oDo = cv.take((size_t)dch * 8);
  carve_sort(cv, maxl, so);
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
  char* ws = (char*)c->objws;
  int *oi = (int*)(ws + oOi), *cnt = (int*)(ws + oCnt), *len = (int*)(ws + oLen), *later = (int*)(ws + oLat), *deg = (int*)(ws + oDeg);
  int *dsum = (int*)(ws + oDs), *cedge = (int*)(ws + oR[0]), *nxt = (int*)(ws + oR[1]);
  int* md[2][3] = {{(int*)(ws + oR[2]), (int*)(ws + oR[3]), (int*)(ws + oR[4])}, {(int*)(ws + oR[5]), (int*)(ws + oR[6]), (int*)(ws + oR[7])}};
  int* slot = md[1][2];
  long long *choff = (long long*)(ws + oOff), *ncorn = (long long*)(ws + oNc), *nloops = (long long*)(ws + oNl), *doff = (long long*)(ws + oDo);
  const SortBuf sb = sort_buf(ws, so);
  const long long* off = (const long long*)offsets_dev;
  const char* nm = "object_outlines";
  HIPCHK(c, hipMemsetAsync(slot, 0xFF, (size_t)maxc * 4, s));
  HIPCHK(c, hipMemsetAsync(len, 0, (size_t)maxl * 4, s));
  HIPCHK(c, hipMemsetAsync(deg, 0, (size_t)(rows + 1) * 4, s));
  if (loop_capacity > 0) HIPCHK(c, hipMemsetAsync(loop_area2_dev, 0, (size_t)loop_capacity * 8, s));
  go(c, s, nm, objmap_kernel, dim3((unsigned)pch), dim3(MT), labels_dev, n, HW, off, capacity, oi);
  go(c, s, nm, corner_count_kernel, dim3((unsigned)pch), dim3(MT), (const int*)oi, n, H, W, cnt);
  go(c, s, nm, chunk_scan_kernel, dim3(1), dim3(SCAN_THREADS), (const int*)cnt, pch, choff, ncorn, vertex_capacity, (int*)status_dev, 2);
  go(c, s, nm, corner_write_kernel, dim3((unsigned)pch), dim3(MT), (const int*)oi, n, H, W, (const long long*)choff, cedge, slot);
  const unsigned cblocks = (unsigned)((maxc + MT - 1) / MT);
  go(c, s, nm, corner_walk_kernel, dim3(cblocks), dim3(MT), (const int*)oi, H, W, connectivity, (const long long*)ncorn, maxc, (const int*)cedge,
     (const int*)slot, nxt, md[0][0], md[0][1], md[0][2]);
  int cur = 0;
  for (int r = 0; r < ebits; ++r, cur ^= 1)   // 2^ebits >= 4HW > the corners of a loop
    go(c, s, "object_outlines rounds", corner_round_kernel, dim3(cblocks), dim3(MT), (const long long*)ncorn, maxc, 1 << r, (const int*)md[cur][0],
       (const int*)md[cur][1], (const int*)md[cur][2], md[cur ^ 1][0], md[cur ^ 1][1], md[cur ^ 1][2]);
  const int *lead = md[cur][0], *dist = md[cur][1];
  go(c, s, nm, loop_count_kernel, dim3((unsigned)cch), dim3(MT), (const long long*)ncorn, maxc, dist, cnt);
  go(c, s, nm, chunk_scan_kernel, dim3(1), dim3(SCAN_THREADS), (const int*)cnt, cch, choff, nloops, loop_capacity, (int*)status_dev, 1);
  go(c, s, nm, loop_write_kernel, dim3((unsigned)cch), dim3(MT), (const long long*)ncorn, maxc, dist, lead, (const int*)cedge, (const int*)oi, ebits,
     (const long long*)choff, maxl, sb.k[0], sb.p[0]);
  const int at = sort_pairs(c, s, "object_outlines sort", sb, nloops, maxl, 0, obits + ebits);
  go(c, s, nm, loop_info_kernel, dim3((unsigned)((maxl + MT - 1) / MT)), dim3(MT), (const long long*)nloops, maxl, (const unsigned long long*)sb.k[at],
     (const int*)sb.p[at], ebits, 4 * HW, (const int*)cedge, (const int*)nxt, dist, len, later, deg);
  counts_to_ptr(c, s, nm, deg, rows, nptr, dsum, doff, (long long*)loop_ptr_dev);
  counts_to_ptr(c, s, nm, len, maxl, lptr, dsum, doff, (long long*)vertex_ptr_dev);
  go(c, s, nm, vertex_write_kernel, dim3(cblocks), dim3(MT), (const long long*)ncorn, maxc, (const long long*)nloops, maxl,
     (const unsigned long long*)sb.k[at], ebits, H, W, (const int*)oi, (const int*)cedge, (const int*)nxt, lead, dist, (const int*)len,
     (const int*)later, loop_capacity, vertex_capacity, (const long long*)vertex_ptr_dev, vertices_dev, (unsigned long long*)loop_area2_dev);
  go(c, s, nm, capacity_kernel, dim3(1), dim3(1), off, B, capacity, (int*)status_dev, 4);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_polygons_to_labels(mgu_ctx* c, const int64_t* loop_ptr_dev, const int64_t* vertex_ptr_dev, const int32_t* vertices_dev, int64_t loop_capacity,
                           int64_t vertex_capacity, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W, int frac_bits,
                           int64_t crossing_capacity, int32_t* labels_dev, int32_t* status_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!loop_ptr_dev || !vertex_ptr_dev || !offsets_dev || !status_dev || loop_capacity < 0 || vertex_capacity < 0 || crossing_capacity < 0 ||
      (vertex_capacity > 0 && !vertices_dev))
    return fail(c, MGU_ERR_INVALID, "bad polygons_to_labels args (null pointer or negative capacity)");
  if (frac_bits < 0 || frac_bits > 4) return fail(c, MGU_ERR_INVALID, "polygons_to_labels: frac_bits must be in 0..4");
  if (int rc = check_sizes(c, "polygons_to_labels", B, H, W, capacity, 2147483647.0)) return rc;
  if (loop_capacity >= 2147483647ll || vertex_capacity >= 2147483647ll || crossing_capacity >= 2147483647ll)
    return fail(c, MGU_ERR_INVALID, "polygons_to_labels: capacities must stay below 2^31");
  const int64_t n = (int64_t)B * H * W;
  if (n > 0 && !labels_dev) return fail(c, MGU_ERR_INVALID, "bad polygons_to_labels args (null pointer or negative capacity)");
  if (n == 0) return MGU_OK;
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t vch = std::max<int64_t>(1, (vertex_capacity + MT - 1) / MT), maxx = std::max<int64_t>(crossing_capacity, 1);
  const int xbits = bits_of((unsigned long long)W), ybits = bits_of((unsigned long long)(H - 1)), obits = bits_of(capacity > 0 ? capacity - 1 : 0);
  Carve cv;
  size_t so[6];
  const size_t oCnt = cv.take((size_t)vch * 4), oOff = cv.take((size_t)vch * 8), oTot = cv.take(8);
  carve_sort(cv, maxx, so);
  if (int rc = ensure(c, &c->objws, &c->objws_bytes, cv.off)) return rc;
  char* ws = (char*)c->objws;
  int* cnt = (int*)(ws + oCnt);
  long long *choff = (long long*)(ws + oOff), *total = (long long*)(ws + oTot);
  const SortBuf sb = sort_buf(ws, so);
  const Polygons P{(const long long*)loop_ptr_dev, (const long long*)vertex_ptr_dev, (const long long*)offsets_dev, vertices_dev, capacity,
                   loop_capacity, vertex_capacity, B, H, W, frac_bits};
  const char* nm = "polygons_to_labels";
  HIPCHK(c, hipMemsetAsync(labels_dev, 0, (size_t)n * 4, s));
  go(c, s, nm, cross_count_kernel, dim3((unsigned)vch), dim3(MT), P, cnt, (int*)status_dev);
  go(c, s, nm, chunk_scan_kernel, dim3(1), dim3(SCAN_THREADS), (const int*)cnt, vch, choff, total, crossing_capacity, (int*)status_dev, 1);
  go(c, s, nm, cross_write_kernel, dim3((unsigned)vch), dim3(MT), P, (const long long*)choff, crossing_capacity, xbits, ybits, sb.k[0], (int*)status_dev);
  const int at = sort_pairs(c, s, "polygons_to_labels sort", sb, total, maxx, 0, obits + ybits + xbits);
  go(c, s, nm, span_paint_kernel, dim3(grid_for(maxx, 2 * MT, 4096)), dim3(MT), (const unsigned long long*)sb.k[at], (const long long*)total,
     crossing_capacity, xbits, ybits, (const long long*)offsets_dev, B, H, W, labels_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
