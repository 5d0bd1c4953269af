// Helpers shared by the object-level kernel files (objects.hip, shapes.hip, split.hip, instances.hip, clean.hip, boundary.hip): each is
// defined here and nowhere else under csrc/ (tests/test_csrc_helpers.py).  device.h keeps what every kernel file shares.
//   device: wave_by_key | block_exclusive_scan | chunk_sum_scan | the pair table (PairTable, pair_add, degree / pour / place kernels;
//           superpixels.hip shares it with instances.hip) | object_index | objects_recorded | pix_key | foreground_class
//           (clahe.hip takes block_exclusive_scan for the cumulative histogram of a tile)
//   host:   check_pixel_count | clear_counts | distance_transform, distance_transform_dims (declared here, defined in split.hip)
#pragma once
#include <climits>

#include "ctx.h"

namespace mgu {

// ---- wave pre-aggregation ---------------------------------------------------------------------------------------------------------
// Every lane holds one record for `key` (key < 0: nothing to add).  The lanes of a wave that share a key are served together: for up
// to ROUNDS distinct keys the first pending lane is the leader, and the WHOLE wave calls group(k, mine, lead) with k = the leader's
// key, mine = this lane holds k, lead = this lane is the leader -- the callback reduces over the lanes with `mine` and lets the lane
// with `lead` issue one atomic for all of them.  It may use wave_sum, wave_min, wave_max or __ballot, which need every lane of the
// wave: so wave_by_key itself must be reached by the whole wave (never under a per-lane branch; a lane without a record passes a
// negative key), and the callback is called convergently here.  Lanes still pending after ROUNDS keys call single() and add their
// own record directly.  The key keeps the caller's type: a 32-bit key costs one ds_bpermute per round, a 64-bit one two.  Callbacks
// capture by value ([=]; they only read, the adds go through pointers): with nested by-reference captures the compiler still sees
// stack slots when it sizes this loop and unrolls it four times, which doubled stats_kernel and panoptic_kernel.
template <int ROUNDS = 4, typename K, typename G, typename S>
__device__ __forceinline__ void wave_by_key(K key, G&& group, S&& single) {
  const int lane = threadIdx.x & 63;
  bool pending = key >= 0;
  for (int it = 0; it < ROUNDS; ++it) {
    const unsigned long long act = __ballot(pending);
    if (!act) break;
    const int leader = __ffsll((long long)act) - 1;
    const K k = __shfl(key, leader);
    const bool mine = pending && key == k;
    group(k, mine, lane == leader);
    if (mine) pending = false;
  }
  if (pending) single();
}

// ---- scans ------------------------------------------------------------------------------------------------------------------------
// exclusive prefix sum over a 256-thread workgroup; *total gets the sum (sh: 4 ints)
__device__ __forceinline__ int block_exclusive_scan(int v, int* sh, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const int u = __shfl_up(inc, off);
    if (lane >= off) inc += u;
  }
  if (lane == 63) sh[wave] = inc;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += sh[w];
  *total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return before + inc - v;
}

// One workgroup of SCAN_THREADS threads scans the n sums the chunk kernels left in cnt: choff[k] = cnt[0] + ... + cnt[k - 1].  A
// thread sums its segment of consecutive chunks, an inclusive Hillis-Steele scan over the segment sums gives every segment its
// start, and the thread walks its segment again.  Every thread gets the grand total; a caller that reads choff entries of other
// threads puts a __syncthreads() first.
constexpr int SCAN_THREADS = 1024;
__device__ __forceinline__ long long chunk_sum_scan(const int* __restrict__ cnt, int64_t n, long long* __restrict__ choff) {
  __shared__ long long sh[SCAN_THREADS];
  const int tid = threadIdx.x;
  const int64_t seg = (n + SCAN_THREADS - 1) / SCAN_THREADS;
  const int64_t k0 = tid * seg < n ? tid * seg : n, k1 = k0 + seg < n ? k0 + seg : n;
  long long s = 0;
  for (int64_t k = k0; k < k1; ++k) s += cnt[k];
  sh[tid] = s;
  __syncthreads();
  for (int off = 1; off < SCAN_THREADS; off <<= 1) {
    const long long u = tid >= off ? sh[tid - off] : 0;
    __syncthreads();
    sh[tid] += u;
    __syncthreads();
  }
  long long run = sh[tid] - s;
  for (int64_t k = k0; k < k1; ++k) {
    choff[k] = run;
    run += cnt[k];
  }
  return sh[SCAN_THREADS - 1];
}

// ---- the pair table: (row, column) pairs with a count, poured into a CSR with ascending columns -----------------------------------
// instances.hip (predicted object x GT object, shared pixels) and superpixels.hip (region x region, shared pixel edges) build their
// sparse tables the same way: (1) their counting kernel calls pair_add(row << 32 | column, count) into an open-addressing hash table
// in global scratch (64-bit compare-and-swap insert; the winner bumps the row's degree), (2) degree_count_kernel, a scan kernel of
// the caller's (chunk_sum_scan plus its own status bits) and degree_write_kernel turn the degrees into the row pointers, (3)
// pair_pour_kernel pours the occupied slots into their rows in whatever order the atomics land in, (4) pair_place_kernel stores every
// entry at its rank inside its row (the number of smaller columns).  The slot of a pair varies from run to run; the outputs do not.
// PTR is the row pointers' type, OUT the type of the column and count arrays.  The kernels are templates so that both files can
// instantiate them from this one definition.
constexpr int PAIR_THREADS = 256;
constexpr int PAIR_ROWCHUNK = 4 * PAIR_THREADS;      // degree scan: 1024 consecutive rows per workgroup
constexpr unsigned long long PAIR_EMPTY = ~0ull;     // a free slot; no pair has this key (both indices stay below 2^31)

struct PairTable {
  unsigned long long* keys;   // slots
  unsigned* cnt;              // slots: the pair's count (B*H*W < 2^31 pixels or 2*B*H*W pixel edges: 32 bits hold any count)
  int* deg;                   // rows: distinct columns met by a row; nullptr: degrees are not kept (no CSR is built of the table)
  unsigned slots;
  int64_t rows;
};

// the slot a key starts probing at: a 64-bit finaliser, then a multiply-shift onto [0, slots)
__device__ __forceinline__ unsigned home_slot(unsigned long long k, unsigned slots) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)(((k & 0xffffffffull) * slots) >> 32);
}

// add c to the pair `key`: linear probing; the table has more than twice as many slots as there can be pairs, so a free slot
// is always met (the probe count is bounded all the same)
__device__ __forceinline__ void pair_add(const PairTable& t, unsigned long long key, unsigned c) {
  unsigned s = home_slot(key, t.slots);
  for (unsigned probe = 0; probe < t.slots; ++probe) {
    unsigned long long k = __hip_atomic_load(&t.keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (k == PAIR_EMPTY) {
      k = atomicCAS(&t.keys[s], PAIR_EMPTY, key);
      if (k == PAIR_EMPTY) {
        if (t.deg) atomicAdd(&t.deg[key >> 32], 1);
        k = key;
      }
    }
    if (k == key) {
      atomicAdd(&t.cnt[s], c);
      return;
    }
    s = s + 1 == t.slots ? 0 : s + 1;
  }
}

// (2a) degrees per chunk of PAIR_ROWCHUNK rows; rows past the table's (no row can have them) have degree 0
template <int UNUSED = 0>
__global__ __launch_bounds__(PAIR_THREADS) void degree_count_kernel(const int* __restrict__ deg, int64_t rows, int* __restrict__ csum) {
  __shared__ int sh[4];
  const int64_t i0 = (int64_t)blockIdx.x * PAIR_ROWCHUNK + 4 * threadIdx.x;
  int c = 0;
  for (int k = 0; k < 4; ++k)
    if (i0 + k < rows) c += deg[i0 + k];
  int total;
  block_exclusive_scan(c, sh, &total);
  if (threadIdx.x == 0) csum[blockIdx.x] = total;
}

// (2c) ptr[i], i in [0, nptr): the chunk's offset plus the exclusive scan inside the chunk
template <typename PTR>
__global__ __launch_bounds__(PAIR_THREADS) void degree_write_kernel(const int* __restrict__ deg, int64_t rows, int64_t nptr,
                                                                    const long long* __restrict__ choff, PTR* __restrict__ ptr) {
  __shared__ int sh[4];
  const int64_t i0 = (int64_t)blockIdx.x * PAIR_ROWCHUNK + 4 * threadIdx.x;
  int d[4], c = 0;
  for (int k = 0; k < 4; ++k) {
    d[k] = i0 + k < rows ? deg[i0 + k] : 0;
    c += d[k];
  }
  int total;
  long long at = choff[blockIdx.x] + block_exclusive_scan(c, sh, &total);
  for (int k = 0; k < 4; ++k) {
    if (i0 + k < nptr) ptr[i0 + k] = (PTR)at;
    at += d[k];
  }
}

// (3) every occupied slot takes the next free place of its row (the row's degree counts down: its final value is 0)
template <typename PTR>
__global__ __launch_bounds__(PAIR_THREADS) void pair_pour_kernel(PairTable t, const PTR* __restrict__ ptr, int* __restrict__ tp,
                                                                 unsigned* __restrict__ tg, unsigned* __restrict__ tc) {
  for (int64_t s = (int64_t)blockIdx.x * PAIR_THREADS + threadIdx.x; s < t.slots; s += (int64_t)gridDim.x * PAIR_THREADS) {
    const unsigned long long k = t.keys[s];
    if (k == PAIR_EMPTY) continue;
    const int p = (int)(k >> 32);
    const long long e = (long long)ptr[p] + atomicSub(&t.deg[p], 1) - 1;
    tp[e] = p, tg[e] = (unsigned)k, tc[e] = t.cnt[s];
  }
}

// (4) entry e of row p goes to the row's place number |{entries of the row with a smaller column}|; places past cap are dropped
template <typename PTR, typename OUT>
__global__ __launch_bounds__(PAIR_THREADS) void pair_place_kernel(const long long* __restrict__ total, const PTR* __restrict__ ptr,
                                                                  const int* __restrict__ tp, const unsigned* __restrict__ tg,
                                                                  const unsigned* __restrict__ tc, int64_t cap, OUT* __restrict__ out_col,
                                                                  OUT* __restrict__ out_cnt) {
  const long long n = *total;
  for (long long e = (long long)blockIdx.x * PAIR_THREADS + threadIdx.x; e < n; e += (long long)gridDim.x * PAIR_THREADS) {
    const int p = tp[e];
    const unsigned g = tg[e];
    const long long r0 = ptr[p], r1 = ptr[p + 1];
    long long at = r0;
    for (long long j = r0; j < r1; ++j) at += tg[j] < g;
    if (at < cap) out_col[at] = (OUT)g, out_cnt[at] = (OUT)tc[e];
  }
}

// ---- the per-object arrays --------------------------------------------------------------------------------------------------------
// row of the per-object arrays of a pixel of image b holding label `lab`: offsets[b] + lab - 1; -1 on background and for an object
// past the arrays' capacity (it was not recorded)
__device__ __forceinline__ long long object_index(int lab, const long long* __restrict__ offsets, int64_t b, int64_t cap) {
  const long long o = lab > 0 ? offsets[b] + lab - 1 : -1;
  return o < cap ? o : -1;
}
// rows of the per-object arrays in use: every object of the batch, or as many as the arrays hold
__device__ __forceinline__ int64_t objects_recorded(const long long* __restrict__ offsets, int B, int64_t cap) {
  return offsets[B] < cap ? offsets[B] : cap;
}

// ---- the value of a pixel ---------------------------------------------------------------------------------------------------------
// value of pixel g: the class map's entry (KIND 0 int64; 2 int32, the internal form of split.hip's zone map; 3 uint8, the internal
// form of clean.hip's class maps), or the first maximal class of the logits (KIND 1, bit-identical to argmax_kernel)
template <int KIND>
__device__ __forceinline__ long long pix_key(const void* src, int64_t g, int C) {
  if constexpr (KIND == 0) {
    return reinterpret_cast<const long long*>(src)[g];
  } else if constexpr (KIND == 2) {
    return reinterpret_cast<const int*>(src)[g];
  } else if constexpr (KIND == 3) {
    return reinterpret_cast<const unsigned char*>(src)[g];
  } else {
    const float* p = reinterpret_cast<const float*>(src) + g * C;
    float best = p[0];
    int bi = 0;
    for (int c = 1; c < C; ++c)
      if (p[c] > best) {
        best = p[c];
        bi = c;
      }
    return bi;
  }
}

// a foreground class 1..ncls-1 of clean.hip and boundary.hip, or 0 (background, -100, out of range)
__device__ __forceinline__ int foreground_class(long long v, int ncls) { return (v >= 1 && v < ncls) ? (int)v : 0; }

}  // namespace mgu

namespace mgud {

// the kernels index pixels with 32-bit integers; fn: the entry point's name as its messages spell it
inline int check_pixel_count(mgu_ctx* c, const char* fn, int B, int H, int W) {
  if ((double)B * H * W >= (double)INT_MAX) return fail(c, MGU_ERR_INVALID, "%s: B*H*W must stay below 2^31", fn);
  return MGU_OK;
}
// split.hip's exact squared distance transform, shared with boundary.hip: D2 of an int32 label map (B, H, W) into d2 (MGU_D2_NONE where
// an image holds no other label, 0 on label 0), with the column distances in g (B*H*W ints of scratch): two launches.  maxlab >= 0
// reads a label outside [0, maxlab] as 0; -1 takes every int32 label.  distance_transform_dims checks what its kernels need of the
// sizes: H, W <= 16384, B <= 65535, B*(H*W+1) < 2^31.
int distance_transform(mgu_ctx* c, const int32_t* labels, int B, int H, int W, int maxlab, int* g, int32_t* d2, hipStream_t s);
int distance_transform_dims(mgu_ctx* c, const char* fn, int B, int H, int W);
// a batch without pixels: every count and offset is 0
inline int clear_counts(mgu_ctx* c, int B, int64_t* counts, int64_t* offsets, hipStream_t s) {
  HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)B * sizeof(int64_t), s));
  HIPCHK(c, hipMemsetAsync(offsets, 0, (size_t)(B + 1) * sizeof(int64_t), s));
  return MGU_OK;
}

}  // namespace mgud
