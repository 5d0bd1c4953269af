// Exact binary s-t min cut of the patch graph: the solver of the energy whose parameters MinCutRefinement's constructor takes
// (model/graph_partition/mincut_refinement.py:9-25 documents gamma_unet_priors, sigma_intensity and sigma_features for an E(S) "if a
// solver was used"; the reference implements none).  The energy is this build's definition:
//   E(S) = sum_i D_i(S_i) + lambda sum_{(i,j) undirected} w_ij [S_i != S_j]
//   D_i(fg) = -log p_i, D_i(bg) = -log(1 - p_i), p clamped to [1e-6, 1 - 1e-6]
//   w_ij = exp(-(I_i - I_j)^2 / (2 sigma_I^2)) + gamma exp(-|f_i - f_j|^2 / (2 sigma_f^2))     (a term whose input is absent is dropped)
// quantised to integers, q(x) = min(lrintf(x unit), 2^20), so that the max-flow value and the minimal sink side of the cut are unique
// and every result below is exact and bit-reproducible although the solver uses atomics.
//   mgu_graphcut_rev_index    CSR-by-source position of every COO edge and of its reverse edge; flags a missing reverse edge, a
//                             duplicate edge, a self loop
//   mgu_graphcut_capacities   cap_source = q(D(bg)), cap_sink = q(D(fg)) per node, cap_edge = q(lambda w) per directed edge (COO order,
//                             bitwise symmetric: the squared distances are formed from the lower to the higher node id)
//   mgu_graphcut_solve        phase 1 of push-relabel in lock step, ONE workgroup per graph, the whole residual graph in LDS
//   mgu_graphcut_energy       E of any labelling in capacity units (integer sums: exact)
//   mgu_graphcut_label_costs / mgu_graphcut_expand / mgu_graphcut_energy_multi   the same energy over K labels, minimised by
//                             alpha-expansion: every move is one binary cut by the rounds of mgu_graphcut_solve, the whole loop one launch
// The solver.  LDS per graph: 64-bit excess (N + 1 words, the last one the flow into the sink), residual arc capacities (E, CSR
// order), height, residual sink capacity and one scratch word per node -- 130 KB + 16 KB for the 64 x 64 patch grid (N = 4096,
// E = 16128) of a 1024^2 image, inside gfx950's 160 KiB.  rowptr / col / rev are read-only and stay in global memory (L2).  A round is
//   snapshot   every active node (excess > 0, height < N + 1) records min(excess, 2^31 - 1); no active node: converged
//   push       heights frozen: to the sink when h == 1, then along the arcs with h[u] == h[v] + 1 in row order.  u -> v and v -> u are
//              never both admissible, so an arc pair has one writer per phase and needs no atomics; the excess of v is raised by
//              several neighbours at once: 64-bit LDS atomic adds (4096 source arcs of 2^20 exceed 2^31)
//   relabel    a node still holding excess takes min over its residual arcs of h[v] + 1 (1 with residual sink capacity, else N + 1),
//              computed from the frozen heights into the scratch word, then committed: deterministic
// and every `period` rounds the heights are replaced by the exact residual distances to the sink (reverse BFS as a relaxation to a
// fixed point: the result does not depend on the order of the sweeps).  The height that stands for "cannot reach the sink" is N + 1: a
// path through all N nodes has distance N.  After the last round the same BFS gives the labels: 1 (foreground, source side) iff the
// sink is NOT reachable in the residual graph.  That set is the same for every maximum preflow, so ties between equal-cost cuts
// always resolve to the largest foreground.
// Every loop is bounded (rounds <= max_rounds, BFS sweeps <= N), the only synchronisation is __syncthreads() inside the workgroup, and
// the capacity arrays handed in are never written: a graph that does not converge ends with converged = 0.
#include <limits.h>

#include "ctx.h"

namespace mgu {
namespace {

constexpr int GC_THREADS = 256;
constexpr int GC_CAP_MAX = 1 << 20;
constexpr int GC_WIDE_DEGREE = 4095;   // from this degree on (1 + degree) 2^20 no longer fits the 32-bit residual sink word of a move
// Defaults of the solver, from the measured table in DESIGN.md section 3 (tools/graphcut_bench.py): at N = 1024 and N = 4096 the largest
// workgroup and a period of 32 rounds (against 2 .. 16 and 64) were fastest.  Smaller graphs get one thread per node, and a period of about sqrt(N)
// rounds -- the sweeps of one global relabel on a grid -- so that a 5 x 7 graph does not wait 32 rounds for its second relabel.
constexpr int GC_MAX_THREADS = 1024;
constexpr int GC_MAX_PERIOD = 32;
inline int gc_default_threads(int N) { return std::min(GC_MAX_THREADS, (N + 63) / 64 * 64); }
inline int gc_default_period(int N) {
  int s = 1;
  while ((int64_t)(s + 1) * (s + 1) <= N) ++s;   // floor(sqrt(N))
  return std::max(4, std::min(GC_MAX_PERIOD, s));
}

// ---- reverse-edge index ---------------------------------------------------------------------------------------------------------
// one thread per COO edge k = (u -> v): p = its position in row u of the CSR by source, perm[p] = k, rev[p] = position of (v -> u)
__global__ __launch_bounds__(GC_THREADS) void graphcut_rev_kernel(const int64_t* __restrict__ coo, int64_t E, int N, const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ col, int32_t* __restrict__ rev,
                                                                  int32_t* __restrict__ perm, int* __restrict__ status) {
  const int64_t k = blockIdx.x * (int64_t)GC_THREADS + threadIdx.x;
  if (k >= E) return;
  const int64_t u = coo[k], v = coo[E + k];
  if (u < 0 || u >= N || v < 0 || v >= N) {
    atomicOr(status, 8);
    return;
  }
  if (u == v) atomicOr(status, 4);
  if (rowptr[u + 1] - rowptr[u] >= GC_WIDE_DEGREE) atomicOr(status, 16);   // not an error: only the multi-label solver refuses it
  int p = -1, q = -1, np = 0;
  for (int i = rowptr[u]; i < rowptr[u + 1]; ++i)
    if (col[i] == (int)v) {
      if (p < 0) p = i;
      ++np;
    }
  for (int i = rowptr[v]; i < rowptr[v + 1]; ++i)
    if (col[i] == (int)u) {
      q = i;
      break;
    }
  if (np != 1) atomicOr(status, p < 0 ? 8 : 2);
  if (q < 0) atomicOr(status, 1);
  if (p >= 0) {
    perm[p] = (int)k;
    rev[p] = q;
  }
}

// ---- energy -> integer capacities -----------------------------------------------------------------------------------------------
__device__ __forceinline__ int gc_quant(float x, float unit) {   // q(x): NaN and negative values give 0
  return (int)lrintf(fminf(fmaxf(x * unit, 0.f), (float)GC_CAP_MAX));
}
// -log x given y = 1 - x, both in [1e-6, 1]: the form that loses nothing near x = 1
__device__ __forceinline__ float gc_neglog(float x, float y) { return x < 0.5f ? -logf(x) : -log1pf(-y); }

struct CapArgs {
  int B, N, C, fg, D;
  int64_t E;
  const int64_t* coo;
  const float* prior;        // (B*N) or NULL
  const int32_t* counts;     // (B*N, C) or NULL
  const float* intensity;    // (B*N) or NULL
  const float* feat;         // (B*N, D) or NULL
  float inv2si, inv2sf, gamma, lambda, unit;
  int32_t *cap_source, *cap_sink, *cap_edge;
};
__global__ __launch_bounds__(GC_THREADS) void graphcut_capacities_kernel(const CapArgs a) {
  const int64_t t = blockIdx.x * (int64_t)GC_THREADS + threadIdx.x, nodes = (int64_t)a.B * a.N;
  if (t < nodes) {
    float p, q;
    if (a.counts) {
      const int32_t* c = a.counts + t * a.C;
      int64_t all = 0;
      for (int j = 0; j < a.C; ++j) all += max(c[j], 0);
      const int64_t fg = max(c[a.fg], 0);
      p = (float)(fg + 1) / (float)(all + 2);
      q = (float)(all - fg + 1) / (float)(all + 2);
    } else {
      p = a.prior[t];
      q = 1.f - p;
    }
    p = fminf(fmaxf(p, 1e-6f), 1.f);
    q = fminf(fmaxf(q, 1e-6f), 1.f);
    a.cap_source[t] = gc_quant(gc_neglog(q, p), a.unit);   // D(bg): cut when the node ends on the sink side
    a.cap_sink[t] = gc_quant(gc_neglog(p, q), a.unit);     // D(fg)
    return;
  }
  const int64_t e = t - nodes;
  if (e >= (int64_t)a.B * a.E) return;
  const int64_t b = e / a.E, k = e - b * a.E;
  const int64_t u = a.coo[k], v = a.coo[a.E + k];
  int cap = 0;
  if (u >= 0 && u < a.N && v >= 0 && v < a.N) {
    const int64_t lo = b * a.N + min(u, v), hi = b * a.N + max(u, v);   // one order for both directions: bitwise symmetric
    float w = 0.f;
    if (a.intensity) {
      const float d = a.intensity[lo] - a.intensity[hi];
      w += expf(-(d * d) * a.inv2si);
    }
    if (a.feat) {
      const float *fl = a.feat + lo * a.D, *fh = a.feat + hi * a.D;
      double s = 0.0;
      for (int j = 0; j < a.D; ++j) {
        const double d = (double)fl[j] - (double)fh[j];
        s += d * d;
      }
      w += a.gamma * expf(-(float)s * a.inv2sf);
    }
    cap = gc_quant(a.lambda * w, a.unit);
  }
  a.cap_edge[e] = cap;
}

// ---- the solver -----------------------------------------------------------------------------------------------------------------
struct SolveArgs {
  int N, E, max_rounds, period;
  const int32_t *rowptr, *col, *rev, *perm;
  const int32_t *cap_source, *cap_sink, *cap_edge;
  uint8_t* labels;
  long long* flow;
  int32_t *rounds, *converged;
};
inline size_t gc_lds_bytes(int64_t N, int64_t E) { return (size_t)(N + 1) * 8 + (size_t)E * 4 + (size_t)N * 12 + 32; }

struct GcGraph {   // the workgroup's view of its graph
  int N, E, T, t;
  const int32_t *rowptr, *col;
  unsigned* cap;     // residual arc capacities, CSR order
  unsigned* sres;    // residual sink capacities
  int* dist;         // scratch word per node
  int* flag;         // [0..2] BFS "changed", [3..5] "some node is active": rotating, so one barrier per use
};
// the arcs of node i, clamped into the arrays
__device__ __forceinline__ void gc_row(const GcGraph& g, int i, int& lo, int& hi) {
  lo = min(max(g.rowptr[i], 0), g.E);
  hi = min(max(g.rowptr[i + 1], lo), g.E);
}
// dist[i] = exact residual distance of node i to the sink, N + 1 when it cannot reach it.  In-place relaxation: every value is the
// length of a real path at any moment and only falls, so the fixed point is the same whatever the threads saw on the way.
__device__ void gc_bfs(const GcGraph& g, int& seq) {
  const int far = g.N + 1;
  for (int i = g.t; i < g.N; i += g.T) g.dist[i] = g.sres[i] ? 1 : far;
  __syncthreads();
  for (int sweep = 0; sweep < g.N; ++sweep) {
    const int cur = seq % 3;
    if (g.t == 0) g.flag[(seq + 1) % 3] = 0;
    ++seq;
    bool changed = false;
    for (int i = g.t; i < g.N; i += g.T) {
      const int d0 = g.dist[i];
      if (d0 <= 1) continue;
      int d = d0, lo, hi;
      gc_row(g, i, lo, hi);
      for (int p = lo; p < hi; ++p) {
        const int v = g.col[p];
        if (g.cap[p] && (unsigned)v < (unsigned)g.N) d = min(d, g.dist[v] + 1);
      }
      if (d < d0) {
        g.dist[i] = d;
        changed = true;
      }
    }
    if (changed) g.flag[cur] = 1;
    __syncthreads();
    if (!g.flag[cur]) break;
  }
}

// Push-relabel rounds on the residual graph in LDS until no node is active (-> 1) or max_rounds rounds are done (-> 0).  On entry
// excess / sres / cap hold the capacities and h is 0; `rounds` and `to_sink` (this thread's share of the flow into the sink) are added to.
__device__ int gc_rounds(const GcGraph& g, unsigned long long* excess, int* h, const int32_t* __restrict__ rev, int period, int max_rounds,
                         int& seq, int& aseq, int& rounds, unsigned long long& to_sink) {
  const int N = g.N, E = g.E, T = g.T, t = g.t, far = N + 1;
  unsigned* cap = g.cap;
  unsigned* sres = g.sres;
  int* dist = g.dist;
  int* flag = g.flag;
  int converged = 0;
  for (int r = 0;; ++r) {
    if (r % period == 0) {                           // global relabel; heights only ever rise
      gc_bfs(g, seq);
      for (int i = t; i < N; i += T) h[i] = max(h[i], dist[i]);
      __syncthreads();
    }
    // snapshot
    const int cur = 3 + aseq % 3;
    if (t == 0) flag[3 + (aseq + 1) % 3] = 0;
    ++aseq;
    bool any = false;
    for (int i = t; i < N; i += T) {
      const long long e = (long long)excess[i];
      const bool act = e > 0 && h[i] < far;
      dist[i] = act ? (int)min(e, (long long)INT_MAX) : 0;
      any |= act;
    }
    if (any) flag[cur] = 1;
    __syncthreads();
    if (!flag[cur]) {
      converged = 1;
      break;
    }
    if (r >= max_rounds) break;
    ++rounds;
    // push
    for (int i = t; i < N; i += T) {
      const unsigned snap = (unsigned)dist[i];
      if (!snap) continue;
      unsigned rem = snap;
      const int hi_ = h[i];
      if (hi_ == 1 && sres[i]) {
        const unsigned d = min(rem, sres[i]);
        sres[i] -= d;
        rem -= d;
        to_sink += d;
      }
      int lo, hi;
      gc_row(g, i, lo, hi);
      for (int p = lo; p < hi && rem; ++p) {
        const int v = g.col[p];
        if ((unsigned)v >= (unsigned)N || h[v] + 1 != hi_) continue;
        const unsigned c = cap[p];
        const int rp = rev[p];
        if (!c || (unsigned)rp >= (unsigned)E) continue;
        const unsigned d = min(rem, c);
        cap[p] = c - d;
        cap[rp] += d;
        atomicAdd(&excess[v], (unsigned long long)d);
        rem -= d;
      }
      if (rem != snap) atomicAdd(&excess[i], 0ull - (unsigned long long)(snap - rem));
    }
    __syncthreads();
    // relabel from the frozen heights ...
    for (int i = t; i < N; i += T) {
      int nh = h[i];
      if ((long long)excess[i] > 0 && nh < far) {
        int m = sres[i] ? 1 : far, lo, hi;
        gc_row(g, i, lo, hi);
        for (int p = lo; p < hi; ++p) {
          const int v = g.col[p];
          if (cap[p] && (unsigned)v < (unsigned)N) m = min(m, h[v] + 1);
        }
        nh = max(nh, min(m, far));
      }
      dist[i] = nh;
    }
    __syncthreads();
    // ... then commit
    for (int i = t; i < N; i += T) h[i] = dist[i];
    __syncthreads();
  }
  return converged;
}

__global__ __launch_bounds__(GC_MAX_THREADS) void graphcut_solve_kernel(const SolveArgs a) {
  extern __shared__ unsigned long long gc_lds[];
  const int N = a.N, E = a.E, T = blockDim.x, t = threadIdx.x, b = blockIdx.x, far = N + 1;
  unsigned long long* excess = gc_lds;                 // [N] excess, [N] flow into the sink
  unsigned* cap = (unsigned*)(excess + N + 1);
  int* h = (int*)(cap + E);
  unsigned* sres = (unsigned*)(h + N);
  int* dist = (int*)(sres + N);
  int* flag = dist + N;
  const GcGraph g = {N, E, T, t, a.rowptr, a.col, cap, sres, dist, flag};
  const int32_t* rev = a.rev;

  // a private copy: saturate the source arcs, negative capacities count as 0
  for (int i = t; i < N; i += T) {
    excess[i] = (unsigned long long)max(a.cap_source[(size_t)b * N + i], 0);
    sres[i] = (unsigned)max(a.cap_sink[(size_t)b * N + i], 0);
    h[i] = 0;
  }
  for (int p = t; p < E; p += T) {
    const int k = a.perm[p];
    cap[p] = (unsigned)k < (unsigned)E ? (unsigned)max(a.cap_edge[(size_t)b * E + k], 0) : 0u;
  }
  if (t < 8) flag[t] = 0;
  if (t == 0) excess[N] = 0;
  __syncthreads();

  int seq = 0, aseq = 0, rounds = 0;
  unsigned long long to_sink = 0;
  const int converged = gc_rounds(g, excess, h, rev, a.period, a.max_rounds, seq, aseq, rounds, to_sink);
  gc_bfs(g, seq);                                      // the sink side of the cut: whoever still reaches the sink
  for (int i = t; i < N; i += T) a.labels[(size_t)b * N + i] = dist[i] >= far ? 1 : 0;
  if (to_sink) atomicAdd(&excess[N], to_sink);
  __syncthreads();
  if (t == 0) {
    a.flow[b] = (long long)excess[N];
    a.rounds[b] = rounds;
    a.converged[b] = converged;
  }
}

// ---- K labels: alpha-expansion over the rounds above ------------------------------------------------------------------------------
//   E(L) = sum_i U_i(L_i) + sum over pairs {i,j} of w_ij [L_i != L_j],  U (B*N, K) int32,  w_ij = cap_edge of the arc from the LOWER to
//   the HIGHER node id (the other direction is not read); both count as clamped to [0, 2^20].
// A move on alpha is the binary cut "x_i = 1: node i takes alpha" of the current labelling, built in LDS by each node's own thread
// (for the pair i < j with a = L_i, b = L_j: A = w[a != b], B = w[a != alpha], C = w[alpha != b]; sink(i) += max(C - A, 0),
// source(i) += max(A - C, 0), source(j) += C, arc j -> i = B + C - A >= 0, arc i -> j = 0; plus U_i(alpha) on the sink and U_i(L_i) on
// the source arc), solved by gc_rounds from h = 0 and read off by gc_bfs.  It is accepted iff it lowers E strictly, alpha runs
// 0 .. K-1 cyclically, K rejected moves in a row end the loop.  LDS: the solver's arrays, one label byte per node and one 64-bit sum.
inline size_t gcm_lds_bytes(int64_t N, int64_t E) { return (size_t)(N + 2) * 8 + (size_t)E * 4 + (size_t)N * 12 + 32 + (size_t)(N + 7) / 8 * 8; }

__device__ __forceinline__ int gcm_clamp(int x) { return min(max(x, 0), GC_CAP_MAX); }

struct ExpandArgs {
  int N, E, K, max_moves, max_rounds, period;
  const int32_t *rowptr, *col, *rev, *perm;
  const int32_t *costs, *cap_edge;
  const uint8_t* init;     // (B, N) or NULL
  uint8_t* labels;
  long long* energy;
  int32_t *moves, *accepted, *rounds, *converged;
};

// the weight of the pair that CSR position p of row i stands for
__device__ __forceinline__ int gcm_pair_weight(const ExpandArgs& a, const int32_t* __restrict__ ce, int i, int v, int p) {
  const int q = i < v ? p : a.rev[p];
  const int k = (unsigned)q < (unsigned)a.E ? a.perm[q] : -1;
  return (unsigned)k < (unsigned)a.E ? gcm_clamp(ce[k]) : 0;
}

// E of the labelling "alpha where dist >= far, else lab" (alpha < 0: of lab itself): every node's thread sums its unary and the pairs
// towards its higher neighbours; integer sums, so the order of the atomic adds does not show.  Every thread returns the total.
__device__ long long gcm_energy(const ExpandArgs& a, const GcGraph& g, const int32_t* __restrict__ U, const int32_t* __restrict__ ce,
                                const uint8_t* lab, unsigned long long* acc, int alpha) {
  const int far = g.N + 1;
  if (g.t == 0) *acc = 0;
  __syncthreads();
  long long s = 0;
  for (int i = g.t; i < g.N; i += g.T) {
    const int li = alpha >= 0 && g.dist[i] >= far ? alpha : lab[i];
    s += gcm_clamp(U[(size_t)i * a.K + li]);
    int lo, hi;
    gc_row(g, i, lo, hi);
    for (int p = lo; p < hi; ++p) {
      const int v = g.col[p];
      if (v <= i || v >= g.N) continue;
      const int lv = alpha >= 0 && g.dist[v] >= far ? alpha : lab[v];
      if (li != lv) s += gcm_pair_weight(a, ce, i, v, p);
    }
  }
  s = wave_sum(s);
  if ((g.t & 63) == 0 && s) atomicAdd(acc, (unsigned long long)s);
  __syncthreads();
  const long long total = (long long)*acc;
  __syncthreads();
  return total;
}

__global__ __launch_bounds__(GC_MAX_THREADS) void graphcut_expand_kernel(const ExpandArgs a) {
  extern __shared__ unsigned long long gc_lds[];
  const int N = a.N, E = a.E, K = a.K, T = blockDim.x, t = threadIdx.x, b = blockIdx.x, far = N + 1;
  unsigned long long* excess = gc_lds;                 // [N] excess, [N] unused here, [N + 1] the energy sum
  unsigned long long* acc = excess + N + 1;
  unsigned* cap = (unsigned*)(excess + N + 2);
  int* h = (int*)(cap + E);
  unsigned* sres = (unsigned*)(h + N);
  int* dist = (int*)(sres + N);
  int* flag = dist + N;
  uint8_t* lab = (uint8_t*)(flag + 8);
  const GcGraph g = {N, E, T, t, a.rowptr, a.col, cap, sres, dist, flag};
  const int32_t* U = a.costs + (size_t)b * N * K;
  const int32_t* ce = a.cap_edge + (size_t)b * E;      // never dereferenced when E == 0

  // start: the caller's labels, or the cheapest label of the node (the lowest on ties) where none or none below K is given
  for (int i = t; i < N; i += T) {
    int l = a.init ? a.init[(size_t)b * N + i] : K;
    if (l >= K) {
      l = 0;
      int best = gcm_clamp(U[(size_t)i * K]);
      for (int k = 1; k < K; ++k) {
        const int u = gcm_clamp(U[(size_t)i * K + k]);
        if (u < best) best = u, l = k;
      }
    }
    lab[i] = (uint8_t)l;
  }
  if (t < 8) flag[t] = 0;
  if (t == 0) excess[N] = 0;
  __syncthreads();
  long long energy = gcm_energy(a, g, U, ce, lab, acc, -1);

  int seq = 0, aseq = 0, rounds = 0, moves = 0, accepted = 0, idle = 0, converged = 0;
  unsigned long long to_sink = 0;
  for (int move = 0; move < a.max_moves; ++move) {
    const int alpha = move % K;
    // the move's residual graph; each thread writes only its own nodes' words and arcs
    for (int i = t; i < N; i += T) {
      const int li = lab[i];
      unsigned long long so = (unsigned long long)gcm_clamp(U[(size_t)i * K + li]), si = (unsigned long long)gcm_clamp(U[(size_t)i * K + alpha]);
      int lo, hi;
      gc_row(g, i, lo, hi);
      for (int p = lo; p < hi; ++p) {
        const int v = g.col[p];
        unsigned c = 0;
        if ((unsigned)v < (unsigned)N && v != i) {
          const int w = gcm_pair_weight(a, ce, i, v, p), lv = lab[v];
          if (i < v) {                                 // this node is the pair's lower end
            const int A = li != lv ? w : 0, C = alpha != lv ? w : 0;
            if (C > A) si += (unsigned)(C - A);
            else so += (unsigned)(A - C);
          } else {                                     // the higher end: a = lv, b = li
            const int A = lv != li ? w : 0, B = lv != alpha ? w : 0, C = alpha != li ? w : 0;
            so += (unsigned)C;
            c = (unsigned)(B + C - A);
          }
        }
        cap[p] = c;
      }
      excess[i] = so;
      sres[i] = (unsigned)min(si, (unsigned long long)UINT_MAX);   // not reached below degree GC_WIDE_DEGREE, which the caller refuses
      h[i] = 0;
    }
    __syncthreads();
    ++moves;
    const int done = gc_rounds(g, excess, h, a.rev, a.period, a.max_rounds, seq, aseq, rounds, to_sink);
    if (!done) break;                                  // the round cap: the labels stay the last accepted ones
    gc_bfs(g, seq);                                    // dist >= far: the node takes alpha
    const long long cand = gcm_energy(a, g, U, ce, lab, acc, alpha);
    if (cand < energy) {
      for (int i = t; i < N; i += T)
        if (dist[i] >= far) lab[i] = (uint8_t)alpha;
      energy = cand;
      ++accepted;
      idle = 0;
      __syncthreads();
    } else if (++idle >= K) {
      converged = 1;
      break;
    }
  }
  for (int i = t; i < N; i += T) a.labels[(size_t)b * N + i] = lab[i];
  if (t == 0) {
    a.energy[b] = energy;
    a.moves[b] = moves;
    a.accepted[b] = accepted;
    a.rounds[b] = rounds;
    a.converged[b] = converged;
  }
}

// ---- label costs and the energy of a K-label labelling -----------------------------------------------------------------------------
// U[r][k] = q(-log p), p = prob[r][k] or (n_k + 1) / (n_all + K) from counts, clamped to [1e-6, 1]; in double, so the count path is exact
__global__ __launch_bounds__(GC_THREADS) void graphcut_label_costs_kernel(int64_t rows, int K, const float* __restrict__ prob,
                                                                          const int32_t* __restrict__ counts, float unit, int32_t* __restrict__ out) {
  const int64_t r = blockIdx.x * (int64_t)GC_THREADS + threadIdx.x;
  if (r >= rows) return;
  long long all = 0;
  if (counts)
    for (int k = 0; k < K; ++k) all += max(counts[r * K + k], 0);
  for (int k = 0; k < K; ++k) {
    double p = counts ? (double)((long long)max(counts[r * K + k], 0) + 1) / (double)(all + K) : (double)prob[r * K + k];
    p = fmin(fmax(p, 1e-6), 1.0);                      // NaN counts as 1e-6
    out[r * K + k] = (int)fmin(rint(fmax(-log(p) * (double)unit, 0.0)), (double)GC_CAP_MAX);
  }
}

__global__ __launch_bounds__(GC_THREADS) void graphcut_energy_multi_kernel(int N, int64_t E, int K, const int64_t* __restrict__ coo,
                                                                           const uint8_t* __restrict__ labels, const int32_t* __restrict__ U,
                                                                           const int32_t* __restrict__ ce, unsigned long long* __restrict__ out) {
  const int b = blockIdx.y;
  const uint8_t* lab = labels + (size_t)b * N;
  long long s = 0;
  for (int64_t i = blockIdx.x * (int64_t)GC_THREADS + threadIdx.x; i < N + E; i += (int64_t)gridDim.x * GC_THREADS) {
    if (i < N) {
      s += gcm_clamp(U[((size_t)b * N + i) * K + min((int)lab[i], K - 1)]);
    } else {
      const int64_t k = i - N, u = coo[k], v = coo[E + k];
      if (u >= 0 && u < v && v < N && lab[u] != lab[v]) s += gcm_clamp(ce[(size_t)b * E + k]);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(&out[b], (unsigned long long)s);
}

// ---- energy of a labelling ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(GC_THREADS) void graphcut_energy_kernel(int N, int64_t E, const int64_t* __restrict__ coo, const uint8_t* __restrict__ labels,
                                                                     const int32_t* __restrict__ cs, const int32_t* __restrict__ ct,
                                                                     const int32_t* __restrict__ ce, unsigned long long* __restrict__ out) {
  const int b = blockIdx.y;
  const uint8_t* lab = labels + (size_t)b * N;
  long long s = 0;
  for (int64_t i = blockIdx.x * (int64_t)GC_THREADS + threadIdx.x; i < N + E; i += (int64_t)gridDim.x * GC_THREADS) {
    if (i < N) {
      s += max(lab[i] ? ct[(size_t)b * N + i] : cs[(size_t)b * N + i], 0);
    } else {
      const int64_t k = i - N, u = coo[k], v = coo[E + k];
      if (u >= 0 && u < N && v >= 0 && v < N && lab[u] && !lab[v]) s += max(ce[(size_t)b * E + k], 0);
    }
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0 && s) atomicAdd(&out[b], (unsigned long long)s);
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_graphcut_rev_index(mgu_ctx* c, const int64_t* coo_dev, int64_t E, int num_nodes, const int32_t* rowptr_dev, const int32_t* col_dev,
                           int32_t* rev_dev, int32_t* perm_dev, int* status_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (E < 0 || E > INT_MAX || num_nodes < 0 || !rowptr_dev || !status_dev || (E > 0 && (!coo_dev || !col_dev || !rev_dev || !perm_dev)))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_rev_index args (E < 2^31)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  HIPCHK(c, hipMemsetAsync(status_dev, 0, sizeof(int), s));
  if (E == 0) return MGU_OK;
  hipLaunchKernelGGL(graphcut_rev_kernel, dim3((unsigned)((E + GC_THREADS - 1) / GC_THREADS)), dim3(GC_THREADS), 0, s, coo_dev, E, num_nodes,
                     rowptr_dev, col_dev, rev_dev, perm_dev, status_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_graphcut_capacities(mgu_ctx* c, int B, int N, const int64_t* coo_dev, int64_t E, const float* prior_dev, const int32_t* counts_dev,
                            int num_classes, int fg_class, const float* intensity_dev, const float* feat_dev, int D, float gamma,
                            float sigma_intensity, float sigma_features, float smoothness, float unit, int32_t* cap_source_dev,
                            int32_t* cap_sink_dev, int32_t* cap_edge_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B < 1 || N < 1 || E < 0 || !cap_source_dev || !cap_sink_dev || (E > 0 && (!coo_dev || !cap_edge_dev)))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_capacities args");
  if (!prior_dev == !counts_dev) return fail(c, MGU_ERR_INVALID, "graphcut_capacities: give the prior as probabilities OR as class counts");
  if (counts_dev && (num_classes < 1 || fg_class < 0 || fg_class >= num_classes))
    return fail(c, MGU_ERR_INVALID, "graphcut_capacities: foreground class %d outside the %d counted classes", fg_class, num_classes);
  if (feat_dev && D < 1) return fail(c, MGU_ERR_INVALID, "graphcut_capacities: features need D >= 1");
  if (!(unit > 0.f) || !(smoothness >= 0.f) || (intensity_dev && !(sigma_intensity > 0.f)) || (feat_dev && !(sigma_features > 0.f)))
    return fail(c, MGU_ERR_INVALID, "graphcut_capacities: unit and the sigmas must be positive, smoothness >= 0");
  const int64_t total = (int64_t)B * N + (int64_t)B * E;
  if ((int64_t)B * N > INT_MAX || (int64_t)B * E > INT_MAX) return fail(c, MGU_ERR_INVALID, "graphcut_capacities: B * N and B * E must stay below 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  CapArgs a;
  a.B = B, a.N = N, a.C = num_classes, a.fg = fg_class, a.D = D, a.E = E;
  a.coo = coo_dev, a.prior = prior_dev, a.counts = counts_dev, a.intensity = intensity_dev, a.feat = feat_dev;
  a.inv2si = intensity_dev ? (float)(1.0 / (2.0 * (double)sigma_intensity * (double)sigma_intensity)) : 0.f;
  a.inv2sf = feat_dev ? (float)(1.0 / (2.0 * (double)sigma_features * (double)sigma_features)) : 0.f;
  a.gamma = gamma, a.lambda = smoothness, a.unit = unit;
  a.cap_source = cap_source_dev, a.cap_sink = cap_sink_dev, a.cap_edge = cap_edge_dev;
  hipLaunchKernelGGL(graphcut_capacities_kernel, dim3((unsigned)((total + GC_THREADS - 1) / GC_THREADS)), dim3(GC_THREADS), 0, s, a);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_graphcut_solve(mgu_ctx* c, int B, int N, int64_t E, const int32_t* rowptr_dev, const int32_t* col_dev, const int32_t* rev_dev,
                       const int32_t* perm_dev, const int32_t* cap_source_dev, const int32_t* cap_sink_dev, const int32_t* cap_edge_dev,
                       int max_rounds, int relabel_period, int threads, uint8_t* labels_dev, int64_t* flow_dev, int32_t* rounds_dev,
                       int32_t* converged_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B < 1 || N < 1 || E < 0 || max_rounds < 0 || !rowptr_dev || !cap_source_dev || !cap_sink_dev || !labels_dev || !flow_dev || !rounds_dev ||
      !converged_dev || (E > 0 && (!col_dev || !rev_dev || !perm_dev || !cap_edge_dev)))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_solve args");
  if (relabel_period == 0) relabel_period = gc_default_period(N);
  if (threads == 0) threads = gc_default_threads(N);
  if (relabel_period < 1 || threads < 64 || threads > 1024 || threads % 64)
    return fail(c, MGU_ERR_INVALID, "graphcut_solve: relabel_period >= 1, threads a multiple of 64 in [64, 1024]");
  HIPCHK(c, hipSetDevice(c->device));
  int budget = 0;
  HIPCHK(c, hipDeviceGetAttribute(&budget, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
  const size_t lds = gc_lds_bytes(N, E);
  if (E > INT_MAX / 2 || N > INT_MAX / 2 || lds > (size_t)budget)
    return fail(c, MGU_ERR_INVALID,
                "graphcut_solve: a graph of %d nodes and %lld directed edges needs %zu bytes of LDS (20 N + 4 E + 40), the device gives one "
                "workgroup %d",
                N, (long long)E, lds, budget);
  static bool attr_done[64] = {};
  if (lds > 65536) HIPCHK(c, ensure_dyn_lds(reinterpret_cast<const void*>(&graphcut_solve_kernel), (size_t)budget, attr_done));
  hipStream_t s = (hipStream_t)hip_stream;
  SolveArgs a;
  a.N = N, a.E = (int)E, a.max_rounds = max_rounds, a.period = relabel_period;
  a.rowptr = rowptr_dev, a.col = col_dev, a.rev = rev_dev, a.perm = perm_dev;
  a.cap_source = cap_source_dev, a.cap_sink = cap_sink_dev, a.cap_edge = cap_edge_dev;
  a.labels = labels_dev, a.flow = (long long*)flow_dev, a.rounds = rounds_dev, a.converged = converged_dev;
  ProfScope ps(c, s, "graphcut_solve_kernel");
  hipLaunchKernelGGL(graphcut_solve_kernel, dim3(B), dim3(threads), lds, s, a);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_graphcut_energy(mgu_ctx* c, int B, int N, const int64_t* coo_dev, int64_t E, const uint8_t* labels_dev, const int32_t* cap_source_dev,
                        const int32_t* cap_sink_dev, const int32_t* cap_edge_dev, int64_t* energy_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B < 1 || N < 1 || E < 0 || B > 65535 || !labels_dev || !cap_source_dev || !cap_sink_dev || !energy_dev || (E > 0 && (!coo_dev || !cap_edge_dev)))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_energy args (1 <= B <= 65535)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  HIPCHK(c, hipMemsetAsync(energy_dev, 0, (size_t)B * sizeof(int64_t), s));
  const unsigned chunks = (unsigned)std::min<int64_t>(64, (N + E + GC_THREADS - 1) / GC_THREADS);
  hipLaunchKernelGGL(graphcut_energy_kernel, dim3(chunks, B), dim3(GC_THREADS), 0, s, N, E, coo_dev, labels_dev, cap_source_dev, cap_sink_dev,
                     cap_edge_dev, (unsigned long long*)energy_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_graphcut_label_costs(mgu_ctx* c, int64_t rows, int K, const float* prob_dev, const int32_t* counts_dev, float unit, int32_t* costs_dev,
                             void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (rows < 1 || K < 1 || K > 255 || rows > INT_MAX / K || !costs_dev || !(unit > 0.f))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_label_costs args (1 <= K <= 255, rows * K < 2^31, unit > 0)");
  if (!prob_dev == !counts_dev) return fail(c, MGU_ERR_INVALID, "graphcut_label_costs: give the prior as probabilities OR as class counts");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  hipLaunchKernelGGL(graphcut_label_costs_kernel, dim3((unsigned)((rows + GC_THREADS - 1) / GC_THREADS)), dim3(GC_THREADS), 0, s, rows, K, prob_dev,
                     counts_dev, unit, costs_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_graphcut_expand(mgu_ctx* c, int B, int N, int64_t E, int K, const int32_t* rowptr_dev, const int32_t* col_dev, const int32_t* rev_dev,
                        const int32_t* perm_dev, const int32_t* costs_dev, const int32_t* cap_edge_dev, const uint8_t* init_dev, int max_cycles,
                        int max_rounds, int relabel_period, int threads, uint8_t* labels_dev, int64_t* energy_dev, int32_t* moves_dev,
                        int32_t* accepted_dev, int32_t* rounds_dev, int32_t* converged_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B < 1 || N < 1 || E < 0 || max_rounds < 0 || !rowptr_dev || !costs_dev || !labels_dev || !energy_dev || !moves_dev || !accepted_dev ||
      !rounds_dev || !converged_dev || (E > 0 && (!col_dev || !rev_dev || !perm_dev || !cap_edge_dev)))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_expand args");
  if (K < 1 || K > 255) return fail(c, MGU_ERR_INVALID, "graphcut_expand: %d labels, a label is one byte: 1 <= K <= 255", K);
  if (max_cycles < 0 || max_cycles > (1 << 20)) return fail(c, MGU_ERR_INVALID, "graphcut_expand: 0 <= max_cycles <= 2^20");
  if (relabel_period == 0) relabel_period = gc_default_period(N);
  if (threads == 0) threads = gc_default_threads(N);
  if (relabel_period < 1 || threads < 64 || threads > 1024 || threads % 64)
    return fail(c, MGU_ERR_INVALID, "graphcut_expand: relabel_period >= 1, threads a multiple of 64 in [64, 1024]");
  HIPCHK(c, hipSetDevice(c->device));
  int budget = 0;
  HIPCHK(c, hipDeviceGetAttribute(&budget, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
  const size_t lds = gcm_lds_bytes(N, E);
  if (E > INT_MAX / 2 || N > INT_MAX / 2 || (int64_t)N * K > INT_MAX || lds > (size_t)budget)
    return fail(c, MGU_ERR_INVALID,
                "graphcut_expand: a graph of %d nodes and %lld directed edges needs %zu bytes of LDS (20 N + 4 E + 48 + N rounded up to 8), the "
                "device gives one workgroup %d",
                N, (long long)E, lds, budget);
  static bool attr_done[64] = {};
  if (lds > 65536) HIPCHK(c, ensure_dyn_lds(reinterpret_cast<const void*>(&graphcut_expand_kernel), (size_t)budget, attr_done));
  hipStream_t s = (hipStream_t)hip_stream;
  ExpandArgs a;
  a.N = N, a.E = (int)E, a.K = K, a.max_moves = max_cycles * K, a.max_rounds = max_rounds, a.period = relabel_period;
  a.rowptr = rowptr_dev, a.col = col_dev, a.rev = rev_dev, a.perm = perm_dev;
  a.costs = costs_dev, a.cap_edge = cap_edge_dev, a.init = init_dev;
  a.labels = labels_dev, a.energy = (long long*)energy_dev, a.moves = moves_dev, a.accepted = accepted_dev, a.rounds = rounds_dev,
  a.converged = converged_dev;
  ProfScope ps(c, s, "graphcut_expand_kernel");
  hipLaunchKernelGGL(graphcut_expand_kernel, dim3(B), dim3(threads), lds, s, a);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_graphcut_energy_multi(mgu_ctx* c, int B, int N, const int64_t* coo_dev, int64_t E, int K, const uint8_t* labels_dev, const int32_t* costs_dev,
                              const int32_t* cap_edge_dev, int64_t* energy_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (B < 1 || N < 1 || E < 0 || B > 65535 || K < 1 || K > 255 || !labels_dev || !costs_dev || !energy_dev || (E > 0 && (!coo_dev || !cap_edge_dev)))
    return fail(c, MGU_ERR_INVALID, "bad graphcut_energy_multi args (1 <= B <= 65535, 1 <= K <= 255)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  HIPCHK(c, hipMemsetAsync(energy_dev, 0, (size_t)B * sizeof(int64_t), s));
  const unsigned chunks = (unsigned)std::min<int64_t>(64, (N + E + GC_THREADS - 1) / GC_THREADS);
  hipLaunchKernelGGL(graphcut_energy_multi_kernel, dim3(chunks, B), dim3(GC_THREADS), 0, s, N, E, K, coo_dev, labels_dev, costs_dev, cap_edge_dev,
                     (unsigned long long*)energy_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
