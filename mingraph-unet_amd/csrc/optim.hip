// The optimizer step with its decisions on the device (include/mgunet.h): the passes over the flat fp32
// buffers between backward and the weight repack.
//   mgu_grad_norm        sum of squares (double), L2 norm of the scaled gradient and non-finite count into the control record, two launches
//   mgu_optim_step       those two launches, the second also deciding clip factor, skip, bias corrections and EMA decay, + one update launch
//   mgu_grad_accumulate  acc = first ? grad : acc + grad, one launch
// Launch 1, grad_norm_partial_kernel: the grid and the chunk of n elements a workgroup owns depend on n alone (norm_geometry).  The
// chunk is cut into quads of four consecutive elements counted from the buffer's FIRST ELEMENT, not from a 16-byte boundary: quad
// q of a chunk goes to thread q % 256, which squares its elements in double (exact: 48 bits) into one accumulator per position in
// the quad, in ascending q.  Which lane adds which element in which order therefore does not depend on where the buffer starts; only
// the loads do.  A buffer on a 16-byte boundary loads a quad as one 16-byte word; one that starts s = 1..3 floats past a boundary
// loads the two aligned words the quad straddles and takes 4 - s elements of the first and s of the second (the neighbour thread
// loads the second again as its first: the same cache line), and the quads whose words would reach outside [0, n) -- the first of the
// buffer, the last one or two -- are read element by element: the peeled head and tail.  The up to three elements past the last whole
// quad are added by thread 0 of the last workgroup.  Lanes combine by butterfly, waves in order (block_fold); thread 0 stores the
// workgroup's sum and count to context scratch.  No atomics, and no workgroup reads what another wrote: launch 2 does, after the launch
// boundary.
// Launch 2, optim_control_kernel, one workgroup: the partial sums go through LDS and thread 0 adds them in index order in double,
// then forms everything the header lists for the record.  NORM_MAX_BLOCKS bounds that serial chain of dependent adds.
// Launch 3, optim_update_kernel<KIND, EMA>: reads the record with plain loads; apply == 0 returns at once.  Where p, g, m, v and ema
// share their offset within 16 bytes the body runs on 16-byte words after `head` single elements that reach the boundary, else -- and
// for head and tail -- element by element, grid-strided; the arithmetic per element is one function either way.
// Measured at n = 7 766 018, the parameters of UNet(3, 2, 32, 4) (tools/optim_step_bench.py, profiles/optim_step_bench.txt): mgu_optim_step
// 47.9 us with every option off and 57.4 us as AdamW + clip + EMA, against 33.3 us for the one launch of mgu_adam_step (the update launch
// alone 35 us; the two norm launches and the launch boundaries are the rest); mgu_grad_norm alone 13.1 us, 3.1 times a device copy of
// the same bytes; the same step composed from torch on the device 431 us.
#include <limits.h>
#include <math.h>

#include <algorithm>
#include <cmath>
#include <initializer_list>

#include "ctx.h"

// An element's result must not depend on whether the 16-byte body or the single-element head and tail computed it, i.e. on where the
// buffers start: hipcc contracts a * b + c by default and chooses differently in the two loops (found by
// tests/test_gpu_optim.py::test_chain_bits_do_not_depend_on_alignment).  Every operation of this file is rounded on its own.
#pragma clang fp contract(off)

namespace mgu {
namespace {

constexpr int OPT_THREADS = 256;
static_assert(OPT_THREADS == 256, "block_fold folds four waves");
constexpr int NORM_MAX_BLOCKS = 512;               // workgroups of launch 1: the partials launch 2 adds one after the other
constexpr int64_t NORM_MIN_CHUNK = 8192;           // elements: eight quads a thread before a second workgroup is worth its partial
constexpr int NORM_UNROLL = 4;                     // quads a thread has in flight
constexpr int UPD_MAX_BLOCKS = 256 * 8;            // as launch_adam
constexpr int64_t OPT_MAX_N = (int64_t)1 << 40;    // a chunk's count of non-finite elements fits 32 bits

struct OptimCtrl {                                 // the 64-byte record of include/mgunet.h
  long long step, skipped;
  double sumsq, norm;
  float scale, bc1, bc2_sqrt, ema_d;
  int apply, nonfinite;
  int reserved[2];
};
static_assert(sizeof(OptimCtrl) == MGU_OPTIM_CTRL_BYTES, "the control record's layout is part of the ABI");

struct NormGeom {
  int blocks;
  int64_t chunk;                                   // a multiple of 4
};
NormGeom norm_geometry(int64_t n) {
  if (n < 1) return {0, 0};
  int64_t b = (n + NORM_MIN_CHUNK - 1) / NORM_MIN_CHUNK;
  if (b > NORM_MAX_BLOCKS) b = NORM_MAX_BLOCKS;
  const int64_t quads = (n + 3) / 4, chunk = (quads + b - 1) / b * 4;
  return {(int)((n + chunk - 1) / chunk), chunk};
}

__device__ __forceinline__ unsigned not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u; }

// the elements 4q .. 4q + 3 of g (all below n), s = floats by which g lies past a 16-byte boundary
__device__ __forceinline__ float4 load_quad(const float* __restrict__ g, int64_t q, int s, int64_t n) {
  const float* p = g + 4 * q;
  if (s == 0) return *reinterpret_cast<const float4*>(p);
  if (q >= 1 && 4 * q + 8 - s <= n) {              // both aligned words lie inside the buffer
    const float4 a = *reinterpret_cast<const float4*>(p - s), b = *reinterpret_cast<const float4*>(p - s + 4);
    if (s == 1) return make_float4(a.y, a.z, a.w, b.x);
    if (s == 2) return make_float4(a.z, a.w, b.x, b.y);
    return make_float4(a.w, b.x, b.y, b.z);
  }
  return make_float4(p[0], p[1], p[2], p[3]);
}

struct NormAcc {
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  unsigned bad = 0;
  __device__ __forceinline__ void add(const float4 v) {
    a[0] += (double)v.x * (double)v.x, a[1] += (double)v.y * (double)v.y;
    a[2] += (double)v.z * (double)v.z, a[3] += (double)v.w * (double)v.w;
    bad += not_finite(v.x) + not_finite(v.y) + not_finite(v.z) + not_finite(v.w);
  }
};

// ---- launch 1 ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void grad_norm_partial_kernel(const float* __restrict__ g, int64_t n, int64_t chunk, int s,
                                                                        double* __restrict__ part, unsigned* __restrict__ cnt) {
  __shared__ double sh[4];
  __shared__ unsigned shc[4];
  const int tid = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk, hi = min(n, lo + chunk);
  const int64_t q1 = hi / 4;                                            // whole quads of [lo, hi): lo / 4 .. q1 - 1
  NormAcc acc;
  int64_t q = lo / 4 + tid;
  for (; q + (NORM_UNROLL - 1) * OPT_THREADS < q1; q += NORM_UNROLL * OPT_THREADS) {
    float4 v[NORM_UNROLL];
#pragma unroll
    for (int u = 0; u < NORM_UNROLL; ++u) v[u] = load_quad(g, q + u * OPT_THREADS, s, n);
#pragma unroll
    for (int u = 0; u < NORM_UNROLL; ++u) acc.add(v[u]);
  }
  for (; q < q1; q += OPT_THREADS) acc.add(load_quad(g, q, s, n));
  double t[1] = {(acc.a[0] + acc.a[1]) + (acc.a[2] + acc.a[3])};
  if (tid == 0)                                                         // only the last workgroup has elements past its whole quads
    for (int64_t i = 4 * q1; i < hi; ++i) t[0] += (double)g[i] * (double)g[i], acc.bad += not_finite(g[i]);
  const unsigned bad = wave_sum(acc.bad);
  if ((tid & 63) == 0) shc[tid >> 6] = bad;
  block_fold<1>(t, sh);                                                 // its barrier also covers shc
  if (tid == 0) {
    part[blockIdx.x] = t[0];
    cnt[blockIdx.x] = (shc[0] + shc[1]) + (shc[2] + shc[3]);
  }
}

// ---- launch 2 ---------------------------------------------------------------------------------------------------------------------------
struct ControlArgs {
  int step_mode;                                   // 0: mgu_grad_norm (sumsq, norm, nonfinite only)
  double grad_scale, max_norm, beta1, beta2, ema_decay;
  int skip_nonfinite, ema_warmup;
};
__global__ __launch_bounds__(OPT_THREADS) void optim_control_kernel(const double* __restrict__ part, const unsigned* __restrict__ cnt,
                                                                    int blocks, const ControlArgs a, OptimCtrl* __restrict__ ctrl) {
  __shared__ double sp[NORM_MAX_BLOCKS];
  __shared__ unsigned long long shc[4];
  const int tid = threadIdx.x;
  unsigned long long bad = 0;
  for (int i = tid; i < blocks; i += OPT_THREADS) sp[i] = part[i], bad += cnt[i];
  bad = wave_sum(bad);
  if ((tid & 63) == 0) shc[tid >> 6] = bad;
  __syncthreads();
  if (tid != 0) return;
  double sumsq = 0.0;
  for (int i = 0; i < blocks; ++i) sumsq += sp[i];
  bad = (shc[0] + shc[1]) + (shc[2] + shc[3]);
  const double norm = fabs(a.grad_scale) * sqrt(sumsq);
  const int nonfinite = (int)(bad > (unsigned long long)INT_MAX ? (unsigned long long)INT_MAX : bad);
  ctrl->sumsq = sumsq, ctrl->norm = norm, ctrl->nonfinite = nonfinite;
  if (!a.step_mode) return;
  const double coef = a.max_norm > 0.0 ? fmin(1.0, a.max_norm / (norm + 1e-6)) : 1.0;
  long long step = ctrl->step;
  const int apply = !(a.skip_nonfinite && nonfinite > 0);
  if (apply) ctrl->step = ++step;
  else ctrl->skipped = ctrl->skipped + 1;
  const double t = (double)step;
  ctrl->scale = (float)(a.grad_scale * coef);
  ctrl->bc1 = (float)(1.0 - pow(a.beta1, t));
  ctrl->bc2_sqrt = (float)sqrt(1.0 - pow(a.beta2, t));
  ctrl->ema_d = (float)(a.ema_warmup ? fmin(a.ema_decay, (1.0 + t) / (10.0 + t)) : a.ema_decay);
  ctrl->apply = apply;
}

// ---- launch 3 ---------------------------------------------------------------------------------------------------------------------------
struct UpdateArgs {
  float* p;
  const float* g;
  float *m, *v, *e;
  const OptimCtrl* ctrl;
  int64_t n, head, quads;                          // [0, head) singly, then `quads` 16-byte words, then the rest singly
  float lr, b1, omb1, b2, omb2, eps, wd, keep, momentum;   // keep = 1 - lr * wd (kind 1), formed in double
};
struct UpdateStep {                                // what the record says about this step
  float scale, bc1, bc2_sqrt, ema_d, omd;
  int first;
};

// one element: the recurrences of adam_kernel / sgd_kernel (train_kernels.hip) with g' = scale * g, AdamW's decay on p itself
template <int KIND, bool EMA>
__device__ __forceinline__ void update_element(float& p, const float g, float& m, float& v, float& e, const UpdateArgs& a, const UpdateStep& k) {
  float pi = p;
  float gi = g * k.scale;
  if (KIND == MGU_OPTIM_ADAMW) pi = pi * a.keep;
  else gi = gi + a.wd * pi;
  if (KIND == MGU_OPTIM_SGD) {
    if (a.momentum != 0.f) {
      gi = k.first ? gi : a.momentum * m + gi;
      m = gi;
    }
    pi = pi - a.lr * gi;
  } else {
    const float mi = a.b1 * m + a.omb1 * gi;
    const float vi = a.b2 * v + a.omb2 * gi * gi;
    m = mi, v = vi;
    pi = pi - (a.lr / k.bc1) * mi / (sqrtf(vi) / k.bc2_sqrt + a.eps);
  }
  p = pi;
  if (EMA) e = k.ema_d * e + k.omd * pi;
}

template <int KIND, bool EMA>
__global__ __launch_bounds__(OPT_THREADS) void optim_update_kernel(const UpdateArgs a) {
  const OptimCtrl* __restrict__ c = a.ctrl;
  if (c->apply == 0) return;                                            // the whole grid: a skipped step touches nothing
  UpdateStep k;
  k.scale = c->scale, k.bc1 = c->bc1, k.bc2_sqrt = c->bc2_sqrt, k.ema_d = c->ema_d, k.omd = 1.0f - c->ema_d;
  k.first = c->step == 1;
  const bool use_m = KIND != MGU_OPTIM_SGD || a.momentum != 0.f;        // the buffers this kind reads and writes
  constexpr bool use_v = KIND != MGU_OPTIM_SGD;
  const int64_t gtid = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x, gsize = (int64_t)gridDim.x * OPT_THREADS;
  for (int64_t q = gtid; q < a.quads; q += gsize) {
    const int64_t i = a.head + 4 * q;
    float4 p = *reinterpret_cast<const float4*>(a.p + i);
    const float4 g = *reinterpret_cast<const float4*>(a.g + i);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f), v = m, e = m;
    if (use_m) m = *reinterpret_cast<const float4*>(a.m + i);
    if (use_v) v = *reinterpret_cast<const float4*>(a.v + i);
    if (EMA) e = *reinterpret_cast<const float4*>(a.e + i);
    update_element<KIND, EMA>(p.x, g.x, m.x, v.x, e.x, a, k);
    update_element<KIND, EMA>(p.y, g.y, m.y, v.y, e.y, a, k);
    update_element<KIND, EMA>(p.z, g.z, m.z, v.z, e.z, a, k);
    update_element<KIND, EMA>(p.w, g.w, m.w, v.w, e.w, a, k);
    *reinterpret_cast<float4*>(a.p + i) = p;
    if (use_m) *reinterpret_cast<float4*>(a.m + i) = m;
    if (use_v) *reinterpret_cast<float4*>(a.v + i) = v;
    if (EMA) *reinterpret_cast<float4*>(a.e + i) = e;
  }
  const int64_t body_end = a.head + 4 * a.quads, singles = a.head + (a.n - body_end);
  for (int64_t j = gtid; j < singles; j += gsize) {
    const int64_t i = j < a.head ? j : body_end + (j - a.head);
    float p = a.p[i], m = 0.f, v = 0.f, e = 0.f;
    if (use_m) m = a.m[i];
    if (use_v) v = a.v[i];
    if (EMA) e = a.e[i];
    update_element<KIND, EMA>(p, a.g[i], m, v, e, a, k);
    a.p[i] = p;
    if (use_m) a.m[i] = m;
    if (use_v) a.v[i] = v;
    if (EMA) a.e[i] = e;
  }
}

// ---- accumulation -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OPT_THREADS) void grad_accumulate_kernel(float* __restrict__ acc, const float* __restrict__ g, int64_t n,
                                                                      int64_t head, int64_t quads, int first) {
  const int64_t gtid = (int64_t)blockIdx.x * OPT_THREADS + threadIdx.x, gsize = (int64_t)gridDim.x * OPT_THREADS;
  for (int64_t q = gtid; q < quads; q += gsize) {
    const int64_t i = head + 4 * q;
    float4 v = *reinterpret_cast<const float4*>(g + i);
    if (!first) {
      const float4 o = *reinterpret_cast<const float4*>(acc + i);
      v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
    }
    *reinterpret_cast<float4*>(acc + i) = v;
  }
  const int64_t body_end = head + 4 * quads, singles = head + (n - body_end);
  for (int64_t j = gtid; j < singles; j += gsize) {
    const int64_t i = j < head ? j : body_end + (j - head);
    acc[i] = first ? g[i] : acc[i] + g[i];
  }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// [0, head) singly, `quads` 16-byte words, the rest singly: 16-byte words where every buffer of the call (NULL: not used) has the same
// offset within 16 bytes, else everything singly
void split_for_vectors(std::initializer_list<const void*> bufs, int64_t n, int64_t* head, int64_t* quads) {
  uintptr_t off = 16;
  bool same = true;
  for (const void* b : bufs) {
    if (!b) continue;
    const uintptr_t o = (uintptr_t)b & 15;
    if (off == 16) off = o;
    same = same && o == off;
  }
  *head = same ? std::min<int64_t>(n, (int64_t)((16 - off) & 15) / 4) : n;
  *quads = (n - *head) / 4;
}
bool misaligned4(std::initializer_list<const void*> bufs) {
  for (const void* b : bufs)
    if ((uintptr_t)b & 3) return true;
  return false;
}
unsigned stream_grid(int64_t quads, int64_t n) {
  return (unsigned)grid_for(std::max(quads, n - 4 * quads), OPT_THREADS, UPD_MAX_BLOCKS);
}

// launches 1 and 2
int norm_and_control(mgu_ctx* c, const float* g, int64_t n, const ControlArgs& ca, OptimCtrl* ctrl, hipStream_t s) {
  const size_t part_bytes = NORM_MAX_BLOCKS * sizeof(double);
  if (int rc = mgud::ensure(c, &c->optws, &c->optws_bytes, part_bytes + NORM_MAX_BLOCKS * sizeof(unsigned))) return rc;
  double* part = (double*)c->optws;
  unsigned* cnt = (unsigned*)((char*)c->optws + part_bytes);
  const NormGeom geo = norm_geometry(n);
  {
    mgud::ProfScope ps(c, s, "grad_norm_partial_kernel", 0, 0, -1);
    hipLaunchKernelGGL(grad_norm_partial_kernel, dim3((unsigned)geo.blocks), dim3(OPT_THREADS), 0, s, g, n, geo.chunk,
                       (int)(((uintptr_t)g >> 2) & 3), part, cnt);
  }
  {
    mgud::ProfScope ps(c, s, "optim_control_kernel", 0, 0, -1);
    hipLaunchKernelGGL(optim_control_kernel, dim3(1), dim3(OPT_THREADS), 0, s, part, cnt, geo.blocks, ca, ctrl);
  }
  return MGU_OK;
}

template <int KIND>
void launch_update(bool ema, unsigned grid, const UpdateArgs& a, hipStream_t s) {
  if (ema) hipLaunchKernelGGL((optim_update_kernel<KIND, true>), dim3(grid), dim3(OPT_THREADS), 0, s, a);
  else hipLaunchKernelGGL((optim_update_kernel<KIND, false>), dim3(grid), dim3(OPT_THREADS), 0, s, a);
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int64_t mgu_grad_norm_chunk(int64_t n) { return norm_geometry(n).chunk; }
int mgu_grad_norm_blocks(int64_t n) { return norm_geometry(n).blocks; }

int mgu_grad_norm(mgu_ctx* c, const void* grad_dev, int64_t n, float grad_scale, void* ctrl_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!grad_dev || !ctrl_dev || n < 1 || n > OPT_MAX_N) return fail(c, MGU_ERR_INVALID, "grad_norm: the gradient, the control record, 1 <= n <= 2^40");
  if (misaligned4({grad_dev}) || ((uintptr_t)ctrl_dev & 7)) return fail(c, MGU_ERR_INVALID, "grad_norm: the gradient needs 4-byte, the control record 8-byte alignment");
  if (!std::isfinite(grad_scale)) return fail(c, MGU_ERR_INVALID, "grad_norm: grad_scale must be finite");
  HIPCHK(c, hipSetDevice(c->device));
  ControlArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.grad_scale = grad_scale;
  if (int rc = norm_and_control(c, (const float*)grad_dev, n, ca, (OptimCtrl*)ctrl_dev, (hipStream_t)hip_stream)) return rc;
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_optim_step(mgu_ctx* c, const mgu_optim_desc* d, void* flat_param_dev, const void* flat_grad_dev, void* exp_avg_dev,
                   void* exp_avg_sq_dev, void* ema_dev, void* ctrl_dev, int64_t n, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!d) return fail(c, MGU_ERR_INVALID, "optim_step: no descriptor");
  if (d->kind < MGU_OPTIM_ADAM || d->kind > MGU_OPTIM_SGD) return fail(c, MGU_ERR_INVALID, "optim_step: kind %d (0 Adam, 1 AdamW, 2 SGD)", d->kind);
  if (!flat_param_dev || !flat_grad_dev || !ctrl_dev || n < 1 || n > OPT_MAX_N)
    return fail(c, MGU_ERR_INVALID, "optim_step: the parameters, the gradient, the control record, 1 <= n <= 2^40");
  const bool adam = d->kind != MGU_OPTIM_SGD, use_m = adam || d->momentum != 0.f;
  if ((use_m && !exp_avg_dev) || (adam && !exp_avg_sq_dev))
    return fail(c, MGU_ERR_INVALID, "optim_step: Adam and AdamW need both moment buffers, SGD with momentum its buffer in exp_avg_dev");
  if (!(d->max_norm >= 0.f) || !std::isfinite(d->max_norm)) return fail(c, MGU_ERR_INVALID, "optim_step: max_norm must be finite and >= 0 (0: off)");
  if (!(d->ema_decay >= 0.f && d->ema_decay < 1.f)) return fail(c, MGU_ERR_INVALID, "optim_step: ema_decay must lie in [0, 1)");
  if (d->ema_decay > 0.f && !ema_dev) return fail(c, MGU_ERR_INVALID, "optim_step: ema_decay > 0 needs the EMA buffer");
  if (!std::isfinite(d->lr) || !std::isfinite(d->grad_scale) || !std::isfinite(d->weight_decay) || !(d->eps >= 0.f) || !(d->momentum >= 0.f))
    return fail(c, MGU_ERR_INVALID, "optim_step: lr, grad_scale and weight_decay must be finite, eps and momentum >= 0");
  if (adam && !(d->beta1 >= 0.0 && d->beta1 < 1.0 && d->beta2 >= 0.0 && d->beta2 < 1.0))
    return fail(c, MGU_ERR_INVALID, "optim_step: the betas must lie in [0, 1)");
  const bool ema = d->ema_decay > 0.f;
  float* m = use_m ? (float*)exp_avg_dev : nullptr;
  float* v = adam ? (float*)exp_avg_sq_dev : nullptr;
  float* e = ema ? (float*)ema_dev : nullptr;
  if (misaligned4({flat_param_dev, flat_grad_dev, m, v, e}) || ((uintptr_t)ctrl_dev & 7))
    return fail(c, MGU_ERR_INVALID, "optim_step: the buffers need 4-byte, the control record 8-byte alignment");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  ControlArgs ca;
  memset(&ca, 0, sizeof ca);
  ca.step_mode = 1, ca.grad_scale = d->grad_scale, ca.max_norm = d->max_norm, ca.beta1 = d->beta1, ca.beta2 = d->beta2;
  ca.ema_decay = d->ema_decay, ca.skip_nonfinite = d->skip_nonfinite ? 1 : 0, ca.ema_warmup = d->ema_warmup ? 1 : 0;
  if (int rc = norm_and_control(c, (const float*)flat_grad_dev, n, ca, (OptimCtrl*)ctrl_dev, s)) return rc;
  UpdateArgs a;
  memset(&a, 0, sizeof a);
  a.p = (float*)flat_param_dev, a.g = (const float*)flat_grad_dev, a.m = m, a.v = v, a.e = e, a.ctrl = (const OptimCtrl*)ctrl_dev, a.n = n;
  split_for_vectors({a.p, a.g, m, v, e}, n, &a.head, &a.quads);
  a.lr = d->lr, a.b1 = (float)d->beta1, a.omb1 = (float)(1.0 - d->beta1), a.b2 = (float)d->beta2, a.omb2 = (float)(1.0 - d->beta2);
  a.eps = d->eps, a.wd = d->weight_decay, a.keep = (float)(1.0 - (double)d->lr * (double)d->weight_decay), a.momentum = d->momentum;
  const unsigned grid = stream_grid(a.quads, n);
  {
    ProfScope ps(c, s, "optim_update_kernel", 0, 0, -1);
    if (d->kind == MGU_OPTIM_ADAM) launch_update<MGU_OPTIM_ADAM>(ema, grid, a, s);
    else if (d->kind == MGU_OPTIM_ADAMW) launch_update<MGU_OPTIM_ADAMW>(ema, grid, a, s);
    else launch_update<MGU_OPTIM_SGD>(ema, grid, a, s);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_grad_accumulate(mgu_ctx* c, void* acc_dev, const void* grad_dev, int64_t n, int first, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!acc_dev || !grad_dev || n < 1) return fail(c, MGU_ERR_INVALID, "grad_accumulate: the accumulator, the gradient, n >= 1");
  if (misaligned4({acc_dev, grad_dev})) return fail(c, MGU_ERR_INVALID, "grad_accumulate: the buffers need 4-byte alignment");
  if (acc_dev == grad_dev) return fail(c, MGU_ERR_INVALID, "grad_accumulate: the accumulator must not be the gradient");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  int64_t head, quads;
  split_for_vectors({acc_dev, grad_dev}, n, &head, &quads);
  {
    ProfScope ps(c, s, "grad_accumulate_kernel", 0, 0, -1);
    hipLaunchKernelGGL(grad_accumulate_kernel, dim3(stream_grid(quads, n)), dim3(OPT_THREADS), 0, s, (float*)acc_dev, (const float*)grad_dev,
                       n, head, quads, first ? 1 : 0);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
