// Device helpers shared by the kernel files: each is defined here and nowhere else under csrc/ (tests/test_csrc_helpers.py).
//   vector types | three-way bf16 operand split and the bf16 MFMA | LDS hand-off barriers | wave and workgroup reductions |
//   order-preserving float encoding | per-pixel softmax and byte normalisation | node -> graph search
// common.h includes this header, so every translation unit sees it.  The GAT-specific slotted max accumulators and the DPP
// reductions built on them are in gat_common.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

namespace mgu {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- exact three-way bf16 operand split for the fp32 kernels that run on the bf16 matrix pipe ----------------------------------
// exact three-way split of two fp32 values into packed bf16 pieces (low half: a, high half: b)
__device__ __forceinline__ void split3_pack(const float a, const float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  p0 = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
  const float ra = a - __uint_as_float(ua & 0xffff0000u), rb = b - __uint_as_float(ub & 0xffff0000u);
  const unsigned va = __float_as_uint(ra), vb = __float_as_uint(rb);
  p1 = __builtin_amdgcn_perm(vb, va, 0x07060302u);
  const float sa = ra - __uint_as_float(va & 0xffff0000u), sb = rb - __uint_as_float(vb & 0xffff0000u);
  p2 = __builtin_amdgcn_perm(__float_as_uint(sb), __float_as_uint(sa), 0x07060302u);
}
// One-instruction fp32 arithmetic the backend cannot pair into v_pk_add_f32 / v_pk_fma_f32: beside a dense MFMA stream the packed
// forms are slow (wino_f32.hip: +2.5 % on the whole forward; the Winograd weight gradient ran 2 x slower with a packed split).
__device__ __forceinline__ float x3_add(float a, float b) {
  float d;
  asm("v_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ float x3_sub(float a, float b) {
  float d;
  asm("v_sub_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__device__ __forceinline__ float x3_fma(float a, float b, float c) {
  float d;
  asm("v_fma_f32 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
  return d;
}
// split3_pack with those subtractions
__device__ __forceinline__ void split3_pack_s(const float a, const float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  const unsigned ua = __float_as_uint(a), ub = __float_as_uint(b);
  p0 = __builtin_amdgcn_perm(ub, ua, 0x07060302u);
  const float ra = x3_sub(a, __uint_as_float(ua & 0xffff0000u)), rb = x3_sub(b, __uint_as_float(ub & 0xffff0000u));
  const unsigned va = __float_as_uint(ra), vb = __float_as_uint(rb);
  p1 = __builtin_amdgcn_perm(vb, va, 0x07060302u);
  const float sa = x3_sub(ra, __uint_as_float(va & 0xffff0000u)), sb = x3_sub(rb, __uint_as_float(vb & 0xffff0000u));
  p2 = __builtin_amdgcn_perm(__float_as_uint(sb), __float_as_uint(sa), 0x07060302u);
}

__device__ __forceinline__ f32x16 mfma_bf16(const u32x4 a, const u32x4 b, const f32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// f(integral_constant<int, I>) for I = I .. N - 1, unrolled at compile time
template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// ---- workgroup barriers for LDS hand-offs ---------------------------------------------------------------------------------------
// __syncthreads() is a workgroup-scope fence + barrier, and the fence makes hipcc wait for vmcnt(0): every outstanding global load
// AND store (CDNA4 counts stores in vmcnt) -- a kernel that prefetches the next step's operands would drain them at every step.  LDS
// operations of a wave complete in order, so lgkmcnt(0) before s_barrier is all a producer needs.  Both raw forms below emit
// `s_waitcnt lgkmcnt(0); s_barrier` and no vmcnt wait, and carry no fence.  They stay apart because the code around them
// differs: the asm statement is opaque to the backend's waitcnt insertion and scheduler, the builtins are not (igemm.hip's LDS-DMA
// kernels come out in another instruction order under the asm spelling).
// lds_barrier: the inline-asm spelling; the "memory" clobber keeps the compiler from moving LDS accesses across it.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// lds_barrier_builtin: the builtin spelling (s_barrier is IntrNoMem); the two empty asm statements are compiler-only ordering points
// that keep every LDS access of the source on its side of the barrier without emitting an instruction.
__device__ __forceinline__ void lds_barrier_builtin() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
  __builtin_amdgcn_s_barrier();
  asm volatile("" ::: "memory");
}
// lds_barrier_fenced: __syncthreads() under the name of what it is used for (gat_fused.hip says why that kernel stays on it).
__device__ __forceinline__ void lds_barrier_fenced() { __syncthreads(); }

// ---- reductions -----------------------------------------------------------------------------------------------------------------
// Full-wave butterflies over __shfl_xor (six ds_bpermute round trips): every lane gets the result; for any type, once or a few times
// per kernel.  In a loop that runs per tile or per edge use the DPP forms instead (wave_max_u32 in gat_common.h, dpp_add / node_sum in
// gat_fused.hip): different instructions, chosen on the measurements written next to them.
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off));
  return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off));
  return v;
}
// fold K doubles of every thread of a 256-thread workgroup; thread 0 gets the totals (fixed order)
template <int K>
__device__ __forceinline__ void block_fold(double (&v)[K], double* sh /* [4][K] */) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) sh[wave * K + k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = sh[k] + sh[K + k] + sh[2 * K + k] + sh[3 * K + k];
}

// ---- order-preserving float <-> unsigned encoding (atomicMax on floats) ---------------------------------------------------------
__device__ __forceinline__ unsigned enc_ordered(float f) {
  const unsigned u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float dec_ordered(unsigned u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u);
}

// ---- per-pixel arithmetic shared by the inference glue (tta.hip, tiled.hip; imageops.hip, augment.hip) --------------------------
// the softmax of one pixel's C <= CM logits at p, up to its normalisation: e[c] = expf(p[c] - max) in fp32, returns their sum; the
// probability of class c is e[c] / sum
template <int CM>
__device__ __forceinline__ float pixel_softmax(const float* p, int C, float (&e)[CM]) {
  float l[CM];
  float m = p[0];
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      l[c] = p[c];
      m = fmaxf(m, l[c]);
    }
  float sum = 0.f;
#pragma unroll
  for (int c = 0; c < CM; ++c)
    if (c < C) {
      e[c] = expf(l[c] - m);
      sum += e[c];
    }
  return sum;
}
// The cross-entropy side of one pixel's softmax, for the loss kernels (train_kernels.hip, seg_eval.hip).  add(c, e) once per class in
// class order with e = expf(l[c] - mx), mx the pixel's largest logit.  se: the sum of all e, the softmax's normalisation; rest: the
// same sum without ONE class whose e is exactly 1 (a maximal class: expf(0) == 1), which is class `skip`.
//   term(mx, ly)  -log softmax[y] = log1pf(rest) + (mx - ly), ly = l[y]: both summands are >= 0, and neither moves when a constant
//                 is added to the pixel's logits.  (mx + logf(se)) - ly cancels at the magnitude of the logits instead: ulp(12) =
//                 9.5e-7 against the 6e-6 of a pixel that is right by a margin of 12, the everyday pixel of a trained network.
//   miss(c, e)    1 - softmax[c] = (se - e) / se, with se - e = rest for the skipped class: 1.f - e / se cancels in the same way.
struct PixelCE {
  float se = 0.f, rest = 0.f;
  int skip = -1;
  __device__ __forceinline__ void add(int c, float e) {
    se += e;
    if (skip < 0 && e == 1.f) skip = c;
    else rest += e;
  }
  __device__ __forceinline__ float term(float mx, float ly) const { return log1pf(rest) + (mx - ly); }
  __device__ __forceinline__ float miss(int c, float e) const { return (c == skip ? rest : se - e) / se; }
};
// torchvision's ToTensor (/255) and Normalize of one byte of channel c in {0, 1, 2}, given the three means and standard deviations
__device__ __forceinline__ float u8_normalize(uint8_t u, int c, float m0, float m1, float m2, float s0, float s1, float s2) {
  const float v = (float)u / 255.f;
  const float mean = c == 0 ? m0 : (c == 1 ? m1 : m2), sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
  return (v - mean) / sd;
}

// graph of a node: binary search over graph_ptr (gp[g] <= node < gp[g + 1]); no graph_ptr or one graph: 0
__device__ __forceinline__ int graph_of(const int32_t* __restrict__ gp, int G, int node) {
  if (!gp || G <= 1) return 0;
  int lo = 0, hi = G;  // gp[lo] <= node < gp[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (gp[mid] <= node) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace mgu
