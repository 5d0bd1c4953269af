// Segmentation evaluation on the device: the scoring loop of experiments/segmentation_performance.py:125-151 without the host.
//   mgu_segmentation_eval   logits + labels -> argmax (:141), confusion counts (experiments/metrics.py:21, sklearn's
//                           confusion_matrix(labels=range(C))) and, optionally, the eval-mode loss (nn.CrossEntropyLoss() and
//                           dice_loss, scripts/train_segmentation.py:29-40, 91) -- ONE read of the logits and of the labels
//   mgu_confusion_matrix    counts of two given label vectors (segmentation_metrics takes two label tensors)
// Counts: per workgroup in registers (C == 2) or in an LDS histogram, then each workgroup adds its nonzero cells to the caller's
// int64 (C, C) buffer with 64-bit INTEGER atomics: the sum does not depend on the order, so it is exact and reproducible.
// Loss: each workgroup writes its double partials to a fixed slot; one finishing workgroup adds them in a fixed order (bitwise
// reproducible, no float atomics) and accumulates the batch loss into the caller's double[2] (the reference's val_loss += loss.item()).
#include <algorithm>

#include "ctx.h"

namespace mgu {
namespace {

constexpr int SE_THREADS = 256;
constexpr int SE_TARGET_BLOCKS = 256;      // about one workgroup per CU: few atomics per confusion cell
constexpr int SE_HIST_CELLS = 8192;        // LDS histogram up to C = 90 (32 KB); above: atomics straight to the caller's buffer
constexpr long long IGNORE_INDEX = -100;   // nn.CrossEntropyLoss default

// ---- C == 2 (configs/model.yaml): 16-byte loads, two pixels per lane and load -----------------------------------------------------
// LOSS 0: counts (+ predictions) only, no exp/log.  1: + cross-entropy partials.  2: + dice partials.
// Record of workgroup (b, blk): [ce_sum, counted, D0, D1, P0, P1, T0, T1] (LOSS 2) or [ce_sum, counted] (LOSS 1).
// Dice: with P = sum p_c and T = the label count, the dice term 1 - (2 I + s) / (P + T + s) is D / (P + T + s), D = P + T - 2 I = the
// sum over the pixels of 1 - p_c where the label is c and of p_c elsewhere.  D is a sum of non-negative terms (PixelCE::miss forms
// 1 - p_c without cancellation); 2 I + s against P + T + s cancels at 1, and a trained network's dice loss is 1e-5.
template <int LOSS>
struct C2Acc {
  unsigned n[4] = {0, 0, 0, 0};   // cm[y][p] at y * 2 + p
  double ce = 0.0, D0 = 0.0, D1 = 0.0, P0 = 0.0, P1 = 0.0;
  bool bad = false;
  __device__ __forceinline__ int pixel(float l0, float l1, long long y) {
    const int p = l1 > l0 ? 1 : 0;   // first maximal index (strict >), as argmax_kernel
    n[0] += (y == 0) & (p == 0);
    n[1] += (y == 0) & (p == 1);
    n[2] += (y == 1) & (p == 0);
    n[3] += (y == 1) & (p == 1);
    if constexpr (LOSS > 0) {
      const float mx = fmaxf(l0, l1);
      const float e0 = expf(l0 - mx), e1 = expf(l1 - mx);
      PixelCE s;
      s.add(0, e0);
      s.add(1, e1);
      const bool counted = y == 0 || y == 1;
      if (counted) ce += (double)s.term(mx, y ? l1 : l0);
      else if (y != IGNORE_INDEX) ce += (double)__builtin_nanf(""), bad = true;   // mgu_cross_entropy's semantics
      if constexpr (LOSS == 2) {
        if (!counted) bad = true;   // F.one_hot raises on any label outside [0, C), -100 included (:34)
        const float inv = 1.f / s.se, p0 = e0 * inv, p1 = e1 * inv;
        D0 += (double)(y == 0 ? s.miss(0, e0) : p0);
        D1 += (double)(y == 1 ? s.miss(1, e1) : p1);
        P0 += (double)p0;
        P1 += (double)p1;
      }
    }
    return p;
  }
};

template <int LOSS>
__global__ __launch_bounds__(SE_THREADS) void seg_eval_c2_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                 int B, int64_t HW, long long* __restrict__ pred,
                                                                 unsigned long long* __restrict__ cm, double* __restrict__ part,
                                                                 int* __restrict__ err_word) {
  __shared__ unsigned shn[4][4];
  __shared__ double shd[4 * 5];
  const int nb = gridDim.x, blk = blockIdx.x, tid = threadIdx.x;
  C2Acc<LOSS> a;
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    const int64_t g0 = (int64_t)b * HW, g1 = g0 + HW;           // this image's pixels, flat over the batch
    const int64_t a0 = (g0 + 1) & ~(int64_t)1, a1 = g1 & ~(int64_t)1;
    // an unaligned first / last pixel of the image (odd H*W): one lane of the image's first workgroup takes each
    if (blk == 0 && tid < 2) {
      const int64_t g = tid == 0 ? g0 : a1;
      if ((tid == 0 && g0 < a0) || (tid == 1 && a1 < g1 && a1 >= a0)) {
        const int p = a.pixel(logits[2 * g], logits[2 * g + 1], labels[g]);
        if (pred) pred[g] = p;
      }
    }
    const int64_t q0 = a0 >> 1, nq = (a1 - a0) >> 1;            // pixel pairs [q0, q0 + nq)
    const int64_t step = (int64_t)nb * SE_THREADS;
    int64_t q = (int64_t)blk * SE_THREADS + tid;
    // four pairs per lane in flight: 128 bytes of loads issued before the first is used
    for (; q + 3 * step < nq; q += 4 * step) {
      float4 l[4];
      longlong2 y[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        l[u] = reinterpret_cast<const float4*>(logits)[q0 + q + u * step];
        y[u] = reinterpret_cast<const longlong2*>(labels)[q0 + q + u * step];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p0 = a.pixel(l[u].x, l[u].y, y[u].x), p1 = a.pixel(l[u].z, l[u].w, y[u].y);
        if (pred) reinterpret_cast<longlong2*>(pred)[q0 + q + u * step] = make_longlong2(p0, p1);
      }
    }
    for (; q < nq; q += step) {
      const float4 l = reinterpret_cast<const float4*>(logits)[q0 + q];
      const longlong2 y = reinterpret_cast<const longlong2*>(labels)[q0 + q];
      const int p0 = a.pixel(l.x, l.y, y.x), p1 = a.pixel(l.z, l.w, y.y);
      if (pred) reinterpret_cast<longlong2*>(pred)[q0 + q] = make_longlong2(p0, p1);
    }
    if (LOSS > 0) {   // per-image records (the dice sums are per (image, class)); the loop above ran for image b only
      if (a.bad && err_word) atomicOr(err_word, 1);
      unsigned cnt[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {   // written out: wave_sum (device.h) here changes this kernel's register allocation
        cnt[k] = a.n[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) cnt[k] += __shfl_xor(cnt[k], off);
      }
      if ((tid & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) shn[tid >> 6][k] = cnt[k];
      double v[5] = {a.ce, a.D0, a.D1, a.P0, a.P1};
      block_fold<5>(v, shd);   // its barrier also publishes shn
      if (tid == 0) {
        unsigned long long t[4];
        for (int k = 0; k < 4; ++k) t[k] = (unsigned long long)shn[0][k] + shn[1][k] + shn[2][k] + shn[3][k];
        double* r = part + ((size_t)b * nb + blk) * (LOSS == 2 ? 8 : 2);
        r[0] = v[0];
        r[1] = (double)(t[0] + t[1] + t[2] + t[3]);
        if (LOSS == 2) r[2] = v[1], r[3] = v[2], r[4] = v[3], r[5] = v[4], r[6] = (double)(t[0] + t[1]), r[7] = (double)(t[2] + t[3]);
        for (int k = 0; k < 4; ++k)
          if (t[k]) atomicAdd(cm + k, t[k]);
      }
      __syncthreads();   // shn / shd are reused by the next image
      a = C2Acc<LOSS>();
    }
  }
  if (LOSS == 0) {   // counts of every image this workgroup saw: one wave reduction, one LDS fold, <= 4 atomics
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) a.n[k] += __shfl_xor(a.n[k], off);
    if ((tid & 63) == 0)
#pragma unroll
      for (int k = 0; k < 4; ++k) shn[tid >> 6][k] = a.n[k];
    __syncthreads();
    if (tid < 4) {
      const unsigned long long t = (unsigned long long)shn[0][tid] + shn[1][tid] + shn[2][tid] + shn[3][tid];
      if (t) atomicAdd(cm + tid, t);
    }
  }
}

// ---- any C: scalar pixels, LDS histogram (or, past SE_HIST_CELLS, atomics to the caller's buffer) ---------------------------------
// NC > 0: C <= NC, the logits of a pixel held in registers (LOSS 2 possible).  NC == 0: any C, LOSS 0 or 1.
// Record of workgroup (b, blk): [ce_sum, counted, D[0..C), P[0..C), T[0..C)] (LOSS 2) or [ce_sum, counted].
template <int NC, int LOSS>
__global__ __launch_bounds__(SE_THREADS) void seg_eval_generic_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                                                                      int B, int64_t HW, int C, long long* __restrict__ pred,
                                                                      unsigned long long* __restrict__ cm, double* __restrict__ part,
                                                                      int* __restrict__ err_word) {
  extern __shared__ unsigned hist[];   // C * C cells when C * C <= SE_HIST_CELLS
  constexpr int K = LOSS == 2 ? 2 + 3 * NC : 2;
  __shared__ double shd[4 * K];
  const int nb = gridDim.x, blk = blockIdx.x, tid = threadIdx.x;
  const int cells = C * C;
  const bool lds = cells <= SE_HIST_CELLS;
  if (lds)
    for (int k = tid; k < cells; k += SE_THREADS) hist[k] = 0;
  __syncthreads();
  for (int b = blockIdx.y; b < B; b += gridDim.y) {
    double v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0.0;
    bool bad = false;
    for (int64_t i = (int64_t)blk * SE_THREADS + tid; i < HW; i += (int64_t)nb * SE_THREADS) {
      const int64_t g = (int64_t)b * HW + i;
      const float* p = logits + g * C;
      const long long y = labels[g];
      float l[NC > 0 ? NC : 1];
      float best;
      int arg = 0;
      if (NC > 0) {
#pragma unroll
        for (int c = 0; c < NC; ++c) l[c] = c < C ? p[c] : 0.f;
        best = l[0];
#pragma unroll
        for (int c = 1; c < NC; ++c)
          if (c < C && l[c] > best) best = l[c], arg = c;
      } else {
        best = p[0];
        for (int c = 1; c < C; ++c) {
          const float x = p[c];
          if (x > best) best = x, arg = c;
        }
      }
      if (pred) pred[g] = arg;
      const bool counted = y >= 0 && y < C;
      if (counted) {
        if (lds) atomicAdd(&hist[(int)y * C + arg], 1u);
        else atomicAdd(cm + (int64_t)y * C + arg, 1ull);
      }
      if constexpr (LOSS > 0) {
        // the sequence of mgu_cross_entropy / dice_partial_kernel: max by fmaxf, sum of exp in class order
        float mx = NC > 0 ? l[0] : p[0];
        if (NC > 0) {
#pragma unroll
          for (int c = 1; c < NC; ++c)
            if (c < C) mx = fmaxf(mx, l[c]);
        } else {
          for (int c = 1; c < C; ++c) mx = fmaxf(mx, p[c]);
        }
        PixelCE s;
        if (NC > 0) {
#pragma unroll
          for (int c = 0; c < NC; ++c) {
            l[c] = c < C ? expf(l[c] - mx) : 0.f;
            if (c < C) s.add(c, l[c]);
          }
        } else {
          for (int c = 0; c < C; ++c) s.add(c, expf(p[c] - mx));
        }
        if (counted) v[0] += (double)s.term(mx, p[y]), v[1] += 1.0;
        else if (y != IGNORE_INDEX) v[0] += (double)__builtin_nanf(""), bad = true;
        if constexpr (LOSS == 2) {
          if (!counted) bad = true;
          const float inv = 1.f / s.se;
#pragma unroll
          for (int c = 0; c < (NC > 0 ? NC : 1); ++c) {
            const float pc = l[c] * inv;
            v[2 + c] += (double)(y == c ? s.miss(c, l[c]) : pc);
            v[2 + NC + c] += (double)pc;
            v[2 + 2 * NC + c] += y == c ? 1.0 : 0.0;
          }
        }
      }
    }
    if (LOSS > 0) {
      if (bad && err_word) atomicOr(err_word, 1);
      block_fold<K>(v, shd);
      if (tid == 0) {
        const int S = LOSS == 2 ? 2 + 3 * C : 2;
        double* r = part + ((size_t)b * nb + blk) * S;
        r[0] = v[0], r[1] = v[1];
        if constexpr (LOSS == 2)
          for (int c = 0; c < C; ++c) r[2 + c] = v[2 + c], r[2 + C + c] = v[2 + NC + c], r[2 + 2 * C + c] = v[2 + 2 * NC + c];
      }
      __syncthreads();
    }
  }
  if (lds) {
    __syncthreads();
    for (int k = tid; k < cells; k += SE_THREADS)
      if (hist[k]) atomicAdd(cm + k, (unsigned long long)hist[k]);
  }
}

// one workgroup: CE mean and dice over all records in a fixed order, then acc[0] += batch loss, acc[1] += 1
__global__ __launch_bounds__(SE_THREADS) void seg_eval_final_kernel(const double* __restrict__ part, int B, int nb, int C, int S, int dice,
                                                                    double smooth, double* __restrict__ terms, double* __restrict__ acc) {
  __shared__ double shd[8];
  const int tid = threadIdx.x;
  double v[2] = {0.0, 0.0};
  const int64_t nrec = (int64_t)B * nb;
  for (int64_t r = tid; r < nrec; r += SE_THREADS) v[0] += part[r * S], v[1] += part[r * S + 1];
  block_fold<2>(v, shd);
  if (dice)
    for (int64_t t = tid; t < (int64_t)B * C; t += SE_THREADS) {
      const int64_t b = t / C;
      const int c = (int)(t - b * C);
      double D = 0, P = 0, T = 0;
      for (int k = 0; k < nb; ++k) {
        const double* r = part + (b * nb + k) * S;
        D += r[2 + c], P += r[2 + C + c], T += r[2 + 2 * C + c];
      }
      terms[t] = D / (P + T + smooth);   // 1 - (2 I + smooth) / (P + T + smooth), train_segmentation.py:39
    }
  __syncthreads();
  if (tid == 0) {
    float loss = (float)(v[0] / v[1]);   // mean over the counted pixels; none counted -> NaN, as torch's 0/0
    if (dice) {
      double s = 0.0;
      for (int64_t t = 0; t < (int64_t)B * C; ++t) s += terms[t];
      loss += (float)(s / ((double)B * C));   // :40, the mean of 1 - dice; loss_ce + loss_dice in fp32 (:130)
    }
    acc[0] += (double)loss;
    acc[1] += 1.0;
  }
}

// counts of (true, pred) pairs; a pair with either label outside [0, C) is not counted (sklearn drops it)
__global__ __launch_bounds__(SE_THREADS) void confusion_kernel(const long long* __restrict__ yt, const long long* __restrict__ yp, int64_t n,
                                                               int C, unsigned long long* __restrict__ cm) {
  extern __shared__ unsigned hist[];
  const int cells = C * C, tid = threadIdx.x;
  const bool lds = cells <= SE_HIST_CELLS;
  if (lds)
    for (int k = tid; k < cells; k += SE_THREADS) hist[k] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * SE_THREADS + tid; i < n; i += (int64_t)gridDim.x * SE_THREADS) {
    const long long t = yt[i], p = yp[i];
    if (t < 0 || t >= C || p < 0 || p >= C) continue;
    if (lds) atomicAdd(&hist[(int)t * C + (int)p], 1u);
    else atomicAdd(cm + t * C + p, 1ull);
  }
  if (lds) {
    __syncthreads();
    for (int k = tid; k < cells; k += SE_THREADS)
      if (hist[k]) atomicAdd(cm + k, (unsigned long long)hist[k]);
  }
}


}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_segmentation_eval(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                          int64_t* confusion_dev, int64_t* pred_dev, int loss_kind, float dice_smooth, double* loss_acc_dev,
                          void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!logits_dev || !labels_dev || !confusion_dev || B < 0 || HW < 0 || num_classes < 1)
    return fail(c, MGU_ERR_INVALID, "bad segmentation_eval args (null pointer, negative size or num_classes < 1)");
  if (loss_kind < 0 || loss_kind > 2) return fail(c, MGU_ERR_INVALID, "bad segmentation_eval loss_kind %d (0 none, 1 ce, 2 ce+dice)", loss_kind);
  if ((loss_kind > 0) != (loss_acc_dev != nullptr))
    return fail(c, MGU_ERR_INVALID, "segmentation_eval: loss_acc_dev must be given iff loss_kind > 0");
  if (loss_kind == 2 && num_classes > 8) return fail(c, MGU_ERR_INVALID, "segmentation_eval: the dice loss needs num_classes <= 8");
  if ((double)num_classes * num_classes > (double)INT32_MAX) return fail(c, MGU_ERR_INVALID, "segmentation_eval: num_classes too large");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const int64_t npix = (int64_t)B * HW;
  if (npix == 0 && loss_kind == 0) return MGU_OK;
  const int C = num_classes;
  // workgroups per image: about SE_TARGET_BLOCKS over the batch, >= 2048 pixels each
  const int nb = npix == 0 ? 0 : (int)std::max<int64_t>(1, std::min<int64_t>((SE_TARGET_BLOCKS + B - 1) / B, (HW + 2047) / 2048));
  const int gy = std::min(B, 65535);
  const int S = loss_kind == 2 ? 2 + 3 * C : 2;
  double* part = nullptr;
  int* err_dev = nullptr;
  if (loss_kind > 0) {
    const size_t doubles = (size_t)B * nb * S + (loss_kind == 2 ? (size_t)B * C : 0) + 1;
    int rc = ensure(c, &c->lossws, &c->lossws_bytes, doubles * sizeof(double));
    if (rc) return rc;
    part = (double*)c->lossws;
    if ((rc = err_word_dev(c, &err_dev))) return rc;
  }
  const float* lg = (const float*)logits_dev;
  const long long* yl = (const long long*)labels_dev;
  long long* pr = (long long*)pred_dev;
  unsigned long long* cm = (unsigned long long*)confusion_dev;
  if (npix > 0) {
    const dim3 grid(nb, gy);
    if (C == 2 && aligned16(logits_dev) && aligned16(labels_dev) && (!pred_dev || aligned16(pred_dev))) {
      if (loss_kind == 0) hipLaunchKernelGGL(seg_eval_c2_kernel<0>, grid, dim3(SE_THREADS), 0, s, lg, yl, B, HW, pr, cm, part, err_dev);
      else if (loss_kind == 1) hipLaunchKernelGGL(seg_eval_c2_kernel<1>, grid, dim3(SE_THREADS), 0, s, lg, yl, B, HW, pr, cm, part, err_dev);
      else hipLaunchKernelGGL(seg_eval_c2_kernel<2>, grid, dim3(SE_THREADS), 0, s, lg, yl, B, HW, pr, cm, part, err_dev);
    } else {
      const size_t lds = (int64_t)C * C <= SE_HIST_CELLS ? (size_t)C * C * sizeof(unsigned) : 0;
#define MGU_SE_GENERIC(NC, LOSS) \
  hipLaunchKernelGGL((seg_eval_generic_kernel<NC, LOSS>), grid, dim3(SE_THREADS), lds, s, lg, yl, B, HW, C, pr, cm, part, err_dev)
      if (C <= 8) {
        if (loss_kind == 0) MGU_SE_GENERIC(8, 0);
        else if (loss_kind == 1) MGU_SE_GENERIC(8, 1);
        else MGU_SE_GENERIC(8, 2);
      } else {
        if (loss_kind == 0) MGU_SE_GENERIC(0, 0);
        else MGU_SE_GENERIC(0, 1);
      }
#undef MGU_SE_GENERIC
    }
  }
  if (loss_kind > 0)
    hipLaunchKernelGGL(seg_eval_final_kernel, dim3(1), dim3(SE_THREADS), 0, s, part, B, nb, C, S, loss_kind == 2 ? 1 : 0, (double)dice_smooth,
                       part + (size_t)B * nb * S, loss_acc_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_confusion_matrix(mgu_ctx* c, const int64_t* true_dev, const int64_t* pred_dev, int64_t n, int num_classes, int64_t* confusion_dev,
                         void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!true_dev || !pred_dev || !confusion_dev || n < 0 || num_classes < 1)
    return fail(c, MGU_ERR_INVALID, "bad confusion_matrix args (null pointer, negative size or num_classes < 1)");
  if ((double)num_classes * num_classes > (double)INT32_MAX) return fail(c, MGU_ERR_INVALID, "confusion_matrix: num_classes too large");
  HIPCHK(c, hipSetDevice(c->device));
  if (n == 0) return MGU_OK;
  const int C = num_classes;
  const int nb = (int)std::max<int64_t>(1, std::min<int64_t>(SE_TARGET_BLOCKS, (n + 4095) / 4096));
  const size_t lds = (int64_t)C * C <= SE_HIST_CELLS ? (size_t)C * C * sizeof(unsigned) : 0;
  hipLaunchKernelGGL(confusion_kernel, dim3(nb), dim3(SE_THREADS), lds, (hipStream_t)hip_stream, (const long long*)true_dev,
                     (const long long*)pred_dev, n, C, (unsigned long long*)confusion_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
