// Object shape on the device: per-object moments of mgu_connected_components' label map, the fitted ellipse and the per-instance
// EllipticalShapeLoss term (model/unet/shape_loss.py:155-180) -- the instance form :42-48 and :85-92 ask for.
//   mgu_object_moments                 labels (B, H, W) -> per object the 12 raw integer power sums of orders 2..4, coordinates taken
//                                      relative to the object's own (xmin, ymin); uint64 integer atomics (exact, order-free)
//   mgu_object_shapes                  one thread per object, fp64 from the exact integers: centroid, covariance, ellipse axes, angle,
//                                      fill ratio, the reference's loss term, a status byte; every output rounded to fp32 once.  The
//                                      term of a thin object (ill-conditioned cov + eps I) comes from a per-pixel pass instead
//   mgu_elliptical_shape_loss_objects  the mean of the terms of the analysed objects, one workgroup, fp64, fixed order
// The launch count is the same for one object and for a million (thin ones or none): no per-object launches, no dense masks, no host synchronisation.
// The term needs no second sweep: with m_j = iyy dy^2 + 2 ixy dy dx + ixx dx^2 (the inverse of cov + eps I applied to the centred
// pixel), sum (m - 1)^2 = sum m^2 - 2 sum m + n is a fixed combination of the central moments of orders 2 and 4, and those follow
// from the raw ones by the binomial shift.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int SH_THREADS = 256;
constexpr int SH_ROWS = 16;                   // rows per tile: a lane keeps one object's sums in registers down its column
constexpr int NMOM = 12;                      // x^2 xy y^2 | x^3 x^2y xy^2 y^3 | x^4 x^3y x^2y^2 xy^3 y^4
typedef unsigned long long u64;

__global__ __launch_bounds__(SH_THREADS) void moments_init_kernel(const long long* __restrict__ offsets, int B, int64_t cap, u64* __restrict__ mom) {
  const int64_t n = objects_recorded(offsets, B, cap) * NMOM;
  for (int64_t i = (int64_t)blockIdx.x * SH_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * SH_THREADS) mom[i] = 0;
}

// a lane adds its sums to object o on its own (zero sums -- a one-pixel object has only those -- cost nothing)
__device__ __forceinline__ void flush_direct(u64* __restrict__ mom, long long o, const u64* acc) {
#pragma unroll
  for (int k = 0; k < NMOM; ++k)
    if (acc[k]) atomicAdd(&mom[o * NMOM + k], acc[k]);
}

// A workgroup takes a tile of 256 columns x SH_ROWS rows of one image; a lane walks down one column, so it mostly stays inside one
// object and adds to 12 registers (background in between does not end the object).  A lane meeting another object adds the sums of
// the one it leaves directly.  What the lanes hold at the end is summed per object inside the wave (the first object here, the next
// three by wave_by_key); each wave's first object then meets those of the consecutive waves in LDS, so an image-sized object receives
// one atomic per sum and tile rather than one per pixel.
__global__ __launch_bounds__(SH_THREADS) void moments_kernel(const int* __restrict__ labels, int H, int W, const long long* __restrict__ offsets,
                                                             int64_t cap, const int* __restrict__ bbox, u64* __restrict__ mom) {
  __shared__ long long sh_obj[SH_THREADS / 64];
  __shared__ u64 sh_sum[SH_THREADS / 64][NMOM];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.z, xx = blockIdx.x * SH_THREADS + tid, yb = blockIdx.y * SH_ROWS;
  const int64_t img = (int64_t)b * H * W;
  int lab[SH_ROWS];
#pragma unroll
  for (int r = 0; r < SH_ROWS; ++r) lab[r] = (xx < W && yb + r < H) ? labels[img + (int64_t)(yb + r) * W + xx] : 0;
  // object_index's rule with the image's offset read once for the lane's 16 rows: calling it per row costs this kernel two more
  // VGPRs or a scalar load in every row
  const long long first = offsets[b];
  long long cur = -1;
  u64 x = 0;
  unsigned y0 = 0;
  u64 acc[NMOM];
#pragma unroll
  for (int k = 0; k < NMOM; ++k) acc[k] = 0;
#pragma unroll
  for (int r = 0; r < SH_ROWS; ++r) {
    if (lab[r] <= 0) continue;
    const long long obj = first + lab[r] - 1;
    if (obj >= cap) continue;
    if (obj != cur) {
      if (cur >= 0) flush_direct(mom, cur, acc);
#pragma unroll
      for (int k = 0; k < NMOM; ++k) acc[k] = 0;
      cur = obj;
      x = (u64)((unsigned)xx - (unsigned)bbox[4 * obj]), y0 = (unsigned)bbox[4 * obj + 1];
    }
    const u64 y = (unsigned)(yb + r) - y0;   // x, y >= 0 with the bbox mgu_object_stats wrote for these labels
    const u64 x2 = x * x, xy = x * y, y2 = y * y;
    acc[0] += x2, acc[1] += xy, acc[2] += y2;
    acc[3] += x2 * x, acc[4] += x2 * y, acc[5] += y2 * x, acc[6] += y2 * y;
    acc[7] += x2 * x2, acc[8] += x2 * xy, acc[9] += x2 * y2, acc[10] += xy * y2, acc[11] += y2 * y2;
  }
  bool pending = cur >= 0;
  {   // round 0: the wave's first object goes to LDS, where equal objects of consecutive waves are added before the atomic
    const unsigned long long act = __ballot(pending);
    const long long lo = act ? __shfl(cur, __ffsll((long long)act) - 1) : -1;
    const bool mine = pending && cur == lo;
    if (lane == 0) sh_obj[wave] = lo;
#pragma unroll
    for (int k = 0; k < NMOM; ++k) {
      const u64 s = wave_sum(mine ? acc[k] : 0ull);
      if (lane == 0) sh_sum[wave][k] = s;
    }
    if (mine) pending = false;
  }
  __syncthreads();
  if (tid < NMOM) {
    long long o = -1;
    u64 s = 0;
    for (int w = 0; w < SH_THREADS / 64; ++w) {
      if (sh_obj[w] != o) {
        if (o >= 0 && s) atomicAdd(&mom[o * NMOM + tid], s);
        o = sh_obj[w], s = 0;
      }
      s += sh_sum[w][tid];
    }
    if (o >= 0 && s) atomicAdd(&mom[o * NMOM + tid], s);
  }
  wave_by_key<3>(
      pending ? cur : -1,
      [=](long long lo, bool mine, bool lead) {
#pragma unroll
        for (int k = 0; k < NMOM; ++k) {
          const u64 s = wave_sum(mine ? acc[k] : 0ull);
          if (lead && s) atomicAdd(&mom[lo * NMOM + k], s);
        }
      },
      [=] { flush_direct(mom, cur, acc); });
}

// ---- second moments as exact integers -------------------------------------------------------------------------------------------
// With a = n u - sum u and b = n v - sum v (n times the centred coordinates), N20 = n sum u^2 - (sum u)^2 = (sum a^2) / n and N11, N02
// alike are integers, cov = N / (n (n - 1)) and its determinant is D / (n (n - 1))^2 with D = N20 N02 - N11^2: 0 EXACTLY for collinear
// pixels, where the difference of the fp64 eigenvalue formula would leave noise.  While n * max(w, h) < 2^30 every N fits 60 bits and
// D, like the per-pixel form N20 b^2 - 2 N11 a b + N02 a^2, fits __int128.
typedef __int128 i128;
struct Second {
  long long n, su, sv, n20, n11, n02;
  bool fits;
};
__device__ __forceinline__ Second second_moments(int64_t o, const long long* area, const int* bbox, const long long* sums, const u64* mom) {
  Second s;
  s.n = area[o];
  const int bx0 = bbox[4 * o], by0 = bbox[4 * o + 1];
  const long long ext = max(bbox[4 * o + 2] - bx0, bbox[4 * o + 3] - by0);
  s.fits = s.n > 0 && ext > 0 && ext < (1ll << 30) && s.n < (1ll << 30) / ext;
  s.su = sums[2 * o] - s.n * bx0, s.sv = sums[2 * o + 1] - s.n * by0;
  s.n20 = s.n11 = s.n02 = 0;
  if (s.fits) {
    const u64* q = mom + o * NMOM;
    s.n20 = s.n * (long long)q[0] - s.su * s.su, s.n11 = s.n * (long long)q[1] - s.su * s.sv, s.n02 = s.n * (long long)q[2] - s.sv * s.sv;
  }
  return s;
}
__device__ __forceinline__ double to_double(i128 v) {   // v >= 0; two roundings (no compiler-rt conversion on the device)
  return (double)(u64)((unsigned __int128)v >> 64) * 18446744073709551616.0 + (double)(u64)v;
}
// fixed-point scale of an object's residual sum: sum (m - 1)^2 <= sum m^2 + n < 4 n^2 (m <= n by the leverage bound), kept below 2^62
__device__ __forceinline__ int residual_shift(long long n) {
  const int bits = 64 - __clzll(n);
  return min(40, 60 - 2 * bits);
}
constexpr double THIN_RATIO = 256.0;   // (l1 + eps) / (l2 + eps) above which the term takes the per-pixel route

// One thread per object.  u = x - xmin, v = y - ymin; m[i][j] = sum u^i v^j as exact integers (orders 0 and 1 from area and sums),
// mu[i][j] the central moments by the binomial shift, everything in fp64.  The closed form of the term loses digits as
// ((l1 + eps) / (l2 + eps))^2 eps_fp64 -- the inverse's entries grow and the fourth-order sums must cancel -- so it is kept up to a
// ratio of THIN_RATIO (error below 1e-11); a thinner object (at the limit a one-pixel diagonal line: singular cov, entries 1 / eps)
// gets term = NaN here, which residual_kernel and residual_finish_kernel replace.
__global__ __launch_bounds__(SH_THREADS) void shapes_kernel(const long long* __restrict__ offsets, int B, int64_t cap, const long long* __restrict__ area,
                                                            const int* __restrict__ bbox, const long long* __restrict__ sums,
                                                            const u64* __restrict__ mom, double eps, int min_pixels, float* __restrict__ centroid,
                                                            float* __restrict__ cov, float* __restrict__ axes, float* __restrict__ angle,
                                                            float* __restrict__ fill, float* __restrict__ term, unsigned char* __restrict__ status,
                                                            u64* __restrict__ racc) {
  const int64_t N = objects_recorded(offsets, B, cap);
  for (int64_t o = (int64_t)blockIdx.x * SH_THREADS + threadIdx.x; o < N; o += (int64_t)gridDim.x * SH_THREADS) {
    const long long n = area[o];
    const int bx0 = bbox[4 * o], by0 = bbox[4 * o + 1], bw = bbox[4 * o + 2] - bx0, bh = bbox[4 * o + 3] - by0;
    const double dn = (double)n;
    float out[10] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // centroid 2, cov 3, axes 2, angle, fill, term
    unsigned char st = 0;
    if (n > 0) out[0] = (float)((double)sums[2 * o] / dn), out[1] = (float)((double)sums[2 * o + 1] / dn);
    // exact while area * (max(w, h) - 1)^4 < 2^64: every one of the 12 sums is at most that product
    const u64 ext = (u64)(max(bw, bh) > 0 ? max(bw, bh) - 1 : 0);
    if (n < (long long)min_pixels || n < 2) st = 1;
    else if (ext >= 65536ull || (ext > 0 && (u64)n > ULLONG_MAX / (ext * ext * ext * ext))) st = 2;
    if (st == 0) {
      double m[5][5];
      for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) m[i][j] = 0.0;
      const u64* q = mom + o * NMOM;
      m[0][0] = dn;
      m[1][0] = (double)(sums[2 * o] - n * bx0), m[0][1] = (double)(sums[2 * o + 1] - n * by0);
      m[2][0] = (double)q[0], m[1][1] = (double)q[1], m[0][2] = (double)q[2];
      m[3][0] = (double)q[3], m[2][1] = (double)q[4], m[1][2] = (double)q[5], m[0][3] = (double)q[6];
      m[4][0] = (double)q[7], m[3][1] = (double)q[8], m[2][2] = (double)q[9], m[1][3] = (double)q[10], m[0][4] = (double)q[11];
      const double ub = m[1][0] / dn, vb = m[0][1] / dn;
      const double binom[5][5] = {{1, 0, 0, 0, 0}, {1, 1, 0, 0, 0}, {1, 2, 1, 0, 0}, {1, 3, 3, 1, 0}, {1, 4, 6, 4, 1}};
      double pu[5], pv[5];   // (-ub)^k, (-vb)^k
      pu[0] = pv[0] = 1.0;
      for (int k = 1; k < 5; ++k) pu[k] = pu[k - 1] * -ub, pv[k] = pv[k - 1] * -vb;
      double mu[5][5];
      for (int i = 0; i < 5; ++i)
        for (int j = 0; i + j < 5; ++j) {
          double s = 0.0;
          for (int k = 0; k <= i; ++k)
            for (int l = 0; l <= j; ++l) s += binom[i][k] * binom[j][l] * pu[i - k] * pv[j - l] * m[k][l];
          mu[i][j] = s;
        }
      const double d1 = dn - 1.0;
      double cxx = mu[2][0] / d1, cyy = mu[0][2] / d1, cxy = mu[1][1] / d1, cdet;
      const Second sm2nd = second_moments(o, area, bbox, sums, mom);
      if (sm2nd.fits) {
        const double c = dn * d1;
        cxx = (double)sm2nd.n20 / c, cxy = (double)sm2nd.n11 / c, cyy = (double)sm2nd.n02 / c;
        cdet = to_double((i128)sm2nd.n20 * sm2nd.n02 - (i128)sm2nd.n11 * sm2nd.n11) / (c * c);
      } else {
        cdet = fmax(cxx * cyy - cxy * cxy, 0.0);
      }
      if (cxy == 0.0) cxy = 0.0;   // -0 -> +0: atan2(-0, negative) would be -pi
      const double half_d = 0.5 * (cxx - cyy), rad = sqrt(half_d * half_d + cxy * cxy);
      const double l1 = 0.5 * (cxx + cyy) + rad, l2 = l1 > 0.0 ? cdet / l1 : 0.0;
      const double a = 2.0 * sqrt(fmax(l1, 0.0)), bb = 2.0 * sqrt(l2);
      const double th = 0.5 * atan2(2.0 * cxy, cxx - cyy);
      const double fl = bb > 0.0 ? dn / (3.14159265358979323846 * a * bb) : 0.0;
      double t;
      if (sm2nd.fits && l1 + eps > THIN_RATIO * (l2 + eps)) {
        t = __builtin_nan("");
      } else {
        // inverse of [[cyy + eps, cxy], [cxy, cxx + eps]] (row, column order of the reference's coordinates)
        const double sxx = cxx + eps, syy = cyy + eps, det = sxx * syy - cxy * cxy;
        const double iyy = sxx / det, ixx = syy / det, ixy = -cxy / det;
        const double sm = iyy * mu[0][2] + 2.0 * ixy * mu[1][1] + ixx * mu[2][0];
        const double sm2 = iyy * iyy * mu[0][4] + ixx * ixx * mu[4][0] + (4.0 * ixy * ixy + 2.0 * iyy * ixx) * mu[2][2] +
                           4.0 * iyy * ixy * mu[1][3] + 4.0 * ixx * ixy * mu[3][1];
        t = (sm2 - 2.0 * sm + dn) / dn;
      }
      out[2] = (float)cxx, out[3] = (float)cxy, out[4] = (float)cyy;
      out[5] = (float)a, out[6] = (float)bb, out[7] = (float)th, out[8] = (float)fl, out[9] = (float)t;
    }
    centroid[2 * o] = out[0], centroid[2 * o + 1] = out[1];
    cov[3 * o] = out[2], cov[3 * o + 1] = out[3], cov[3 * o + 2] = out[4];
    axes[2 * o] = out[5], axes[2 * o + 1] = out[6];
    angle[o] = out[7], fill[o] = out[8], term[o] = out[9], status[o] = st;
    racc[o] = 0;
  }
}

// The per-pixel route of a thin object (term[o] is NaN): one thread per pixel evaluates m = d^T (cov + eps I)^-1 d as
// (Q + eps |d|^2) / det' with Q = (N20 b^2 - 2 N11 a b + N02 a^2) / (n^3 (n - 1)) from exact integers -- for collinear pixels Q is
// 0 exactly, where an fp64 product with the 1 / eps entries of the inverse would be noise -- and det' = D / (n (n - 1))^2 +
// eps tr(cov) + eps^2, a sum of non-negative terms.  (m - 1)^2 is added as round(. * 2^shift) with uint64 integer atomics (the lanes
// of one object summed inside the wave first): a pure function of each pixel and an order-free sum, so bitwise repeatable.
__global__ __launch_bounds__(SH_THREADS) void residual_kernel(const int* __restrict__ labels, int W, int64_t HW, int64_t n,
                                                              const long long* __restrict__ offsets, int64_t cap, const long long* __restrict__ area,
                                                              const int* __restrict__ bbox, const long long* __restrict__ sums,
                                                              const u64* __restrict__ mom, double eps, const float* __restrict__ term,
                                                              u64* __restrict__ racc) {
  const int64_t g = (int64_t)blockIdx.x * SH_THREADS + threadIdx.x;
  long long obj = -1;
  u64 qv = 0;
  if (g < n) {
    const int lab = labels[g];
    const int64_t b = g / HW, i = g - b * HW;
    obj = object_index(lab, offsets, b, cap);
    if (obj >= 0 && term[obj] == term[obj]) obj = -1;   // only objects whose term is NaN
    if (obj >= 0) {
      const Second s = second_moments(obj, area, bbox, sums, mom);
      const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
      const long long a = s.n * (x - bbox[4 * obj]) - s.su, bq = s.n * (y - bbox[4 * obj + 1]) - s.sv;
      const i128 qs = (i128)s.n20 * bq * bq - 2 * (i128)s.n11 * a * bq + (i128)s.n02 * a * a;
      const double dn = (double)s.n, c = dn * (dn - 1.0);
      const double tr = ((double)s.n20 + (double)s.n02) / c;
      const double det = to_double((i128)s.n20 * s.n02 - (i128)s.n11 * s.n11) / (c * c) + eps * tr + eps * eps;
      const double r2 = ((double)a * (double)a + (double)bq * (double)bq) / (dn * dn);
      const double m = (to_double(qs) / (c * dn * dn) + eps * r2) / det;
      qv = __double2ull_rn(fmin((m - 1.0) * (m - 1.0) * (double)(1ull << residual_shift(s.n)), 4.0e18));
    }
  }
  wave_by_key(
      obj,
      [=](long long lo, bool mine, bool lead) {
        const u64 sum = wave_sum(mine ? qv : 0ull);
        if (lead) atomicAdd(&racc[lo], sum);
      },
      [=] { atomicAdd(&racc[obj], qv); });
}

__global__ __launch_bounds__(SH_THREADS) void residual_finish_kernel(const long long* __restrict__ offsets, int B, int64_t cap,
                                                                     const long long* __restrict__ area, const u64* __restrict__ racc,
                                                                     float* __restrict__ term) {
  const int64_t N = objects_recorded(offsets, B, cap);
  for (int64_t o = (int64_t)blockIdx.x * SH_THREADS + threadIdx.x; o < N; o += (int64_t)gridDim.x * SH_THREADS)
    if (term[o] != term[o]) term[o] = (float)((double)racc[o] / (double)(1ull << residual_shift(area[o])) / (double)area[o]);
}

// One workgroup: thread t adds the terms of objects t, t + 256, ... in index order, then a fixed tree over the 256 partial sums
__global__ __launch_bounds__(SH_THREADS) void shape_loss_kernel(const long long* __restrict__ offsets, int B, int64_t cap, const float* __restrict__ term,
                                                                const unsigned char* __restrict__ status, const long long* __restrict__ cls,
                                                                long long keep, float* __restrict__ loss) {
  __shared__ double ssum[SH_THREADS];
  __shared__ long long scnt[SH_THREADS];
  const int64_t N = objects_recorded(offsets, B, cap);
  double s = 0.0;
  long long cnt = 0;
  for (int64_t o = threadIdx.x; o < N; o += SH_THREADS)
    if (status[o] == 0 && (!cls || cls[o] == keep)) s += (double)term[o], ++cnt;
  ssum[threadIdx.x] = s, scnt[threadIdx.x] = cnt;
  __syncthreads();
  for (int off = SH_THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) ssum[threadIdx.x] += ssum[threadIdx.x + off], scnt[threadIdx.x] += scnt[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) *loss = scnt[0] > 0 ? (float)(ssum[0] / (double)scnt[0]) : 0.f;
}

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_object_moments(mgu_ctx* c, const int32_t* labels_dev, int B, int H, int W, const int64_t* offsets_dev, int64_t capacity,
                       const int32_t* bbox_dev, uint64_t* moments_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !offsets_dev || B < 0 || H < 0 || W < 0 || capacity < 0 || (capacity > 0 && (!bbox_dev || !moments_dev)))
    return fail(c, MGU_ERR_INVALID, "bad object_moments args (null pointer or negative size)");
  if (int rc = check_pixel_count(c, "object_moments", B, H, W)) return rc;
  if (B > 65535 || (H + SH_ROWS - 1) / SH_ROWS > 65535) return fail(c, MGU_ERR_INVALID, "object_moments: at most 65535 images and %d rows per call", 65535 * SH_ROWS);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (capacity == 0) return MGU_OK;
  const int64_t n = (int64_t)B * H * W;
  const long long* off = (const long long*)offsets_dev;
  const unsigned initblocks = grid_for(capacity * NMOM, SH_THREADS, 1024);
  hipLaunchKernelGGL(moments_init_kernel, dim3(initblocks), dim3(SH_THREADS), 0, s, off, B, capacity, (u64*)moments_dev);
  if (n > 0)
    hipLaunchKernelGGL(moments_kernel, dim3((W + SH_THREADS - 1) / SH_THREADS, (H + SH_ROWS - 1) / SH_ROWS, B), dim3(SH_THREADS), 0, s, labels_dev, H, W,
                       off, capacity, bbox_dev, (u64*)moments_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_object_shapes(mgu_ctx* c, const int32_t* labels_dev, int B, int H, int W, const int64_t* offsets_dev, int64_t capacity,
                      const int64_t* area_dev, const int32_t* bbox_dev, const int64_t* sums_dev, const uint64_t* moments_dev, float epsilon,
                      int min_pixels, float* centroid_dev, float* cov_dev, float* axes_dev, float* angle_dev, float* fill_dev, float* term_dev,
                      uint8_t* status_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev || !offsets_dev || B < 0 || H < 0 || W < 0 || capacity < 0)
    return fail(c, MGU_ERR_INVALID, "bad object_shapes args (null labels or offsets, or negative size)");
  if (capacity > 0 && (!area_dev || !bbox_dev || !sums_dev || !moments_dev || !centroid_dev || !cov_dev || !axes_dev || !angle_dev || !fill_dev ||
                       !term_dev || !status_dev))
    return fail(c, MGU_ERR_INVALID, "object_shapes: every per-object array is needed for a nonzero capacity");
  if (!(epsilon >= 0.f)) return fail(c, MGU_ERR_INVALID, "object_shapes: epsilon must be >= 0");
  if (min_pixels < 0) return fail(c, MGU_ERR_INVALID, "object_shapes: min_pixels must be >= 0");
  if (int rc = check_pixel_count(c, "object_shapes", B, H, W)) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  if (capacity == 0) return MGU_OK;
  int rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)capacity * 8);
  if (rc) return rc;
  u64* racc = (u64*)c->objws;
  hipStream_t s = (hipStream_t)hip_stream;
  const long long* off = (const long long*)offsets_dev;
  const int64_t HW = (int64_t)H * W, n = (int64_t)B * HW;
  const unsigned blocks = grid_for(capacity, SH_THREADS, 1024);
  hipLaunchKernelGGL(shapes_kernel, dim3(blocks), dim3(SH_THREADS), 0, s, off, B, capacity, (const long long*)area_dev, bbox_dev,
                     (const long long*)sums_dev, (const u64*)moments_dev, (double)epsilon, min_pixels, centroid_dev, cov_dev, axes_dev, angle_dev,
                     fill_dev, term_dev, status_dev, racc);
  if (n > 0)
    hipLaunchKernelGGL(residual_kernel, dim3(grid_for(n, SH_THREADS, INT_MAX)), dim3(SH_THREADS), 0, s, labels_dev, W, HW, n, off, capacity,
                       (const long long*)area_dev, bbox_dev, (const long long*)sums_dev, (const u64*)moments_dev, (double)epsilon, term_dev, racc);
  hipLaunchKernelGGL(residual_finish_kernel, dim3(blocks), dim3(SH_THREADS), 0, s, off, B, capacity, (const long long*)area_dev, racc, term_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_elliptical_shape_loss_objects(mgu_ctx* c, int B, const int64_t* offsets_dev, int64_t capacity, const float* term_dev,
                                      const uint8_t* status_dev, const int64_t* class_dev, int64_t keep_class, float* loss_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!offsets_dev || !loss_dev || B < 0 || capacity < 0 || (capacity > 0 && (!term_dev || !status_dev)))
    return fail(c, MGU_ERR_INVALID, "bad elliptical_shape_loss_objects args (null pointer or negative size)");
  HIPCHK(c, hipSetDevice(c->device));
  hipLaunchKernelGGL(shape_loss_kernel, dim3(1), dim3(SH_THREADS), 0, (hipStream_t)hip_stream, (const long long*)offsets_dev, B, capacity, term_dev,
                     status_dev, (const long long*)class_dev, (long long)keep_class, loss_dev);
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
