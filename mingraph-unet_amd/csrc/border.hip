// The U-Net border weight map on the device (Ronneberger et al., MICCAI 2015, eq. 2): for every pixel the exact squared distances to
// the nearest and to the second-nearest OBJECT of an int32 instance map, the nearest object's label, the weight
//   w = class_weight[cls] + w0 exp(-(sqrt(d1sq) + sqrt(d2sq))^2 / (2 sigma^2))
// and the class map with touching instances separated by one pixel (include/mgunet.h states the definitions).
//   mgu_border_weights   labels (B, H, W) -> d1sq, d2sq, nearest, weight, target (each optional)
// The distances are integers throughout and the weight is one fp64 expression of them rounded to fp32 once: every output is a pure
// function of the input, bitwise repeatable.  Two launches, whatever B, the objects and the outputs asked for:
// (1) columns: a lane per column scans down, then up.  A scan carries the last two runs of DISTINCT labels it met, (a1, y1) the
//     newer: a labelled pixel with l == a1 refreshes y1, any other label pushes (a1, y1) to the second slot and takes the first.  Per
//     pixel the best two entries with distinct labels among the up to four candidates, in (g, label) order, go to scratch as
//     (g1, a1, g2, a2), g the vertical distance (G_NONE: no entry).  A label that is not among a column's two best distinct labels has
//     two other labels at least as near in that column, so it is not among the pixel's two best overall: two per column suffice.
// (2) rows: a workgroup per row keeps the row's (g1^2, a1, g2^2, a2) in LDS, 16 bytes per pixel read and written as one 16-byte word
//     per lane (consecutive lanes on consecutive words: no bank conflict), and every pixel walks outward over x -+ dx, merging both
//     candidates of each column into its running best two distinct, until dx^2 passes the current d2sq (a candidate at dx^2 == d2sq
//     can still win the tie on `nearest`, so the walk stops one step after d2sq is reached) or both sides have left the row.  The
//     weight and the target are formed in the same kernel.  An image with fewer than two objects never bounds d2sq: every pixel
//     walks its whole row, O(W^2) per row (README.md carries the measured cost).
// Limits: H, W <= 16384 (every real distance stays below MGU_D2_NONE) and W * 16 bytes within the LDS one workgroup may take
// (10240 pixels at 160 KiB); B <= 65535; B*H*W < 2^31.  Scratch: 16 bytes per pixel of the context's object workspace.
#include "objects_common.h"

namespace mgu {
namespace {

constexpr int BW_THREADS = 256;
constexpr int BW_COL_BATCH = 8;              // rows whose loads the column scan issues at once
constexpr int BW_MAX_DIM = 16384;
constexpr int BW_G_NONE = 32768;             // column distance "no entry"; its square is MGU_D2_NONE
static_assert((long long)BW_G_NONE * BW_G_NONE == MGU_D2_NONE, "the sentinel is the square of the column sentinel");

// the two nearest entries with distinct labels, in (d, label) order; an empty slot is (MGU_D2_NONE or BW_G_NONE, 0)
struct Best2 {
  int d1, l1, d2, l2;
};
__device__ __forceinline__ bool bw_before(int d, int l, int d0, int l0) { return d < d0 || (d == d0 && l < l0); }
// merge the entry (d, l), l != 0: a label already held keeps its smaller distance, a new one takes the place its pair earns
__device__ __forceinline__ void bw_merge(Best2& b, int d, int l) {
  if (l == b.l1) {
    b.d1 = min(b.d1, d);
  } else if (l == b.l2) {
    if (d < b.d2) {
      b.d2 = d;
      if (bw_before(b.d2, b.l2, b.d1, b.l1)) {
        const int td = b.d1, tl = b.l1;
        b.d1 = b.d2, b.l1 = b.l2, b.d2 = td, b.l2 = tl;
      }
    }
  } else if (bw_before(d, l, b.d1, b.l1)) {
    b.d2 = b.d1, b.l2 = b.l1, b.d1 = d, b.l1 = l;
  } else if (bw_before(d, l, b.d2, b.l2)) {
    b.d2 = d, b.l2 = l;
  }
}

// the last two runs of distinct labels a column scan has met
struct Runs {
  int a1 = 0, y1 = 0, a2 = 0, y2 = 0;
  __device__ __forceinline__ void step(int l, int y) {
    if (l == 0) return;
    if (l == a1) {
      y1 = y;
    } else {
      a2 = a1, y2 = y1, a1 = l, y1 = y;
    }
  }
};

// (1) columns: lane = column x of image blockIdx.y; cols[pixel] = (g1, a1, g2, a2)
__global__ __launch_bounds__(64) void bw_col_kernel(const int* __restrict__ labels, int H, int W, int4* __restrict__ cols) {
  const int x = blockIdx.x * 64 + threadIdx.x;
  if (x >= W) return;
  const int64_t base = (int64_t)blockIdx.y * H * W + x;
  // the scan is one dependent chain per lane, so the loads of BW_COL_BATCH rows are issued together ahead of it
  Runs r;
  for (int y0 = 0; y0 < H; y0 += BW_COL_BATCH) {   // down: the runs above, the newer one is the nearer
    int l[BW_COL_BATCH];
#pragma unroll
    for (int k = 0; k < BW_COL_BATCH; ++k) l[k] = y0 + k < H ? labels[base + (int64_t)(y0 + k) * W] : 0;
#pragma unroll
    for (int k = 0; k < BW_COL_BATCH; ++k) {
      const int y = y0 + k;
      if (y < H) {
        r.step(l[k], y);
        cols[base + (int64_t)y * W] = make_int4(r.a1 ? y - r.y1 : BW_G_NONE, r.a1, r.a2 ? y - r.y2 : BW_G_NONE, r.a2);
      }
    }
  }
  r = Runs();
  for (int y0 = H - 1; y0 >= 0; y0 -= BW_COL_BATCH) {   // up: the runs below, merged into what the way down left
    int l[BW_COL_BATCH];
    int4 v[BW_COL_BATCH];
#pragma unroll
    for (int k = 0; k < BW_COL_BATCH; ++k) {   // every entry of the batch is read before any of them is written
      const bool in = y0 - k >= 0;
      l[k] = in ? labels[base + (int64_t)(y0 - k) * W] : 0;
      v[k] = in ? cols[base + (int64_t)(y0 - k) * W] : make_int4(0, 0, 0, 0);
    }
#pragma unroll
    for (int k = 0; k < BW_COL_BATCH; ++k) {
      const int y = y0 - k;
      if (y >= 0) {
        r.step(l[k], y);
        Best2 b{v[k].x, v[k].y, v[k].z, v[k].w};
        if (r.a1) bw_merge(b, r.y1 - y, r.a1);
        if (r.a2) bw_merge(b, r.y2 - y, r.a2);
        cols[base + (int64_t)y * W] = make_int4(b.d1, b.l1, b.d2, b.l2);
      }
    }
  }
}

struct BwOut {
  const int* labels;
  const long long* classes;     // or nullptr
  const float* class_weight;    // or nullptr
  int num_classes;
  double w0, two_s2;            // 2 sigma^2
  long long background;
  int* d1sq;
  int* d2sq;
  int* nearest;
  float* weight;
  long long* target;
};

// (2) rows: workgroup = row blockIdx.x of image blockIdx.y; LDS: (g1^2, a1, g2^2, a2) [W]
__global__ __launch_bounds__(BW_THREADS) void bw_row_kernel(const int4* __restrict__ cols, int H, int W, BwOut o) {
#pragma clang fp contract(off)   // the weight is the header's expression, operation by operation
  extern __shared__ int4 bw_row[];
  const int y = blockIdx.x;
  const int64_t img = (int64_t)blockIdx.y * H * W, row = img + (int64_t)y * W;
  for (int x = threadIdx.x; x < W; x += BW_THREADS) {
    int4 v = cols[row + x];
    v.x *= v.x, v.z *= v.z;
    bw_row[x] = v;
  }
  __syncthreads();
  for (int x = threadIdx.x; x < W; x += BW_THREADS) {
    const int4 own = bw_row[x];
    Best2 b{own.x, own.y, own.z, own.w};
    for (int dx = 1;; ++dx) {   // outward from x; a column farther than sqrt(d2sq) changes neither distance nor the nearest label
      const int dd = dx * dx, xl = x - dx, xr = x + dx;
      if (dd > b.d2 || (xl < 0 && xr >= W)) break;
      // an entry farther than d2sq changes nothing (one AT d2sq may still win a tie), and a column's second entry is no nearer
      // than its first; an empty entry (MGU_D2_NONE) is always farther
      if (xl >= 0) {
        const int4 v = bw_row[xl];
        if (dd + v.x <= b.d2) {
          bw_merge(b, dd + v.x, v.y);
          if (dd + v.z <= b.d2) bw_merge(b, dd + v.z, v.w);
        }
      }
      if (xr < W) {
        const int4 v = bw_row[xr];
        if (dd + v.x <= b.d2) {
          bw_merge(b, dd + v.x, v.y);
          if (dd + v.z <= b.d2) bw_merge(b, dd + v.z, v.w);
        }
      }
    }
    const int64_t i = row + x;
    if (o.d1sq) o.d1sq[i] = b.d1;
    if (o.d2sq) o.d2sq[i] = b.d2;
    if (o.nearest) o.nearest[i] = b.l1;
    const long long cls = o.classes ? o.classes[i] : 0;
    if (o.weight) {
      double cw = 1.0;
      if (o.classes && o.class_weight) cw = (cls >= 0 && cls < o.num_classes) ? (double)o.class_weight[cls] : 0.0;
      double e = 0.0;
      if (b.d2 < MGU_D2_NONE) {
        const double s = sqrt((double)b.d1) + sqrt((double)b.d2);
        e = o.w0 * exp(-(s * s) / o.two_s2);
      }
      o.weight[i] = (float)(cw + e);
    }
    if (o.target) {   // an object pixel with a 4-neighbour of another object becomes background
      const int l = o.labels[i];
      bool touch = false;
      if (l != 0) {
        int n;
        if (x > 0 && (n = o.labels[i - 1]) != 0 && n != l) touch = true;
        if (x + 1 < W && (n = o.labels[i + 1]) != 0 && n != l) touch = true;
        if (y > 0 && (n = o.labels[i - W]) != 0 && n != l) touch = true;
        if (y + 1 < H && (n = o.labels[i + W]) != 0 && n != l) touch = true;
      }
      o.target[i] = touch ? o.background : cls;
    }
  }
}

bool g_bw_row_lds[64];

}  // namespace
}  // namespace mgu

using namespace mgu;
using namespace mgud;

extern "C" {

int mgu_border_weights(mgu_ctx* c, const int32_t* labels_dev, int B, int H, int W, const int64_t* classes_dev, const float* class_weight_dev,
                       int num_classes, double w0, double sigma, int64_t background_class, int32_t* d1sq_dev, int32_t* d2sq_dev,
                       int32_t* nearest_dev, float* weight_dev, int64_t* target_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!labels_dev) return fail(c, MGU_ERR_INVALID, "bad border_weights args (labels_dev is NULL)");
  if (B < 1 || H < 1 || W < 1) return fail(c, MGU_ERR_INVALID, "border_weights: a shape without pixels");
  if (!(sigma > 0.0)) return fail(c, MGU_ERR_INVALID, "border_weights: sigma must be > 0");
  if (!(w0 >= 0.0)) return fail(c, MGU_ERR_INVALID, "border_weights: w0 must be >= 0");
  if (target_dev && !classes_dev) return fail(c, MGU_ERR_INVALID, "border_weights: target_dev needs classes_dev");
  if (class_weight_dev && (num_classes < 1 || num_classes > 8))
    return fail(c, MGU_ERR_INVALID, "border_weights: class weights take 1 <= num_classes <= 8");
  if (H > BW_MAX_DIM || W > BW_MAX_DIM) return fail(c, MGU_ERR_INVALID, "border_weights: H and W at most %d", BW_MAX_DIM);
  if (B > 65535) return fail(c, MGU_ERR_INVALID, "border_weights: at most 65535 images per call");
  int rc = check_pixel_count(c, "border_weights", B, H, W);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  const size_t lds = (size_t)W * sizeof(int4);
  if (lds > 65536) {   // the opt-in is set once per device: for the widest row the device takes, not for this call's
    int budget = 0;
    HIPCHK(c, hipDeviceGetAttribute(&budget, hipDeviceAttributeMaxSharedMemoryPerBlock, c->device));
    if (lds > (size_t)budget)
      return fail(c, MGU_ERR_INVALID, "border_weights: a row of %d pixels needs %zu bytes of LDS, the device gives one workgroup %d", W, lds, budget);
    HIPCHK(c, ensure_dyn_lds((const void*)bw_row_kernel, std::min((size_t)BW_MAX_DIM * sizeof(int4), (size_t)budget), g_bw_row_lds));
  }
  const int64_t n = (int64_t)B * H * W;
  rc = ensure(c, &c->objws, &c->objws_bytes, (size_t)n * sizeof(int4));
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  int4* cols = (int4*)c->objws;
  BwOut o;
  o.labels = labels_dev, o.classes = (const long long*)classes_dev, o.class_weight = class_weight_dev, o.num_classes = num_classes;
  o.w0 = w0, o.two_s2 = 2.0 * sigma * sigma, o.background = background_class;
  o.d1sq = d1sq_dev, o.d2sq = d2sq_dev, o.nearest = nearest_dev, o.weight = weight_dev, o.target = (long long*)target_dev;
  {
    ProfScope ps(c, s, "border_weights columns");
    hipLaunchKernelGGL(bw_col_kernel, dim3((W + 63) / 64, B), dim3(64), 0, s, labels_dev, H, W, cols);
  }
  {
    ProfScope ps(c, s, "border_weights rows");
    hipLaunchKernelGGL(bw_row_kernel, dim3(H, B), dim3(BW_THREADS), lds, s, cols, H, W, o);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
