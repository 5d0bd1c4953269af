// Elastic deformation folded into the scale / crop / colour pass (include/mgunet.h, "elastic deformation": THIS BUILD'S DEFINITION,
// integers only up to the final ToTensor + Normalize): a displacement field interpolated from a coarse grid of control nodes by the
// uniform cubic B-spline is one more term of the source coordinate of mgu_augment_affine_color; everything behind the coordinate is that
// entry's definition, and the image is still resampled once.
//   elastic_color_kernel   one launch for the images, the uint8 masks and the int32 instance labels of the whole batch
//   elastic_field_kernel   the displacement field alone, int32 (B, 2, H, W)
// Both walk 32 x 32 result tiles as affine_color_kernel does and form a tile's field in three steps in LDS (elastic_tile_field): the
// control nodes the tile spans, the row sums q over the four lattice rows of each tile row, and per pixel four taps of q per plane.  The
// sums are exact in int64, so factoring them changes no bit.  The Q14 weight table is built once per workgroup from its integer formula.
#include <algorithm>

#include "augment_affine.h"

namespace mgu {

constexpr int EL_MIN_NODES = 4, EL_MAX_NODES = 32;
constexpr int EL_QP = AFF_TX + 1;   // pitch of a row of q (8-byte words): 33, so that the eight tile rows of a wave start on different banks

struct ElasticLds {
  int w[256][4];                                // Wq[t][0..3], Q14, rows sum to 16384
  int c[2][EL_MAX_NODES][EL_MAX_NODES];         // the nodes the tile spans, [plane][row - j_lo][column - i_lo]: at most 8 KiB
  long long q[2][AFF_TY][EL_QP];                // q[plane][tile row][column - i_lo] = sum_b Wq[s][b] c[j + b][column]
};

// Wq[t] for t = threadIdx.x of a 256-thread workgroup.  T = 256, D = 6 T^3: n0 = (T - t)^3, n1 = 3 t^3 - 6 T t^2 + 4 T^3,
// n2 = -3 t^3 + 3 T t^2 + 3 T^2 t + T^3, n3 = t^3 (all >= 0, sum D); w_k = (2 * 16384 n_k + D) / (2 D), and the larger of w1, w2
// (w1 on a tie) takes what is missing from 16384.
__device__ __forceinline__ void elastic_weights(ElasticLds& L) {
  const long long T = 256, t = (long long)threadIdx.x, T3 = T * T * T, D = 6 * T3;
  const long long n[4] = {(T - t) * (T - t) * (T - t), 3 * t * t * t - 6 * T * t * t + 4 * T3, -3 * t * t * t + 3 * T * t * t + 3 * T * T * t + T3,
                          t * t * t};
  int w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) w[k] = (int)((unsigned long long)(2 * 16384 * n[k] + D) / (unsigned long long)(2 * D));
  const int rem = 16384 - (w[0] + w[1] + w[2] + w[3]);
  if (w[2] > w[1]) w[2] += rem;
  else w[1] += rem;
  *(int4*)L.w[threadIdx.x] = make_int4(w[0], w[1], w[2], w[3]);
}

// The displacements (dx, dy)[k] of the pixels (x0 + k, y), k < AFF_XV, of the tile at (tx0, ty0), x0 = tx0 + lx, y = ty0 + ly, of an
// image with the control nodes cb (2, gh, gw).  Every thread of the workgroup calls it (it holds three barriers); the values of a
// pixel outside the W x H result are those of the last pixel of its row / column and are not to be used.
__device__ __forceinline__ void elastic_tile_field(ElasticLds& L, const int* __restrict__ cb, int gh, int gw, int su, int sv, int tx0, int ty0,
                                                   int H, int W, int lx, int ly, long long (&dx)[AFF_XV], long long (&dy)[AFF_XV]) {
  // u = x su + (su >> 1) < W su <= (gw - 3) 2^16: an int holds it (the definition's int64 gives the same value)
  const int i_lo = (tx0 * su + (su >> 1)) >> 16, i_hi = (min(tx0 + AFF_TX - 1, W - 1) * su + (su >> 1)) >> 16;
  const int j_lo = (ty0 * sv + (sv >> 1)) >> 16, j_hi = (min(ty0 + AFF_TY - 1, H - 1) * sv + (sv >> 1)) >> 16;
  const int nc = i_hi - i_lo + 4, nr = j_hi - j_lo + 4;   // i_hi <= gw - 4, j_hi <= gh - 4: at most gw x gh nodes, all of them inside
  __syncthreads();                                         // the previous tile's readers are done
  for (int e = (int)threadIdx.x; e < 2 * nr * EL_MAX_NODES; e += 256) {
    const int ic = e % EL_MAX_NODES, jr = (e / EL_MAX_NODES) % nr, pl = e / (EL_MAX_NODES * nr);
    if (ic < nc) L.c[pl][jr][ic] = cb[(pl * gh + j_lo + jr) * gw + i_lo + ic];
  }
  __syncthreads();
  {   // row sums: 8 threads a tile row, columns ic = (tid & 7) + 8 m
    const int ry = (int)threadIdx.x >> 3, v = min(ty0 + ry, H - 1) * sv + (sv >> 1);
    const int jr = (v >> 16) - j_lo, s = (v >> 8) & 255;
    const int4 ws = *(const int4*)L.w[s];
#pragma unroll
    for (int m = 0; m < EL_MAX_NODES / 8; ++m) {
      const int ic = ((int)threadIdx.x & 7) + 8 * m;
      if (ic < nc) {
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
          L.q[pl][ry][ic] = (long long)ws.x * L.c[pl][jr][ic] + (long long)ws.y * L.c[pl][jr + 1][ic] + (long long)ws.z * L.c[pl][jr + 2][ic] +
                            (long long)ws.w * L.c[pl][jr + 3][ic];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < AFF_XV; ++k) {
    const int u = min(tx0 + lx + k, W - 1) * su + (su >> 1);
    const int ic = (u >> 16) - i_lo, t = (u >> 8) & 255;
    const int4 wt = *(const int4*)L.w[t];
    const long long* q0 = &L.q[0][ly][ic];
    const long long* q1 = &L.q[1][ly][ic];
    const long long ax = wt.x * q0[0] + wt.y * q0[1] + wt.z * q0[2] + wt.w * q0[3];   // |acc| < 2^54
    const long long ay = wt.x * q1[0] + wt.y * q1[1] + wt.z * q1[2] + wt.w * q1[3];
    dx[k] = (ax + (1ll << 27)) >> 28;
    dy[k] = (ay + (1ll << 27)) >> 28;
  }
}

// affine_color_kernel with the displacement of the pixel added to its source coordinates and the int32 labels sampled beside the
// mask.  ctrl == nullptr: no displacement (the affine result).  One thread: AFF_XV consecutive x of one output row of one image.
// VEC: as there, and labels_out 16-byte aligned.
template <bool VEC>
__global__ __launch_bounds__(256) void elastic_color_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                            const int* __restrict__ labels, int B, int Hs, int Ws, int bgr, int num_classes,
                                                            float* __restrict__ out, int H, int W, AffStrides so, AffNorm nm, int fill0, int fill1,
                                                            int fill2, int64_t* __restrict__ mask_out, int64_t mask_fill,
                                                            int* __restrict__ labels_out, int label_fill, const int* __restrict__ params,
                                                            const unsigned long long* __restrict__ sums, const int* __restrict__ ctrl, int gh,
                                                            int gw) {
  __shared__ ElasticLds L;
  const unsigned tiles_x = (unsigned)((W + AFF_TX - 1) / AFF_TX), tiles_y = (unsigned)((H + AFF_TY - 1) / AFF_TY);
  const unsigned total = (unsigned)B * tiles_y * tiles_x;   // < 2^31 (checked on the host)
  const int lx = (int)(threadIdx.x % (AFF_TX / AFF_XV)) * AFF_XV, ly = (int)(threadIdx.x / (AFF_TX / AFF_XV));
  const int fill[3] = {fill0, fill1, fill2};
  const int row = Ws * 3;
  const uint8_t* img_end = img + (int64_t)B * Hs * row;
  int su = 0, sv = 0;
  if (ctrl) {
    su = ((gw - 3) << 16) / W, sv = ((gh - 3) << 16) / H;
    elastic_weights(L);   // read behind the barriers of elastic_tile_field
  }
  for (unsigned t = blockIdx.x; t < total; t += gridDim.x) {
    const int tx0 = (int)(t % tiles_x) * AFF_TX;
    const unsigned r = t / tiles_x;
    const int ty0 = (int)(r % tiles_y) * AFF_TY, b = (int)(r / tiles_y);
    const int x0 = tx0 + lx, y = ty0 + ly;
    long long dx[AFF_XV] = {0, 0, 0, 0}, dy[AFF_XV] = {0, 0, 0, 0};
    if (ctrl) elastic_tile_field(L, ctrl + (int64_t)b * 2 * gh * gw, gh, gw, su, sv, tx0, ty0, H, W, lx, ly, dx, dy);
    if (y >= H || x0 >= W) continue;   // behind the tile's barriers
    const int* p = params + 16 * b;
    const int64_t sx0 = (int64_t)p[2] + (int64_t)y * p[1] + (int64_t)x0 * p[0];
    const int64_t sy0 = (int64_t)p[5] + (int64_t)y * p[4] + (int64_t)x0 * p[3];
    const int a0 = p[0], a3 = p[3];
    int A[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = p[6 + i];
    const int kq = p[15];
    int tt = 0;
    if (kq != 0 && sums) tt = (int)(((int64_t)kq * aff_mean_q8(sums[b], Hs * Ws) + 128) >> 8);   // |k m| < 2^31
    const uint8_t* ib = img + (int64_t)b * Hs * row;
    const uint8_t* mb = mask + (int64_t)b * Hs * Ws;
    const int* lb = labels + (int64_t)b * Hs * Ws;
    float val[3][AFF_XV];
    int64_t lab[AFF_XV];
    int ins[AFF_XV];
#pragma unroll
    for (int k = 0; k < AFF_XV; ++k) {
      const int64_t sx = sx0 + (int64_t)k * a0 + dx[k], sy = sy0 + (int64_t)k * a3 + dy[k];
      // every index below -1 or above the side is as far outside as -2 / the side: no tap of it lies inside
      const int ix = (int)min(max(sx >> 16, (int64_t)-2), (int64_t)Ws), iy = (int)min(max(sy >> 16, (int64_t)-2), (int64_t)Hs);
      const unsigned fx = (unsigned)(sx >> 8) & 255u, fy = (unsigned)(sy >> 8) & 255u;
      const bool x0in = (unsigned)ix < (unsigned)Ws, x1in = (unsigned)(ix + 1) < (unsigned)Ws;
      const bool y0in = (unsigned)iy < (unsigned)Hs, y1in = (unsigned)(iy + 1) < (unsigned)Hs;
      const unsigned w00 = (256u - fx) * (256u - fy), w10 = fx * (256u - fy), w01 = (256u - fx) * fy, w11 = fx * fy;
      const int o = iy * row + ix * 3;   // dereferenced only where a tap of that row lies inside
      unsigned ta0, ta1, tb0, tb1;       // the two rows' six bytes
      aff_load_run(ib + o, img, img_end, (const uint8_t*)p, x0in && y0in, x1in && y0in, ta0, ta1);
      aff_load_run(ib + o + row, img, img_end, (const uint8_t*)p, x0in && y1in, x1in && y1in, tb0, tb1);
      int v[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int sc = bgr ? 2 - c : c;   // byte sc of the first tap, byte 3 + sc of the second
        const unsigned sh0 = 8u * (unsigned)sc, sh1 = 8u * (unsigned)((3 + sc) & 3);
        const unsigned p00 = (x0in && y0in) ? (ta0 >> sh0) & 255u : (unsigned)fill[c];
        const unsigned p10 = (x1in && y0in) ? ((sc == 0 ? ta0 : ta1) >> sh1) & 255u : (unsigned)fill[c];
        const unsigned p01 = (x0in && y1in) ? (tb0 >> sh0) & 255u : (unsigned)fill[c];
        const unsigned p11 = (x1in && y1in) ? ((sc == 0 ? tb0 : tb1) >> sh1) & 255u : (unsigned)fill[c];
        v[c] = (int)((w00 * p00 + w10 * p10 + w01 * p01 + w11 * p11 + 32768u) >> 16);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int q = (A[3 * c] * v[0] + A[3 * c + 1] * v[1] + A[3 * c + 2] * v[2] + tt + 2048) >> 12;   // below 2^25 + 2^23: int
        val[c][k] = u8_normalize((uint8_t)min(max(q, 0), 255), c, nm.m0, nm.m1, nm.m2, nm.s0, nm.s1, nm.s2);
      }
      if (mask_out || labels_out) {
        const int mx = (int)min(max((sx + 32768) >> 16, (int64_t)-1), (int64_t)Ws), my = (int)min(max((sy + 32768) >> 16, (int64_t)-1), (int64_t)Hs);
        const bool in = (unsigned)mx < (unsigned)Ws && (unsigned)my < (unsigned)Hs;
        int64_t m = mask_fill;
        int id = label_fill;
        if (in && mask_out) {
          const int u = mb[my * Ws + mx];
          m = num_classes > 0 ? min(u, num_classes - 1) : u;
        }
        if (in && labels_out) id = lb[my * Ws + mx];
        lab[k] = m, ins[k] = id;
      }
    }
    const int64_t obase = b * so.b + y * so.h;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* o = out + obase + c * so.c;
      if (VEC) {
        *(float4*)(o + x0) = make_float4(val[c][0], val[c][1], val[c][2], val[c][3]);
      } else {
#pragma unroll
        for (int k = 0; k < AFF_XV; ++k)
          if (x0 + k < W) o[(x0 + k) * so.w] = val[c][k];
      }
    }
    if (mask_out) {
      int64_t* mo = mask_out + (int64_t)b * H * W + (int64_t)y * W + x0;
      if (VEC) {
        ((longlong2*)mo)[0] = make_longlong2(lab[0], lab[1]);
        ((longlong2*)mo)[1] = make_longlong2(lab[2], lab[3]);
      } else {
#pragma unroll
        for (int k = 0; k < AFF_XV; ++k)
          if (x0 + k < W) mo[k] = lab[k];
      }
    }
    if (labels_out) {
      int* lo = labels_out + (int64_t)b * H * W + (int64_t)y * W + x0;
      if (VEC) {
        *(int4*)lo = make_int4(ins[0], ins[1], ins[2], ins[3]);
      } else {
#pragma unroll
        for (int k = 0; k < AFF_XV; ++k)
          if (x0 + k < W) lo[k] = ins[k];
      }
    }
  }
}

// field (B, 2, H, W): plane 0 Dx, plane 1 Dy of every result pixel.  vec: W % 4 == 0 and field 16-byte aligned.
__global__ __launch_bounds__(256) void elastic_field_kernel(const int* __restrict__ ctrl, int B, int gh, int gw, int H, int W,
                                                            int* __restrict__ field, int vec) {
  __shared__ ElasticLds L;
  const unsigned tiles_x = (unsigned)((W + AFF_TX - 1) / AFF_TX), tiles_y = (unsigned)((H + AFF_TY - 1) / AFF_TY);
  const unsigned total = (unsigned)B * tiles_y * tiles_x;   // < 2^31 (checked on the host)
  const int lx = (int)(threadIdx.x % (AFF_TX / AFF_XV)) * AFF_XV, ly = (int)(threadIdx.x / (AFF_TX / AFF_XV));
  const int su = ((gw - 3) << 16) / W, sv = ((gh - 3) << 16) / H;
  elastic_weights(L);
  for (unsigned t = blockIdx.x; t < total; t += gridDim.x) {
    const int tx0 = (int)(t % tiles_x) * AFF_TX;
    const unsigned r = t / tiles_x;
    const int ty0 = (int)(r % tiles_y) * AFF_TY, b = (int)(r / tiles_y);
    const int x0 = tx0 + lx, y = ty0 + ly;
    long long dx[AFF_XV], dy[AFF_XV];
    elastic_tile_field(L, ctrl + (int64_t)b * 2 * gh * gw, gh, gw, su, sv, tx0, ty0, H, W, lx, ly, dx, dy);
    if (y >= H || x0 >= W) continue;
    int* fx = field + ((int64_t)b * 2 * H + y) * W + x0;
    int* fy = fx + (int64_t)H * W;
    if (vec) {
      *(int4*)fx = make_int4((int)dx[0], (int)dx[1], (int)dx[2], (int)dx[3]);
      *(int4*)fy = make_int4((int)dy[0], (int)dy[1], (int)dy[2], (int)dy[3]);
    } else {
#pragma unroll
      for (int k = 0; k < AFF_XV; ++k)
        if (x0 + k < W) fx[k] = (int)dx[k], fy[k] = (int)dy[k];
    }
  }
}

}  // namespace mgu

using namespace mgu;
using namespace mgud;

namespace {

int64_t result_tiles(int B, int H, int W) { return (int64_t)B * ((H + AFF_TY - 1) / AFF_TY) * ((W + AFF_TX - 1) / AFF_TX); }

}  // namespace

extern "C" {

// The argument checks come before the context check, so each refusal has its message (mgu_last_error(NULL) without a context).
int mgu_augment_elastic_color(mgu_ctx* c, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, const uint8_t* mask_u8, int num_classes,
                              float* out, int H, int W, const int64_t* out_strides, const float* mean3, const float* std3,
                              const uint8_t* fill_rgb, int64_t* mask_out, int64_t mask_fill, const int32_t* params_dev, int need_mean,
                              const int32_t* labels_i32, int32_t* labels_out, int32_t label_fill, const int32_t* ctrl_dev, int gh, int gw,
                              void* hip_stream) {
  if (!img_u8 || !out || !out_strides || !mean3 || !std3 || !fill_rgb || !params_dev)
    return fail(c, MGU_ERR_INVALID, "augment_elastic_color: null pointer (images, out, out_strides, mean3, std3, fill_rgb or params_dev)");
  if (B < 1 || Hs < 1 || Ws < 1 || H < 1 || W < 1 || num_classes < 0)
    return fail(c, MGU_ERR_INVALID, "augment_elastic_color: B, Hs, Ws, H, W must be >= 1 and num_classes >= 0");
  if (Hs > AFF_MAX_SIDE || Ws > AFF_MAX_SIDE || H > AFF_MAX_SIDE || W > AFF_MAX_SIDE)
    return fail(c, MGU_ERR_INVALID, "augment_elastic_color: %d x %d -> %d x %d is above %d pixels a side", Hs, Ws, H, W, AFF_MAX_SIDE);
  if (!mask_u8 != !mask_out) return fail(c, MGU_ERR_INVALID, "augment_elastic_color: mask_u8 and mask_out go together");
  if (!labels_i32 != !labels_out) return fail(c, MGU_ERR_INVALID, "augment_elastic_color: labels_i32 and labels_out go together");
  if (ctrl_dev ? (gh < EL_MIN_NODES || gh > EL_MAX_NODES || gw < EL_MIN_NODES || gw > EL_MAX_NODES) : (gh != 0 || gw != 0))
    return fail(c, MGU_ERR_INVALID, "augment_elastic_color: %d x %d control nodes: both in [%d, %d] with ctrl_dev, both 0 without", gh, gw,
                EL_MIN_NODES, EL_MAX_NODES);
  const int64_t tiles = result_tiles(B, H, W), luma_tile = mgu_augment_luma_tile();
  if (tiles >= ((int64_t)1 << 31) || (int64_t)B * (((int64_t)Hs * Ws + luma_tile - 1) / luma_tile) >= ((int64_t)1 << 31))
    return fail(c, MGU_ERR_INVALID, "augment_elastic_color: batch too large for one launch (B * tiles >= 2^31)");
  if (!c) return fail(c, MGU_ERR_INVALID, "augment_elastic_color: null context");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  unsigned long long* sums = nullptr;
  if (need_mean) {   // the affine entry's luma pass: one fill and the luma kernel
    int rc = ensure(c, &c->imgws, &c->imgws_bytes, (size_t)B * sizeof(unsigned long long));
    if (rc) return rc;
    sums = (unsigned long long*)c->imgws;
    if ((rc = mgu_augment_luma_sums(c, img_u8, B, Hs, Ws, bgr, (int64_t*)sums, hip_stream))) return rc;
  }
  const AffStrides so{out_strides[0], out_strides[1], out_strides[2], out_strides[3]};
  const AffNorm nm{mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2]};
  const bool vec = so.w == 1 && W % 4 == 0 && so.h % 4 == 0 && so.c % 4 == 0 && so.b % 4 == 0 && aligned16(out) && (!mask_out || aligned16(mask_out)) &&
                   (!labels_out || aligned16(labels_out));
  const dim3 grid((unsigned)std::min<int64_t>(tiles, 256 * 16));
  {
    ProfScope ps(c, s, "augment elastic");
    if (vec)
      hipLaunchKernelGGL(elastic_color_kernel<true>, grid, dim3(256), 0, s, img_u8, mask_u8, (const int*)labels_i32, B, Hs, Ws, bgr ? 1 : 0,
                         num_classes, out, H, W, so, nm, (int)fill_rgb[0], (int)fill_rgb[1], (int)fill_rgb[2], mask_out, mask_fill,
                         (int*)labels_out, (int)label_fill, (const int*)params_dev, sums, (const int*)ctrl_dev, gh, gw);
    else
      hipLaunchKernelGGL(elastic_color_kernel<false>, grid, dim3(256), 0, s, img_u8, mask_u8, (const int*)labels_i32, B, Hs, Ws, bgr ? 1 : 0,
                         num_classes, out, H, W, so, nm, (int)fill_rgb[0], (int)fill_rgb[1], (int)fill_rgb[2], mask_out, mask_fill,
                         (int*)labels_out, (int)label_fill, (const int*)params_dev, sums, (const int*)ctrl_dev, gh, gw);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

int mgu_elastic_field(mgu_ctx* c, const int32_t* ctrl_dev, int B, int gh, int gw, int H, int W, int32_t* field_out, void* hip_stream) {
  if (!ctrl_dev || !field_out) return fail(c, MGU_ERR_INVALID, "elastic_field: null pointer (ctrl_dev or field_out)");
  if (B < 1 || H < 1 || W < 1) return fail(c, MGU_ERR_INVALID, "elastic_field: B, H, W must be >= 1");
  if (H > AFF_MAX_SIDE || W > AFF_MAX_SIDE) return fail(c, MGU_ERR_INVALID, "elastic_field: %d x %d is above %d pixels a side", H, W, AFF_MAX_SIDE);
  if (gh < EL_MIN_NODES || gh > EL_MAX_NODES || gw < EL_MIN_NODES || gw > EL_MAX_NODES)
    return fail(c, MGU_ERR_INVALID, "elastic_field: %d x %d control nodes: both must be in [%d, %d]", gh, gw, EL_MIN_NODES, EL_MAX_NODES);
  const int64_t tiles = result_tiles(B, H, W);
  if (tiles >= ((int64_t)1 << 31)) return fail(c, MGU_ERR_INVALID, "elastic_field: batch too large for one launch (B * tiles >= 2^31)");
  if (!c) return fail(c, MGU_ERR_INVALID, "elastic_field: null context");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  {
    ProfScope ps(c, s, "elastic field");
    hipLaunchKernelGGL(elastic_field_kernel, dim3((unsigned)std::min<int64_t>(tiles, 256 * 16)), dim3(256), 0, s, (const int*)ctrl_dev, B, gh, gw, H, W,
                       (int*)field_out, (W % 4 == 0 && aligned16(field_out)) ? 1 : 0);
  }
  HIPCHK(c, hipGetLastError());
  return MGU_OK;
}

}  // extern "C"
