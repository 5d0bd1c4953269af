// Backward building blocks behind the C-ABI: each entry point runs ONE stage of loss.backward()
// (scripts/train_segmentation.py:133) on caller-provided tensors.  The convolution stages call the very functions mgu_unet_backward
// runs (conv_wgrad, conv_dgrad, convt_wgrad, convt_dgrad in mgunet_train.hip) on a Layer that describes the caller's tensors.  They exist so that every backward kernel can be checked in isolation against a float64
// reference on fixed (x, dz) -- where nothing is ill-conditioned -- instead of only through a whole train step whose
// BatchNorm + ReLU + MaxPool chain amplifies rounding (tests/test_gpu_backward_kernels.py).
// Kernel selection is the launchers' own (pick_conv, pick_wgrad), on the context's switches (MGU_NO_WINO_WGRAD, MGU_NO_WGRAD_HALO,
// MGU_NO_THIN_WGRAD, MGU_NO_WINO_DGRAD, MGU_NO_WINOGRAD, ... read at mgu_create), so a test reaches every variant.
#include <algorithm>

#include "ctx.h"

using namespace mgu;
using namespace mgud;

namespace {

// scale / shift of the train-mode forward from the batch statistics: y = relu(scale * z + shift)
__global__ void fold_batch_stats_kernel(const float* gamma, const float* beta, const float* mean, const float* invstd, float* scale,
                                        float* shift, int C) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < C) {
    const float sc = gamma[i] * invstd[i];
    scale[i] = sc;
    shift[i] = beta[i] - mean[i] * sc;
  }
}

struct Scratch : BwdScratch {
  float* wug;   // a Winograd data-gradient set
};

int get_scratch(mgu_ctx* c, size_t panel_floats, size_t dgp_floats, size_t wug_floats, int Cmax, Scratch* out) {
  Carve k;
  const size_t dwp_floats = std::max(panel_floats, (size_t)12 << 20);   // room for the atomics-free kernels' partial panels
  const size_t o_dwp = k.take(dwp_floats * 4), o_dgp = k.take(std::max<size_t>(dgp_floats, 64) * 4), o_wug = k.take((wug_floats + 64) * 4);
  const size_t o_sums = k.take(sizeof(double) * 2 * (size_t)std::max(Cmax, 64) + 64);
  int rc = ensure(c, &c->gws, &c->gws_bytes, k.off);
  if (rc) return rc;
  const size_t need = chan_reduce_work_bytes(std::max(Cmax, 64));
  if (c->redws_bytes < need) {   // the slots must be zero between reductions: a fresh allocation is cleared once
    if ((rc = ensure(c, &c->redws, &c->redws_bytes, need))) return rc;
    HIPCHK(c, hipMemset(c->redws, 0, need));
  }
  char* g = (char*)c->gws;
  out->dwp = (float*)(g + o_dwp), out->dgp = (float*)(g + o_dgp), out->wug = (float*)(g + o_wug);
  out->dwp_floats = dwp_floats, out->dgp_floats = std::max<size_t>(dgp_floats, 64);
  out->sums = (double*)(g + o_sums);
  out->red = (double*)c->redws;
  out->clear = true;   // the scratch is shared with every other building block: no panel row is known to be zero
  return MGU_OK;
}

// the caller's tensors as the layer whose backward runs: its shape and the grid its forward ran on (input grid of a ConvTranspose)
Layer caller_layer(int Cin, int Cout, int KS, bool convt, int B, int H, int W) {
  Layer L;
  L.Cin = Cin, L.Cp = rup(Cin, 4), L.Cout = Cout, L.KS = KS, L.convt = convt;
  L.K = KS * KS * L.Cp, L.Kp = rup(L.K, 32);
  L.t_B = B, L.t_H = H, L.t_W = W;
  return L;
}

}  // namespace

extern "C" {

int mgu_conv2d_wgrad_nhwc(mgu_ctx* c, const void* in_dev, int ld_in, const void* dz_dev, int B, int H, int W, int Cin, int Cout,
                          int ksize, void* dw_oihw_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !dz_dev || !dw_oihw_dev || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ksize != 1 && ksize != 3))
    return fail(c, MGU_ERR_INVALID, "bad conv2d_wgrad args (ksize must be 1 or 3)");
  if (ld_in < rup(Cin, 4) || (ld_in & 3)) return fail(c, MGU_ERR_INVALID, "ld_in must be a multiple of 4 and >= Cin rounded up to 4");
  if ((int64_t)B * H * W >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  Layer L = caller_layer(Cin, Cout, ksize, false, B, H, W);
  L.t_in = (const float*)in_dev, L.t_ldin = ld_in;   // dz rows are padded to a multiple of 4 channels (zeros)
  Scratch sc;
  int rc = get_scratch(c, (size_t)rup(rup(Cout, 4), 128) * L.Kp, 0, 0, 64, &sc);
  if (rc) return rc;
  return conv_wgrad(c, L, (const float*)dz_dev, (float*)dw_oihw_dev, sc, false, (hipStream_t)hip_stream);
}

int mgu_conv2d_dgrad_nhwc(mgu_ctx* c, const void* dz_dev, const void* w_oihw_dev, int B, int H, int W, int Cin, int Cout, int ksize,
                          void* din_dev, int ld_out, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!dz_dev || !w_oihw_dev || !din_dev || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 1 || (ksize != 1 && ksize != 3))
    return fail(c, MGU_ERR_INVALID, "bad conv2d_dgrad args (ksize must be 1 or 3)");
  if (ld_out < Cin) return fail(c, MGU_ERR_INVALID, "ld_out %d < Cin %d", ld_out, Cin);
  if ((int64_t)B * H * W >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  const int Cop = rup(Cout, 4);
  Layer L = caller_layer(Cin, Cout, ksize, false, B, H, W);
  L.w_src = (const float*)w_oihw_dev;
  Scratch sc;
  const bool wino = wino_dgrad_layer(c->tn, ksize, Cop);
  int rc = get_scratch(c, 0, (size_t)rup(Cin, 128) * rup(ksize * ksize * Cop, 32), wino ? wino_u_floats(Cin, Cop) : 0, 64, &sc);
  if (rc) return rc;
  L.wug = sc.wug;   // the Winograd set, when the pick takes that kernel, is packed into the scratch
  return conv_dgrad(c, L, (const float*)dz_dev, (float*)din_dev, ld_out, sc, false, (hipStream_t)hip_stream);
}

int mgu_conv_transpose2x2_wgrad_nhwc(mgu_ctx* c, const void* in_dev, const void* dout_dev, int ld_d, int c_off, int B, int H, int W,
                                     int Cin, int Cout, void* dw_iohw_dev, void* dbias_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !dout_dev || !dw_iohw_dev || B < 1 || H < 1 || W < 1 || Cin < 4 || (Cin & 3) || Cout < 4 || (Cout & 3) || Cout > 1024)
    return fail(c, MGU_ERR_INVALID, "bad convT_wgrad args (Cin, Cout multiples of 4)");
  if (ld_d < c_off + Cout || (ld_d & 3) || (c_off & 3)) return fail(c, MGU_ERR_INVALID, "ld_d / c_off must be multiples of 4, ld_d >= c_off + Cout");
  if ((int64_t)B * H * W * 4 >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "4*B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Layer U = caller_layer(Cin, Cout, 1, true, B, H, W);
  U.t_in = (const float*)in_dev, U.t_ldin = Cin;
  Scratch sc;
  int rc = get_scratch(c, (size_t)rup(Cin, 128) * rup(4 * Cout, 32), 0, 0, Cout, &sc);
  if (rc) return rc;
  if ((rc = convt_wgrad(c, U, (const float*)dout_dev, ld_d, c_off, 2 * H, 2 * W, (float*)dw_iohw_dev, sc, s))) return rc;
  if (dbias_dev)
    HIPCHK(c, launch_colsum((const float*)dout_dev + c_off, ld_d, (int64_t)B * H * W * 4, Cout, sc.red, (float*)dbias_dev, s));
  return MGU_OK;
}

int mgu_conv_transpose2x2_dgrad_nhwc(mgu_ctx* c, const void* dout_dev, int ld_d, int c_off, const void* w_iohw_dev, int B, int H,
                                     int W, int Cin, int Cout, void* din_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!dout_dev || !w_iohw_dev || !din_dev || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 4 || (Cout & 3))
    return fail(c, MGU_ERR_INVALID, "bad convT_dgrad args (Cout a multiple of 4)");
  if (ld_d < c_off + Cout || (ld_d & 3) || (c_off & 3)) return fail(c, MGU_ERR_INVALID, "ld_d / c_off must be multiples of 4, ld_d >= c_off + Cout");
  if ((int64_t)B * H * W * 4 >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "4*B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  Layer U = caller_layer(Cin, Cout, 1, true, B, H, W);
  U.w_src = (const float*)w_iohw_dev;
  Scratch sc;
  int rc = get_scratch(c, 0, std::max((size_t)rup(Cin, 128) * rup(4 * Cout, 32), convt_x3_dgrad_floats(Cin, Cout)), 0, 64, &sc);
  if (rc) return rc;
  return convt_dgrad(c, U, (const float*)dout_dev + c_off, ld_d, 2 * H, 2 * W, (float*)din_dev, sc, false, (hipStream_t)hip_stream);
}

int mgu_bn_relu_train_nhwc(mgu_ctx* c, const void* z_dev, const void* gamma_dev, const void* beta_dev, int64_t M, int C, void* y_dev,
                           int ld_y, void* mean_dev, void* invstd_dev, void* run_mean_dev, void* run_var_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!z_dev || !gamma_dev || !beta_dev || !y_dev || !mean_dev || !invstd_dev || !run_mean_dev || !run_var_dev || M < 2 || C < 4 ||
      (C & 3) || C > 1024 || ld_y < C || (ld_y & 3))
    return fail(c, MGU_ERR_INVALID, "bad bn_relu_train args (4 <= C <= 1024, C and ld_y multiples of 4, M >= 2)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Scratch sc;
  int rc = get_scratch(c, 0, 2 * (size_t)C, 0, C, &sc);   // dgp holds the folded scale / shift
  if (rc) return rc;
  float *tscale = sc.dgp, *tshift = sc.dgp + C;
  HIPCHK(c, launch_bn_stats((const float*)z_dev, C, M, C, sc.red, sc.sums, s));
  HIPCHK(c, launch_bn_finalize(sc.sums, sc.sums + C, M, 1e-5f, 0.1f, (const float*)gamma_dev, (const float*)beta_dev, (float*)mean_dev,
                               (float*)invstd_dev, tscale, tshift, (float*)run_mean_dev, (float*)run_var_dev, C, s));
  HIPCHK(c, launch_bn_apply_relu((const float*)z_dev, tscale, tshift, (float*)y_dev, ld_y, M, C, s));
  return MGU_OK;
}

int mgu_bn_relu_backward_nhwc(mgu_ctx* c, const void* dy_dev, int ld_dy, const void* z_dev, const void* gamma_dev, const void* beta_dev,
                              const void* mean_dev, const void* invstd_dev, int64_t M, int C, void* dz_dev, void* dgamma_dev,
                              void* dbeta_dev, void* dbias_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!dy_dev || !z_dev || !gamma_dev || !beta_dev || !mean_dev || !invstd_dev || !dz_dev || !dgamma_dev || !dbeta_dev || !dbias_dev ||
      M < 2 || C < 4 || (C & 3) || C > 1024 || ld_dy < C || (ld_dy & 3))
    return fail(c, MGU_ERR_INVALID, "bad bn_relu_backward args (4 <= C <= 1024, C and ld_dy multiples of 4, M >= 2)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Scratch sc;
  int rc = get_scratch(c, 0, 2 * (size_t)C, 0, C, &sc);
  if (rc) return rc;
  // forward scale/shift (the ReLU mask is recomputed from z): scale = gamma*invstd, shift = beta - mean*scale
  float *tscale = sc.dgp, *tshift = sc.dgp + C;
  hipLaunchKernelGGL(fold_batch_stats_kernel, dim3((C + 255) / 256), dim3(256), 0, s, (const float*)gamma_dev, (const float*)beta_dev,
                     (const float*)mean_dev, (const float*)invstd_dev, tscale, tshift, C);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, launch_bn_bwd_reduce((const float*)dy_dev, ld_dy, tscale, tshift, (const float*)z_dev, C, (const float*)mean_dev,
                                 (const float*)invstd_dev, M, C, sc.red, sc.sums, (float*)dbeta_dev, (float*)dgamma_dev, s));
  HIPCHK(c, launch_bn_bwd_apply((const float*)dy_dev, ld_dy, tscale, tshift, (const float*)z_dev, (const float*)mean_dev,
                                (const float*)invstd_dev, (const float*)gamma_dev, sc.sums, M, C, (float*)dz_dev, sc.red,
                                (float*)dbias_dev, s));
  return MGU_OK;
}

int mgu_maxpool2x2_backward_nhwc(mgu_ctx* c, const void* y_dev, int ld_y, const void* dpool_dev, void* dskip_dev, int ld_d, int B, int H,
                                 int W, int Cc, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!y_dev || !dpool_dev || !dskip_dev || B < 1 || H < 2 || W < 2 || Cc < 4 || (Cc & 3) || ld_y < Cc || (ld_y & 3) || ld_d < Cc || (ld_d & 3))
    return fail(c, MGU_ERR_INVALID, "bad maxpool_backward args (C, ld_y, ld_d multiples of 4, H,W >= 2)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_maxpool2_bwd_add((const float*)y_dev, ld_y, (const float*)dpool_dev, (float*)dskip_dev, ld_d, B, H, W, Cc,
                                    (hipStream_t)hip_stream));
  return MGU_OK;
}

}  // extern "C"
