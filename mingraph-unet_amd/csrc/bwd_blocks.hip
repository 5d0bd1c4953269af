// Backward building blocks behind the C-ABI: each entry point runs ONE stage of loss.backward() (scripts/train_segmentation.py:133)
// on caller-provided tensors.  The convolution stages call the very functions mgu_unet_backward runs (conv_wgrad, conv_dgrad,
// convt_wgrad, convt_dgrad in mgunet_train.hip) on a Layer of the caller's shape (fp32, input channels stored padded to 4) and a
// FwdRecord of the caller's tensors.  They exist so that every backward kernel can be checked in isolation against a float64 reference
// on fixed (x, dz) -- where nothing is ill-conditioned -- instead of only through a whole train step whose BatchNorm + ReLU + MaxPool
// chain amplifies rounding (tests/test_gpu_backward_kernels.py).
// Kernel selection is the launchers' own (pick_conv, pick_wgrad), on the context's switches (MGU_NO_WINO_WGRAD, MGU_NO_WGRAD_HALO,
// MGU_NO_THIN_WGRAD, MGU_NO_WINO_DGRAD, MGU_NO_WINOGRAD, ... read at mgu_create), so a test reaches every variant.
#include <algorithm>
#include <cmath>

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
  if ((rc = ensure_red(c, Cmax))) return rc;
  char* g = (char*)c->gws;
  out->dwp = (float*)(g + o_dwp), out->dgp = (float*)(g + o_dgp), out->wug = (float*)(g + o_wug);
  out->dwp_floats = dwp_floats, out->dgp_floats = std::max<size_t>(dgp_floats, 64);
  out->sums = (double*)(g + o_sums);
  out->red = (double*)c->redws;
  out->clear = true;   // the scratch is shared with every other building block: no panel row is known to be zero
  return MGU_OK;
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
  const Layer L = make_layer(MGU_DTYPE_F32, Cin, rup(Cin, 4), Cout, ksize, false);
  const FwdRecord r{.in = (const float*)in_dev, .ldin = ld_in, .B = B, .H = H, .W = W};   // dz rows are padded to a multiple of 4 channels (zeros)
  Scratch sc;
  int rc = get_scratch(c, (size_t)rup(rup(Cout, 4), 128) * L.Kp, 0, 0, 64, &sc);
  if (rc) return rc;
  return conv_wgrad(c, L, r, (const float*)dz_dev, (float*)dw_oihw_dev, sc, false, (hipStream_t)hip_stream);
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
  Layer L = make_layer(MGU_DTYPE_F32, Cin, rup(Cin, 4), Cout, ksize, false);
  L.w_src = (const float*)w_oihw_dev;
  Scratch sc;
  const bool wino = wino_dgrad_layer(c->tn, ksize, Cop);
  int rc = get_scratch(c, 0, (size_t)rup(Cin, 128) * rup(ksize * ksize * Cop, 32), wino ? wino_u_floats(Cin, Cop) : 0, 64, &sc);
  if (rc) return rc;
  L.wug = sc.wug;   // the Winograd set, when the pick takes that kernel, is packed into the scratch
  return conv_dgrad(c, L, {.B = B, .H = H, .W = W}, (const float*)dz_dev, (float*)din_dev, ld_out, sc, false, (hipStream_t)hip_stream);
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
  const Layer U = make_layer(MGU_DTYPE_F32, Cin, Cin, Cout, 1, true);
  const FwdRecord r{.in = (const float*)in_dev, .ldin = Cin, .B = B, .H = H, .W = W};
  Scratch sc;
  int rc = get_scratch(c, (size_t)rup(Cin, 128) * rup(4 * Cout, 32), 0, 0, Cout, &sc);
  if (rc) return rc;
  if ((rc = convt_wgrad(c, U, r, (const float*)dout_dev, ld_d, c_off, 2 * H, 2 * W, (float*)dw_iohw_dev, sc, s))) return rc;
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
  Layer U = make_layer(MGU_DTYPE_F32, Cin, rup(Cin, 4), Cout, 1, true);
  U.w_src = (const float*)w_iohw_dev;
  Scratch sc;
  int rc = get_scratch(c, 0, std::max((size_t)rup(Cin, 128) * rup(4 * Cout, 32), convt_x3_dgrad_floats(Cin, Cout)), 0, 64, &sc);
  if (rc) return rc;
  return convt_dgrad(c, U, {.B = B, .H = H, .W = W}, (const float*)dout_dev + c_off, ld_d, 2 * H, 2 * W, (float*)din_dev, sc, false,
                     (hipStream_t)hip_stream);
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

int mgu_conv_bn_relu_train_nhwc(mgu_ctx* c, const void* in_dev, int ld_in, int B, int H, int W, int Cin, const void* w_oihw_dev,
                                const void* bias_dev, const void* gamma_dev, const void* beta_dev, int Cout, void* z_dev, void* y_dev,
                                int ld_y, void* pooled_dev, void* mean_dev, void* invstd_dev, void* run_mean_dev, void* run_var_dev,
                                int* stats_fused_out, int* pool_fused_out, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !w_oihw_dev || !bias_dev || !gamma_dev || !beta_dev || !z_dev || !y_dev || !mean_dev || !invstd_dev || !run_mean_dev ||
      !run_var_dev || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 4 || (Cout & 3) || Cout > 1024 || ld_y < Cout || (ld_y & 3))
    return fail(c, MGU_ERR_INVALID, "bad conv_bn_relu_train args (4 <= Cout <= 1024, Cout and ld_y multiples of 4)");
  if (ld_in < rup(Cin, 4) || (ld_in & 3)) return fail(c, MGU_ERR_INVALID, "ld_in must be a multiple of 4 and >= Cin rounded up to 4");
  if ((int64_t)B * H * W >= (1ll << 31) || (int64_t)B * H * W < 2) return fail(c, MGU_ERR_INVALID, "B*H*W must be in [2, 2^31)");
  if (pooled_dev && (H < 2 || W < 2)) return fail(c, MGU_ERR_INVALID, "the pooled output needs H, W >= 2");
  if (c->dtype != MGU_DTYPE_F32) return fail(c, MGU_ERR_STATE, "training runs in fp32 only (bf16 storage is an inference mode)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  // the caller's tensors as a model layer (mgu_unet_configure / repack_weights): the direct panel is packed by run_layer if its
  // pick reads it, the Winograd set and the first convolution's forms here
  Layer L = make_layer(MGU_DTYPE_F32, Cin, rup(Cin, 4), Cout, 3, false);
  L.w_src = (const float*)w_oihw_dev, L.b_src = (const float*)bias_dev, L.gamma = (const float*)gamma_dev, L.beta = (const float*)beta_dev;
  L.run_mean = (float*)run_mean_dev, L.run_var = (float*)run_var_dev, L.mean = (float*)mean_dev, L.invstd = (float*)invstd_dev;
  L.wino = wino_layer(c->tn, 3, L.Cp);
  L.first = first_conv_applicable(MGU_DTYPE_F32, Cin, L.Cp, Cout, 8, 0);
  Carve k;
  const size_t panel = (size_t)L.Np * L.Kp;
  const size_t o_wp = k.take(panel * 4), o_ts = k.take(2 * (size_t)Cout * 4), o_sums = k.take(sizeof(double) * 2 * (size_t)Cout);
  const size_t o_wf = k.take(L.first ? 9 * 4 * (size_t)Cout * 4 : 0), o_wfm = k.take(L.first ? first_mfma_floats() * 4 : 0);
  int rc = ensure(c, &c->gws, &c->gws_bytes, k.off);
  if (rc) return rc;
  if ((rc = ensure_red(c, Cout))) return rc;
  char* g = (char*)c->gws;
  L.wp = (float*)(g + o_wp), L.wp_dirty = true;
  L.tscale = (float*)(g + o_ts), L.tshift = L.tscale + Cout;
  HIPCHK(c, hipMemsetAsync(L.wp, 0, panel * 4, s));   // the panel's padding is read as zeros
  if (L.wino) {
    if ((rc = ensure(c, &c->wuws, &c->wuws_bytes, wino_u_floats(Cout, L.Cp) * sizeof(float)))) return rc;
    L.wu = (float*)c->wuws;
    HIPCHK(c, launch_pack_one(pack_wino(L.w_src, L.wu, Cout, Cin, L.Cp, 0, c->tn.wino_prec), s));
  }
  if (L.first) {
    L.wf = (float*)(g + o_wf);
    HIPCHK(c, launch_pack_one(pack_first_w(L.w_src, L.wf, Cout, Cin), s));
    if (Cout == 32 && Cin <= 3) {
      L.wfm = (float*)(g + o_wfm);
      HIPCHK(c, launch_pack_one(pack_first_mfma(L.w_src, L.wfm, Cout, Cin), s));
    }
  }
  const FwdRecord r{(const float*)in_dev, ld_in, (float*)z_dev, (float*)y_dev, ld_y, B, H, W};
  ConvTaken took;
  rc = conv_bn_relu_train(c, L, r, (double*)(g + o_sums), (double*)c->redws, s, (float*)pooled_dev, &took);
  if (stats_fused_out) *stats_fused_out = took.stats;
  if (pool_fused_out) *pool_fused_out = took.pool;
  return red_cleared_on_error(c, rc, s);   // the epilogue's sums may be waiting for their fold
}

int mgu_bn_relu_conv_backward_nhwc(mgu_ctx* c, const void* in_dev, int ld_in, const void* z_dev, const void* dy_dev, int ld_dy,
                                   const void* gamma_dev, const void* beta_dev, const void* mean_dev, const void* invstd_dev,
                                   const void* w_oihw_dev, int B, int H, int W, int Cin, int Cout, void* dz_dev, void* dgamma_dev,
                                   void* dbeta_dev, void* dbias_dev, void* dw_oihw_dev, void* din_dev, int ld_din, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !z_dev || !dy_dev || !gamma_dev || !beta_dev || !mean_dev || !invstd_dev || !w_oihw_dev || !dz_dev || !dgamma_dev ||
      !dbeta_dev || !dbias_dev || !dw_oihw_dev || B < 1 || H < 1 || W < 1 || Cin < 1 || Cout < 4 || (Cout & 3) || Cout > 1024 ||
      ld_dy < Cout || (ld_dy & 3))
    return fail(c, MGU_ERR_INVALID, "bad bn_relu_conv_backward args (4 <= Cout <= 1024, Cout and ld_dy multiples of 4)");
  if (ld_in < rup(Cin, 4) || (ld_in & 3)) return fail(c, MGU_ERR_INVALID, "ld_in must be a multiple of 4 and >= Cin rounded up to 4");
  if (din_dev && ld_din < Cin) return fail(c, MGU_ERR_INVALID, "ld_din %d < Cin %d", ld_din, Cin);
  if ((int64_t)B * H * W >= (1ll << 31) || (int64_t)B * H * W < 2) return fail(c, MGU_ERR_INVALID, "B*H*W must be in [2, 2^31)");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Layer L = make_layer(MGU_DTYPE_F32, Cin, rup(Cin, 4), Cout, 3, false);
  const FwdRecord r{.in = (const float*)in_dev, .ldin = ld_in, .z = (float*)const_cast<void*>(z_dev), .B = B, .H = H, .W = W};
  L.w_src = (const float*)w_oihw_dev, L.gamma = (const float*)gamma_dev, L.beta = (const float*)beta_dev;
  L.mean = (float*)const_cast<void*>(mean_dev), L.invstd = (float*)const_cast<void*>(invstd_dev);
  const bool wino = din_dev && wino_dgrad_layer(c->tn, 3, Cout);
  const size_t dpanel = din_dev ? (size_t)rup(Cin, 128) * rup(9 * Cout, 32) : 0;
  Scratch sc;
  int rc = get_scratch(c, (size_t)rup(Cout, 128) * L.Kp, dpanel + 2 * (size_t)Cout, wino ? wino_u_floats(Cin, Cout) : 0, Cout, &sc);
  if (rc) return rc;
  L.wug = wino ? sc.wug : nullptr;   // the Winograd set, when the pick takes that kernel, is packed into the scratch
  // forward scale / shift behind the data-gradient panel (the ReLU mask is recomputed from z): scale = gamma*invstd, shift = beta - mean*scale
  L.tscale = sc.dgp + dpanel, L.tshift = L.tscale + Cout;
  hipLaunchKernelGGL(fold_batch_stats_kernel, dim3((Cout + 255) / 256), dim3(256), 0, s, L.gamma, L.beta, L.mean, L.invstd, L.tscale, L.tshift,
                     Cout);
  HIPCHK(c, hipGetLastError());
  LayerGrads g;
  g.dw = (float*)dw_oihw_dev, g.dbias = (float*)dbias_dev, g.dgamma = (float*)dgamma_dev, g.dbeta = (float*)dbeta_dev;
  rc = conv_bn_relu_backward(c, L, r, (const float*)dy_dev, ld_dy, (float*)dz_dev, g, (float*)din_dev, ld_din, sc, s);
  return red_cleared_on_error(c, rc, s);   // the deferred column sums may be waiting for their fold
}

int mgu_reduction_slots_absmax(mgu_ctx* c, double* absmax_out, void* hip_stream) {
  if (!c || !absmax_out) return MGU_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize((hipStream_t)hip_stream));
  std::vector<double> host(c->redws_bytes / sizeof(double));
  if (!host.empty()) HIPCHK(c, hipMemcpy(host.data(), c->redws, host.size() * sizeof(double), hipMemcpyDeviceToHost));
  double m = 0.0;
  for (double v : host) {
    if (std::fabs(v) <= m) continue;
    m = std::fabs(v);
    if (m != m) break;   // a NaN is the answer
  }
  *absmax_out = m;
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
