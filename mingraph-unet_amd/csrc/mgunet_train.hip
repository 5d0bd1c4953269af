// Training step schedule behind the C-ABI: train-mode forward (batch-statistics BatchNorm), backward
// (dgrad / wgrad / BN / ReLU / MaxPool / ConvTranspose / 1x1), softmax cross-entropy, Adam.
// Replaces the autograd graph the reference builds at scripts/train_segmentation.py:121-134
// (optimizer.zero_grad -> model(images) -> CrossEntropyLoss -> loss.backward -> optimizer.step).
// Host orchestration only; kernels live in igemm.hip, wgrad_f32.hip, train_kernels.hip.
#include <algorithm>

#include <string>

#include "ctx.h"
#include <cstdlib>

using namespace mgu;
using namespace mgud;

namespace {

struct TPlan {
  size_t xin = 0, bott = 0, ta = 0, tb = 0, tc = 0, dwp = 0, dwp_floats = 0, dgp = 0, dgp_floats = 0, sums = 0, total = 0;
  std::vector<size_t> z, y1, pooled, dcat;
};

TPlan plan_train(const mgu_ctx* c, int B, int H, int W) {
  std::vector<int> hs, ws;
  level_dims(H, W, c->depth, hs, ws);
  // floats of a block's output (Cout channels) on level l
  auto out = [&](const Block& b, int l) { return (size_t)B * hs[l] * ws[l] * c->layers[b.conv2].Cout; };
  TPlan p;
  Carve k;
  auto fl = [&](size_t n) { return k.take(n * sizeof(float)); };
  p.xin = fl((size_t)B * H * W * c->Cp0);
  p.z.assign(c->layers.size(), 0);
  p.y1.assign(c->layers.size(), 0);
  auto blk = [&](const Block& b) {
    p.z[b.conv1] = fl(out(b, b.level));
    p.y1[b.conv1] = fl(out(b, b.level));
    p.z[b.conv2] = fl(out(b, b.level));
  };
  for (const Block& b : c->enc) blk(b);
  blk(c->bott);
  for (const Block& b : c->dec) blk(b);
  for (const Block& b : c->enc) p.pooled.push_back(fl(out(b, b.level + 1)));
  p.bott = fl(out(c->bott, c->bott.level));
  size_t tmax = out(c->bott, c->bott.level);
  for (const Block& b : c->enc) tmax = std::max(tmax, out(b, b.level));
  p.ta = fl(tmax);
  p.tb = fl(tmax);
  p.tc = fl(tmax);
  for (const Block& b : c->enc) p.dcat.push_back(fl(2 * out(b, b.level)));
  size_t pmax = (size_t)128 * 32;
  for (auto& L : c->layers) {
    pmax = std::max(pmax, (size_t)L.Np * L.Kp);                                              // wgrad panel (conv / convT)
    const size_t cop = rup(L.Cout, 4);
    pmax = std::max(pmax, (size_t)rup(L.Cp, 128) * rup(L.KS * L.KS * (int)cop * (L.convt ? 4 : 1), 32));  // dgrad panel
    if (L.convt) pmax = std::max(pmax, convt_x3_dgrad_floats(L.Cin, L.Cout));                          // its three-piece form
  }
  p.dwp_floats = std::max(pmax, (size_t)12 << 20);   // >= 48 MB: room for the atomics-free wgrad's partial panels
  p.dwp = fl(p.dwp_floats);
  p.dgp = fl(pmax);
  p.dgp_floats = pmax;
  // a Winograd data-gradient set the size of the largest L.wug: unused since every layer that takes that kernel keeps its own (the
  // region stays so that the published workspace size does not change)
  size_t umax = 0;
  for (const auto& L : c->layers)
    if (L.wug) umax = std::max(umax, wino_u_floats(L.Cin, rup(L.Cout, 4)));
  fl(umax + 64);
  p.sums = k.take(sizeof(double) * 2 * (size_t)c->layers[c->bott.conv2].Cout + 64);
  p.total = k.off;
  return p;
}

inline float* at(mgu_ctx* c, size_t off) { return (float*)((char*)c->tws + off); }

struct Bwd : BwdScratch {
  mgu_ctx* c;
  hipStream_t s;
  float *ta, *tb, *flat;
};

// where layer L's parameter gradients live in the flat gradient vector
LayerGrads flat_grads(const Bwd& w, const Layer& L) {
  LayerGrads g;
  g.dw = w.flat + L.off_w, g.dbias = w.flat + L.off_b, g.dgamma = w.flat + L.off_gamma, g.dbeta = w.flat + L.off_beta;
  return g;
}

// ConvBlock backward (unet_encoder.py:15-25 reversed).  dy has pitch lddy; dinput may be null.
int block_backward(Bwd& w, const Block& b, const float* dy, int lddy, float* dinput, int ld_dinput) {
  mgu_ctx* c = w.c;
  const Layer &L1 = c->layers[b.conv1], &L2 = c->layers[b.conv2];
  int rc;
  if ((rc = conv_bn_relu_backward(c, L2, c->fwd[b.conv2], dy, lddy, w.ta, flat_grads(w, L2), w.tb, L2.Cin, w, w.s))) return rc;   // d(y1), dense pitch C
  return conv_bn_relu_backward(c, L1, c->fwd[b.conv1], w.tb, L2.Cin, w.ta, flat_grads(w, L1), dinput, ld_dinput, w, w.s);
}

}  // namespace

// The reduction slots are zero between launches: slot_reduce_kernel clears what it read, so only a fresh allocation
// needs a memset (instead of one before each of the ~60 per-channel reductions of a step).
int mgud::ensure_red(mgu_ctx* c, int Cmax) {
  const size_t need = chan_reduce_work_bytes(std::max(Cmax, 64));
  if (c->redws_bytes >= need) return MGU_OK;
  int rc = ensure(c, &c->redws, &c->redws_bytes, need);
  if (rc) return rc;
  HIPCHK(c, hipMemset(c->redws, 0, need));
  return MGU_OK;
}

// conv (+bias) -> z ; batch statistics ; y = relu(bn(z)) written with pitch ldy
int mgud::conv_bn_relu_train(mgu_ctx* c, const Layer& L, const FwdRecord& r, double* sums, double* red, hipStream_t s, float* pooled,
                             ConvTaken* took) {
  const int64_t M = (int64_t)r.B * r.H * r.W;
  const int C = L.Cout;
  ConvTaken t;   // Winograd layers accumulate sum z / sum z^2 in the conv epilogue
  int rc = run_layer(c, L, {.in = r.in, .ldin = r.ldin, .B = r.B, .H = r.H, .W = r.W, .out = r.z, .ldout = C, .shift = L.b_src}, s,
                     {.stat_slots = red}, &t);  // unet_encoder.py:16 / :20
  if (rc) return rc;
  if (took) *took = t;
  if (t.stats) {
    HIPCHK(c, launch_bn_finalize_slots(red, t.stat_rows, sums, M, 1e-5f, 0.1f, L.gamma, L.beta, L.mean, L.invstd, L.tscale, L.tshift, L.run_mean,
                                       L.run_var, C, s));  // nn.BatchNorm2d defaults, unet_encoder.py:12-13
  } else {
    HIPCHK(c, launch_bn_stats(r.z, C, M, C, red, sums, s));
    HIPCHK(c, launch_bn_finalize(sums, sums + C, M, 1e-5f, 0.1f, L.gamma, L.beta, L.mean, L.invstd, L.tscale, L.tshift,
                                 L.run_mean, L.run_var, C, s));
  }
  if (pooled && !(r.H & 1) && !(r.W & 1)) {   // MaxPool2d(2) of y in the same pass (even sizes: windows tile the image)
    HIPCHK(c, launch_bn_apply_relu_pool(r.z, L.tscale, L.tshift, r.y, r.ldy, pooled, r.B, r.H, r.W, C, s));
    if (took) took->pool = true;
  } else {
    HIPCHK(c, launch_bn_apply_relu(r.z, L.tscale, L.tshift, r.y, r.ldy, M, C, s));
    if (pooled) HIPCHK(c, launch_maxpool2(r.y, r.ldy, pooled, 0, r.B, r.H, r.W, C, s));   // odd sizes: floor-mode windows leave a row / column out
  }
  return MGU_OK;
}

// BN(train) + ReLU backward, weight gradient (+ the bias gradient's fold), data gradient of one conv -> BN -> ReLU
int mgud::conv_bn_relu_backward(mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dy, int lddy, float* dz, const LayerGrads& g,
                                float* din, int ld_din, const BwdScratch& w, hipStream_t s) {
  const int64_t M = (int64_t)r.B * r.H * r.W;
  const int C = L.Cout;
  HIPCHK(c, launch_bn_bwd_reduce(dy, lddy, L.tscale, L.tshift, r.z, C, L.mean, L.invstd, M, C, w.red, w.sums, g.dbeta, g.dgamma, s));
  // dz and, fused, the column sums of dz (the conv bias gradient, analytically ~0 under BatchNorm): they stay in the reduction slots
  // until conv_wgrad -- the next user of the slots -- folds them inside its unpack launch
  int pend_rows = 0;
  HIPCHK(c, launch_bn_bwd_apply_deferred(dy, lddy, L.tscale, L.tshift, r.z, L.mean, L.invstd, L.gamma, w.sums, M, C, dz, w.red,
                                         &pend_rows, s));
  int rc;
  if ((rc = conv_wgrad(c, L, r, dz, g.dw, w, true, s, &pend_rows, g.dbias))) return rc;
  if (din && (rc = conv_dgrad(c, L, r, dz, din, ld_din, w, true, s))) return rc;
  return MGU_OK;
}

// weight gradient of a conv layer: Z = dz (dense, pitch rup(Cout, 4)), A = gather of the layer's input
int mgud::conv_wgrad(mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dz, float* dw, const BwdScratch& w, bool record,
                     hipStream_t s, int* fold_rows, float* dbias) {
  const int N = rup(L.Cout, 4);
  WgradDesc d = wgrad_desc(c, dz, N, r.in, r.ldin, 0, L.Cp, L.KS, r.B, r.H, r.W, 0, 0, N, w.dwp, w.dwp_floats);
  {
    const double alg = 2.0 * d.M * (double)L.KS * L.KS * L.Cin * L.Cout;
    const WgradKernel k = pick_wgrad(d);
    const WgradCost cost = wgrad_cost(k, alg);
    ProfScope ps(record ? c : nullptr, s, wgrad_kernel_name(k), alg, cost.mfma, cost.pipe);
    HIPCHK(c, launch_wgrad_f32(d, s));
  }
  if (!fold_rows) {
    HIPCHK(c, launch_unpack_conv_grad(w.dwp, d.groups, (size_t)d.N * d.Kp, dw, L.Cout, L.Cin, L.Cp, L.KS, L.Kp, s));
    return MGU_OK;
  }
  // ... and, in the same launch, the fold of the bias gradient's column sums that conv_bn_relu_backward left in the reduction slots
  HIPCHK(c, launch_unpack_conv_grad(w.dwp, d.groups, (size_t)d.N * d.Kp, dw, L.Cout, L.Cin, L.Cp, L.KS, L.Kp, s, w.red, *fold_rows,
                                    L.Cout, dbias));
  *fold_rows = 0;
  return MGU_OK;
}

// data gradient of a conv layer: din = conv(dz, flipped/transposed W) -> out (pitch ldout)
int mgud::conv_dgrad(mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dz, float* out, int ldout, const BwdScratch& w,
                     bool record, hipStream_t s) {
  const int Cop = rup(L.Cout, 4);
  IgemmDesc d = dgrad_desc(c, L, r, dz, Cop, L.wxg_valid ? L.wxg : w.dgp, out, ldout);
  if (L.wug && wino_dgrad_layer(c->tn, L.KS, Cop)) d.wu = L.wug;   // same Winograd kernel, weights flipped + transposed
  // only the weight form the chosen kernel reads is built -- Winograd U or the direct flipped/transposed panel -- unless the layer
  // keeps a current one (normally packed with all the others by the last weight refresh, repack_weights)
  const ConvKernel k = pick_conv(d, 0);
  if (conv_is_wino(k)) {
    if (!L.wug_valid) {
      HIPCHK(c, launch_pack_one(pack_wino(L.w_src, L.wug, L.Cin, L.Cout, Cop, 1, c->tn.wino_prec), s));
      L.wug_valid = true;
    }
  } else if (!L.wxg_valid) {
    if (w.clear) HIPCHK(c, hipMemsetAsync(w.dgp, 0, (size_t)rup(L.Cin, 128) * d.Kp * sizeof(float), s));   // panel rows are padded to 128
    HIPCHK(c, launch_pack_one(pack_dgrad_panel(L.w_src, w.dgp, L.Cout, L.Cin, Cop, L.KS, d.Kp), s));
  }
  const double alg = 2.0 * d.M * (double)L.KS * L.KS * L.Cin * L.Cout;
  const ConvCost cost = conv_cost(k, d);
  ProfScope ps(record ? c : nullptr, s, conv_dgrad_name(k, d), alg, cost.mfma, cost.pipe);
  HIPCHK(c, launch_conv(d, k, 0, s));
  return MGU_OK;
}

// ConvTranspose2d(2, 2) data gradient: the 2x2 stride-2 gather of d(out) (channels at dout, pitch ld_d, on its Hout x Wout grid) -> out
// (dense, pitch Cin).  The forward layer's three-piece kernel in its gather mode (convt_x3.hip) where the shapes allow, else the
// generic tile kernel.
int mgud::convt_dgrad(mgu_ctx* c, const Layer& U, const FwdRecord& r, const float* dout, int ld_d, int Hout, int Wout, float* out,
                      const BwdScratch& w, bool record, hipStream_t s) {
  IgemmDesc q = dgrad_desc(c, U, r, dout, ld_d, w.dgp, out, U.Cin, Hout, Wout);
  if (U.wxg_valid || convt_x3_dgrad_floats(U.Cin, U.Cout) <= w.dgp_floats) q.wu = U.wxg_valid ? U.wxg : w.dgp;
  const ConvKernel k = pick_conv(q, 0);
  if (k != ConvKernel::ConvtX3Dgrad) {
    if (w.clear) HIPCHK(c, hipMemsetAsync(w.dgp, 0, (size_t)rup(U.Cin, 128) * q.Kp * sizeof(float), s));
    HIPCHK(c, launch_pack_one(pack_convt_dgrad_panel(U.w_src, w.dgp, U.Cin, U.Cout, q.Kp), s));
  } else if (!U.wxg_valid) {
    HIPCHK(c, launch_pack_one(pack_convt_x3(U.w_src, w.dgp, U.Cin, U.Cout, 1), s));   // else: packed by the last weight refresh
  }
  const double alg = 2.0 * q.M * (double)q.K * U.Cin;
  const ConvCost cost = conv_cost(k, q);
  ProfScope ps(record ? c : nullptr, s, conv_dgrad_name(k, q), alg, cost.mfma, cost.pipe);
  HIPCHK(c, launch_conv(q, k, 0, s));
  return MGU_OK;
}

// ConvTranspose2d(2, 2) weight gradient: the roles swap -- Z = the layer's INPUT (M, Cin), A = the 2x2 stride-2 gather of d(out)
// (channels [c_off, c_off + Cout) of a pixel with pitch ld_d, on its Hout x Wout grid)
int mgud::convt_wgrad(mgu_ctx* c, const Layer& U, const FwdRecord& r, const float* dout, int ld_d, int c_off, int Hout, int Wout, float* dw,
                      const BwdScratch& w, hipStream_t s) {
  WgradDesc g = wgrad_desc(c, r.in, r.ldin, dout, ld_d, c_off, U.Cout, 2, r.B, r.H, r.W, Hout, Wout, U.Cin, w.dwp, w.dwp_floats);
  HIPCHK(c, launch_wgrad_f32(g, s));
  HIPCHK(c, launch_unpack_convt_grad(w.dwp, g.groups, (size_t)g.N * g.Kp, dw, U.Cin, U.Cout, g.Kp, s));
  return MGU_OK;
}

size_t mgud::train_ws_bytes(const mgu_ctx* c, int B, int H, int W) { return plan_train(c, B, H, W).total; }

int mgud::unet_forward_train(mgu_ctx* c, const float* x, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int B,
                             int H, int W, float* logits, void* const* cat_dev, void* const* feat_dev, hipStream_t s) {
  for (auto& L : c->layers)
    if (!L.w_src || !L.b_src || (!L.bn.empty() && (!L.gamma || !L.run_mean)))
      return fail(c, MGU_ERR_STATE, "training needs the parameter tensors recorded by mgu_unet_load_weights");
  const TPlan p = plan_train(c, B, H, W);
  c->have_train_fwd = false;
  c->want_train = true;    // from now on a weight refresh also packs the data-gradient Winograd sets (repack_weights)
  c->fold_dirty = true;    // this forward updates the BatchNorm running statistics in place: the eval fold is stale
  int rc = ensure(c, &c->tws, &c->tws_bytes, p.total);
  if (rc) return rc;
  if ((rc = ensure_red(c, c->feat << c->depth))) return rc;
  std::vector<int> hs, ws;
  level_dims(H, W, c->depth, hs, ws);
  double* sums = (double*)((char*)c->tws + p.sums);
  double* red = (double*)c->redws;
  for (const Block& b : c->enc) {
    const int i = b.level;
    if (2 * hs[i + 1] != hs[i] || 2 * ws[i + 1] != ws[i])
      HIPCHK(c, hipMemsetAsync(cat_dev[i], 0, (size_t)B * hs[i] * ws[i] * 2 * c->layers[b.conv2].Cout * sizeof(float), s));
  }
  float* xin = at(c, p.xin);
  HIPCHK(c, launch_pack_input(x, xin, 0, B, c->in_ch, c->Cp0, H, W, xs_n, xs_c, xs_h, xs_w, s));

  // conv1 -> BN -> ReLU -> conv2 -> BN -> ReLU of block b on its level, output y with pitch ldy (and, fused where it can be, pooled)
  auto block = [&](const Block& b, const float* in, int ldin, float* y, int ldy, float* pooled) {
    const int i = b.level, C = c->layers[b.conv1].Cout;
    FwdRecord &r1 = c->fwd[b.conv1], &r2 = c->fwd[b.conv2];
    r1 = FwdRecord{in, ldin, at(c, p.z[b.conv1]), at(c, p.y1[b.conv1]), C, B, hs[i], ws[i]};
    r2 = FwdRecord{r1.y, C, at(c, p.z[b.conv2]), y, ldy, B, hs[i], ws[i]};
    int r = conv_bn_relu_train(c, c->layers[b.conv1], r1, sums, red, s);
    if (r) return r;
    return conv_bn_relu_train(c, c->layers[b.conv2], r2, sums, red, s, pooled);
  };
  const float* cur = xin;
  int ld = c->Cp0;
  for (const Block& b : c->enc) {  // encoder
    const int i = b.level, C = c->layers[b.conv1].Cout;
    float* cat = (float*)cat_dev[i];
    float* pooled = at(c, p.pooled[i]);
    if ((rc = block(b, cur, ld, cat, 2 * C, pooled))) return rc;
    cur = pooled, ld = C;
  }
  {  // bottleneck
    float* bott = at(c, p.bott);
    const int C = c->layers[c->bott.conv1].Cout;
    if ((rc = block(c->bott, cur, ld, bott, C, nullptr))) return rc;
    cur = bott, ld = C;
  }
  for (const Block& b : c->dec) {  // decoder
    const int i = b.level, C = c->layers[b.conv1].Cout;
    float* cat = (float*)cat_dev[i];
    float* feat = (float*)feat_dev[i];
    const Layer& U = c->layers[b.up];
    if ((rc = run_layer(c, U, {.in = cur, .ldin = ld, .B = B, .H = hs[i + 1], .W = ws[i + 1], .out = cat, .ldout = 2 * C, .coff = C,
                               .shift = U.shift, .Hout = hs[i], .Wout = ws[i]}, s)))
      return rc;
    c->fwd[b.up] = FwdRecord{cur, ld, nullptr, nullptr, 0, B, hs[i + 1], ws[i + 1]};
    if ((rc = block(b, cat, 2 * C, feat, C, nullptr))) return rc;
    cur = feat, ld = C;
  }
  const Layer& F = c->layers[c->head];
  c->fwd[c->head] = FwdRecord{cur, ld, nullptr, nullptr, 0, B, H, W};
  if (c->ncls <= 4) {
    HIPCHK(c, launch_conv1x1_head(cur, 0, ld, F.Cin, F.w_src, F.b_src, logits, c->ncls, c->ncls, (int64_t)B * H * W, s));
  } else if ((rc = run_layer(c, F, {.in = cur, .ldin = ld, .B = B, .H = H, .W = W, .out = logits, .ldout = c->ncls, .shift = F.shift}, s))) {
    return rc;
  }
  c->tB = B, c->tH = H, c->tW = W;
  c->have_train_fwd = true;
  return MGU_OK;
}

extern "C" {

// invalid data seen by an EARLIER kernel of this context (the word is host-mapped: no synchronisation needed to read it)
static int pending_data_error(mgu_ctx* c) {
  if (c->err_word && *(volatile int*)c->err_word) {
    const int w = *(volatile int*)c->err_word;
    *(volatile int*)c->err_word = 0;
    return fail(c, MGU_ERR_INVALID, "%s", err_word_message(w));
  }
  return MGU_OK;
}

int mgu_cross_entropy(mgu_ctx* c, const void* logits_dev, const int64_t* labels_dev, int64_t npix, int num_classes,
                      float grad_scale, void* dlogits_dev, float* loss_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!logits_dev || !labels_dev || !dlogits_dev || !loss_dev || npix < 1 || num_classes < 1)
    return fail(c, MGU_ERR_INVALID, "bad cross_entropy args");
  HIPCHK(c, hipSetDevice(c->device));
  int rc = pending_data_error(c);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)hip_stream;
  if ((rc = ensure(c, &c->gws, &c->gws_bytes, 256))) return rc;
  int* err_dev = nullptr;
  if ((rc = err_word_dev(c, &err_dev))) return rc;
  HIPCHK(c, launch_ce((const float*)logits_dev, labels_dev, npix, num_classes, -100 /* nn.CrossEntropyLoss default */, grad_scale,
                      (float*)dlogits_dev, rup(num_classes, 4), (double*)c->gws, err_dev, loss_dev, s));
  return MGU_OK;
}

int mgu_sync_check(mgu_ctx* c, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, hipStreamSynchronize((hipStream_t)hip_stream));
  return pending_data_error(c);
}

}  // extern "C"

// exchange != 0: the gradient of every finished block is mean-all-reduced on the context's communicator stream while the
// blocks below it are still being differentiated.  Blocks finish in reverse parameter order (final conv, decoder shallow ->
// deep, bottleneck, encoder deep -> shallow), so the finished part of the flat vector is a suffix that grows downwards;
// it is flushed whenever >= 4 MB are pending (xGMI collectives are latency-bound below that) and once at the end.
static int backward_body(mgu_ctx* c, const void* dlogits_dev, void* flat_grad_dev, void* hip_stream, int exchange) {
  if (!c) return MGU_ERR_INVALID;
  if (!c->have_train_fwd) return fail(c, MGU_ERR_STATE, "mgu_unet_backward needs a preceding mgu_unet_forward(training=1)");
  if (!dlogits_dev || !flat_grad_dev) return fail(c, MGU_ERR_INVALID, "NULL buffer");
  HIPCHK(c, hipSetDevice(c->device));
  {
    int prc = pending_data_error(c);
    if (prc) return prc;
  }
  hipStream_t s = (hipStream_t)hip_stream;
  const int B = c->tB, H = c->tH, W = c->tW;
  const TPlan p = plan_train(c, B, H, W);
  if (p.total > c->tws_bytes) return fail(c, MGU_ERR_STATE, "training workspace changed since the forward");
  std::vector<int> hs, ws;
  level_dims(H, W, c->depth, hs, ws);
  Bwd w;
  w.c = c, w.s = s;
  w.ta = at(c, p.ta), w.tb = at(c, p.tb), w.dwp = at(c, p.dwp), w.dgp = at(c, p.dgp);
  w.dgp_floats = p.dgp_floats;
  w.dwp_floats = p.dwp_floats;
  w.flat = (float*)flat_grad_dev;
  w.sums = (double*)((char*)c->tws + p.sums);
  w.red = (double*)c->redws;
  float* tc = at(c, p.tc);
  int rc;
  int64_t pend_hi = c->nparams;   // flat[pend_lo, pend_hi) is finished but not yet exchanged
  auto block_done = [&](int64_t lo, bool last) -> int {
    if (!exchange) return MGU_OK;
    if (!last && (pend_hi - lo) < (1 << 20)) return MGU_OK;
    int r = comm_bucket(c, w.flat, lo, pend_hi, s);
    pend_hi = lo;
    return r;
  };

  // ---- final 1x1 conv (unet_decoder.py:143) ------------------------------------------------------
  const Layer& F = c->layers[c->head];
  const int ldd = rup(c->ncls, 4);
  const float* dlog = (const float*)dlogits_dev;
  HIPCHK(c, launch_colsum(dlog, ldd, (int64_t)B * H * W, ldd, w.red, (float*)w.sums, s));   // padded to ldd columns, then trimmed
  HIPCHK(c, hipMemcpyAsync(w.flat + F.off_b, w.sums, sizeof(float) * c->ncls, hipMemcpyDeviceToDevice, s));
  if ((rc = conv_wgrad(c, F, c->fwd[c->head], dlog, w.flat + F.off_w, w, false, s))) return rc;
  // the panel of the data gradient: normally already packed with every other weight form by the last refresh (repack_weights)
  if ((rc = conv_dgrad(c, F, c->fwd[c->head], dlog, tc, F.Cin, w, false, s))) return rc;
  const float* dy = tc;
  int lddy = F.Cin;
  if ((rc = block_done(F.off_w, false))) return rc;

  // ---- decoder blocks, shallow -> deep (reverse of unet_decoder.py:139-141) ------------------------
  for (auto b = c->dec.rbegin(); b != c->dec.rend(); ++b) {
    const int i = b->level, C = c->layers[b->conv1].Cout;
    const Layer& U = c->layers[b->up];
    float* dcat = at(c, p.dcat[i]);
    if ((rc = block_backward(w, *b, dy, lddy, dcat, 2 * C))) return rc;
    // ConvTranspose2d backward (unet_decoder.py:36): d(up) = channels [C, 2C) of d(cat)
    const int64_t Mi = (int64_t)B * hs[i] * ws[i];
    if (2 * hs[i + 1] != hs[i] || 2 * ws[i + 1] != ws[i])  // F.pad backward (unet_decoder.py:46-47) drops the pad row/col
      HIPCHK(c, launch_zero_pad_region(dcat, 2 * C, C, C, B, hs[i], ws[i], 2 * hs[i + 1], 2 * ws[i + 1], s));
    HIPCHK(c, launch_colsum(dcat + C, 2 * C, Mi, C, w.red, w.flat + U.off_b, s));
    if ((rc = convt_wgrad(c, U, c->fwd[b->up], dcat, 2 * C, C, hs[i], ws[i], w.flat + U.off_w, w, s))) return rc;
    if ((rc = convt_dgrad(c, U, c->fwd[b->up], dcat + C, 2 * C, hs[i], ws[i], tc, w, true, s))) return rc;
    dy = tc, lddy = U.Cin;
    if ((rc = block_done(U.off_w, false))) return rc;
  }
  // ---- bottleneck -----------------------------------------------------------------------------------
  {
    const Layer& L1 = c->layers[c->bott.conv1];
    if ((rc = block_backward(w, c->bott, dy, lddy, tc, L1.Cin))) return rc;
    if ((rc = block_done(L1.off_w, false))) return rc;
  }
  // ---- encoder blocks, deep -> shallow -----------------------------------------------------------------
  for (auto b = c->enc.rbegin(); b != c->enc.rend(); ++b) {
    const int i = b->level, C = c->layers[b->conv1].Cout;
    const bool first = b + 1 == c->enc.rend();
    float* dcat = at(c, p.dcat[i]);
    // d(skip) = d(cat)[:, :C] (decoder path) + MaxPool backward of d(pooled); the skip is conv2's y, in the concat buffer
    const FwdRecord& r2 = c->fwd[b->conv2];
    HIPCHK(c, launch_maxpool2_bwd_add(r2.y, r2.ldy, tc, dcat, 2 * C, B, hs[i], ws[i], C, s));
    const Layer& L1 = c->layers[b->conv1];
    if ((rc = block_backward(w, *b, dcat, 2 * C, first ? nullptr : tc, L1.Cin))) return rc;
    if ((rc = block_done(L1.off_w, first))) return rc;
  }
  if (exchange && (rc = comm_join(c, s))) return rc;   // the caller's stream continues after the last bucket
  return MGU_OK;
}

static int backward_impl(mgu_ctx* c, const void* dlogits_dev, void* flat_grad_dev, void* hip_stream, int exchange) {
  const int rc = red_cleared_on_error(c, backward_body(c, dlogits_dev, flat_grad_dev, hip_stream, exchange), (hipStream_t)hip_stream);
  if (rc != MGU_OK && exchange && c && c->comm) {
    // an error return after some buckets were issued: the caller's stream must still be ordered behind the communicator
    // stream (the buckets read and write flat_grad_dev), or the caller could free / reuse the buffer under a running collective
    const std::string keep = c->err;
    (void)comm_join(c, (hipStream_t)hip_stream);
    c->err = keep;
  }
  return rc;
}

extern "C" {

int mgu_unet_backward(mgu_ctx* c, const void* dlogits_dev, void* flat_grad_dev, void* hip_stream) {
  return backward_impl(c, dlogits_dev, flat_grad_dev, hip_stream, 0);
}

int mgu_unet_backward_allreduce(mgu_ctx* c, const void* dlogits_dev, void* flat_grad_dev, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!c->comm) return fail(c, MGU_ERR_STATE, "mgu_unet_backward_allreduce needs mgu_comm_init_rank on this context");
  return backward_impl(c, dlogits_dev, flat_grad_dev, hip_stream, 1);
}

// ---- test hook: the record of the last train-mode forward, read-only ---------------------------------------------------------------
// the layer whose state_dict prefix (Layer::prefix + Layer::conv) is `name`, or -1
static int record_layer(const mgu_ctx* c, const char* name) {
  const std::string key(name);
  for (size_t i = 0; i < c->layers.size(); ++i)
    if (key == c->layers[i].prefix + c->layers[i].conv) return (int)i;
  return -1;
}

int mgu_unet_train_record_dims(mgu_ctx* c, const char* layer, int* B_out, int* H_out, int* W_out, int* Cin_out, int* Cout_out) {
  if (!c) return MGU_ERR_INVALID;
  if (!layer || !B_out || !H_out || !W_out || !Cin_out || !Cout_out) return fail(c, MGU_ERR_INVALID, "NULL argument");
  if (!c->have_train_fwd) return fail(c, MGU_ERR_STATE, "mgu_unet_train_record_dims needs a preceding mgu_unet_forward(training=1)");
  const int i = record_layer(c, layer);
  if (i < 0) return fail(c, MGU_ERR_INVALID, "no layer named '%s'", layer);
  const FwdRecord& r = c->fwd[i];
  *B_out = r.B, *H_out = r.H, *W_out = r.W, *Cin_out = c->layers[i].Cin, *Cout_out = c->layers[i].Cout;
  return MGU_OK;
}

int mgu_unet_train_record_copy(mgu_ctx* c, const char* layer, void* in_dev, void* z_dev, void* y_dev, void* mean_dev, void* invstd_dev,
                               void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!layer) return fail(c, MGU_ERR_INVALID, "NULL layer name");
  if (!c->have_train_fwd) return fail(c, MGU_ERR_STATE, "mgu_unet_train_record_copy needs a preceding mgu_unet_forward(training=1)");
  const int i = record_layer(c, layer);
  if (i < 0) return fail(c, MGU_ERR_INVALID, "no layer named '%s'", layer);
  const Layer& L = c->layers[i];
  const FwdRecord& r = c->fwd[i];
  if ((z_dev || y_dev || mean_dev || invstd_dev) && (L.bn.empty() || !r.z || !r.y))
    return fail(c, MGU_ERR_INVALID, "layer '%s' has no BatchNorm: it records its input only", layer);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  const size_t M = (size_t)r.B * r.H * r.W, f = sizeof(float);
  // M rows of n floats from pitch ld to a dense tensor
  auto rows = [&](void* dst, const float* src, int ld, int n) {
    return hipMemcpy2DAsync(dst, n * f, src, ld * f, n * f, M, hipMemcpyDeviceToDevice, s);
  };
  if (in_dev) HIPCHK(c, rows(in_dev, r.in, r.ldin, L.Cin));
  if (z_dev) HIPCHK(c, rows(z_dev, r.z, L.Cout, L.Cout));
  if (y_dev) HIPCHK(c, rows(y_dev, r.y, r.ldy, L.Cout));
  if (mean_dev) HIPCHK(c, hipMemcpyAsync(mean_dev, L.mean, L.Cout * f, hipMemcpyDeviceToDevice, s));
  if (invstd_dev) HIPCHK(c, hipMemcpyAsync(invstd_dev, L.invstd, L.Cout * f, hipMemcpyDeviceToDevice, s));
  return MGU_OK;
}

int mgu_adam_step(mgu_ctx* c, void* flat_param_dev, const void* flat_grad_dev, void* exp_avg_dev, void* exp_avg_sq_dev,
                  int64_t n, float lr, double beta1, double beta2, float eps, float weight_decay, int step, float grad_scale,
                  void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!flat_param_dev || !flat_grad_dev || !exp_avg_dev || !exp_avg_sq_dev || n < 0 || step < 1)
    return fail(c, MGU_ERR_INVALID, "bad adam args (step counts from 1)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_adam((float*)flat_param_dev, (const float*)flat_grad_dev, (float*)exp_avg_dev, (float*)exp_avg_sq_dev, n, lr,
                        beta1, beta2, eps, weight_decay, step, grad_scale, (hipStream_t)hip_stream));
  return MGU_OK;
}

int mgu_sgd_step(mgu_ctx* c, void* flat_param_dev, const void* flat_grad_dev, void* momentum_buf_dev, int64_t n, float lr,
                 float momentum, float weight_decay, int step, float grad_scale, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!flat_param_dev || !flat_grad_dev || (momentum != 0.f && !momentum_buf_dev) || n < 0 || step < 1 || momentum < 0.f)
    return fail(c, MGU_ERR_INVALID, "bad sgd args (step counts from 1; a momentum buffer when momentum != 0)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_sgd((float*)flat_param_dev, (const float*)flat_grad_dev, (float*)momentum_buf_dev, n, lr, momentum, weight_decay,
                       step, grad_scale, (hipStream_t)hip_stream));
  return MGU_OK;
}

}  // extern "C"
