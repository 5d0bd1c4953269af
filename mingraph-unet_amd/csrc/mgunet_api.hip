// C-ABI of libmgunet.so (see include/mgunet.h): context, weight repacking, U-Net forward schedule,
// GAT layer schedule.  Host orchestration only -- every arithmetic op is a kernel in igemm.hip,
// elementwise.hip or gat.hip.  No CPU fallback exists: without a HIP device every call fails.
#include "ctx.h"

#include <algorithm>

using namespace mgu;
using namespace mgud;

namespace mgud {
std::string g_create_err;
}

namespace {

struct WsPlan {
  size_t xin, tmp, tmp_slice, bott, total;
  std::vector<size_t> pooled;
};

// Image groups of an eval forward (Tuning::fwd_groups): two once the batch has an image for each.  Group g walks images
// [g * group_images, ...) of the batch.
int fwd_groups(const mgu_ctx* c, int B) { return c->tn.fwd_groups >= 2 && B >= 2 ? 2 : 1; }
int group_images(const mgu_ctx* c, int B) { return (B + fwd_groups(c, B) - 1) / fwd_groups(c, B); }

WsPlan plan_ws(const mgu_ctx* c, int B, int H, int W) {
  std::vector<int> hs, wsz;
  level_dims(H, W, c->depth, hs, wsz);
  // elements of a block's output (Cout channels) on level l
  auto out = [&](const Block& b, int l) { return (size_t)B * hs[l] * wsz[l] * c->layers[b.conv2].Cout; };
  WsPlan p;
  Carve k;
  const size_t es = c->dtype == MGU_DTYPE_BF16 ? 2 : 4;
  p.xin = k.take((size_t)B * H * W * c->Cp0 * es);
  size_t tmax = out(c->bott, c->bott.level);
  for (const Block& b : c->enc) tmax = std::max(tmax, out(b, b.level));
  // the conv1 temporary: one fixed slice per image group, each holding group_images images of the largest level (the groups are on
  // different levels at the same time, so a region indexed by global image number with each level's geometry would overlap)
  const int G = fwd_groups(c, B);
  p.tmp_slice = (tmax / B * group_images(c, B) * es + 255) / 256 * 256;
  p.tmp = k.take(G == 1 ? tmax * es : G * p.tmp_slice);
  for (const Block& b : c->enc) p.pooled.push_back(k.take(out(b, b.level + 1) * es));
  p.bott = k.take(out(c->bott, c->bott.level) * es);
  p.total = k.off;
  return p;
}

// Every weight form layer L keeps in the arena, in arena order: form(pointer, floats) once per form the layer holds.  It also makes
// the layer's kernel-form decisions (wino, ctx3, ctb, first).  The one list sizes the arena and hands out its pointers.
template <class F>
void weight_forms(const mgu_ctx* c, Layer& L, F form) {
  const int dtype = c->dtype;
  L.wino = dtype == MGU_DTYPE_F32 && !L.convt && wino_layer(c->tn, L.KS, L.Cp);   // Winograd F(2x2,3x3) layers (wino_f32.hip)
  // fp32 ConvTranspose on fragment-ordered three-piece weights (convt_x3.hip).  (A bf16-storage sibling of that kernel -- one
  // fragment per operand straight from global memory -- was measured SLOWER than the LDS-tiled generic kernel, 0.178 vs 0.163 ms per
  // step: 32-byte row segments per K slice; not kept.)
  L.ctx3 = dtype == MGU_DTYPE_F32 && L.convt && convt_x3_layer(c->tn, L.Cin, L.Cout);
  // bf16 storage: the layer's weights as bf16 MFMA fragments for convt2x2_bf16_kernel (whole-row LDS staging, transposed 16-byte stores)
  L.ctb = dtype == MGU_DTYPE_BF16 && L.convt && convt_bf16f_layer(c->tn, L.Cin, L.Cout);
  L.first = !L.convt && L.KS == 3 && first_conv_applicable(dtype, L.Cin, L.Cp, L.Cout, 8, 0);
  form(L.wp, (size_t)L.Np * L.Kp);
  form(L.scale, (size_t)L.Np);
  form(L.shift, (size_t)L.Np);
  if (L.wino) form(L.wu, wino_u_floats(L.Cout, L.Cp));
  if (L.wino && rup(L.Cout, 4) % 16 == 0) form(L.wug, wino_u_floats(L.Cin, rup(L.Cout, 4)));   // data-gradient conv: roles swapped
  if (L.ctx3) form(L.wu, convt_x3_floats(L.Cin, L.Cout));
  if (L.ctb) form(L.wu, convt_bf16f_floats(L.Cin, L.Cout));
  if (L.ctx3) form(L.wxg, convt_x3_dgrad_floats(L.Cin, L.Cout));
  if (dtype == MGU_DTYPE_F32 && !L.convt && L.bn.empty())   // final conv: data-gradient panel
    form(L.wxg, (size_t)rup(L.Cin, 128) * rup(L.KS * L.KS * rup(L.Cout, 4), 32));
  if (L.first) form(L.wf, 9 * 4 * (size_t)L.Cout);
  if (L.first) form(L.wfm, first_mfma_floats());
  if (!L.bn.empty()) {   // batch statistics of the training forward
    form(L.mean, (size_t)L.Np);
    form(L.invstd, (size_t)L.Np);
    form(L.tscale, (size_t)L.Np);
    form(L.tshift, (size_t)L.Np);
  }
}

}  // namespace

extern "C" {

const char* mgu_version(void) { return "mgunet 0.2 (gfx950: fp32 Winograd / bf16 MFMA forward, fp32 training step, GAT, RCCL gradient exchange)"; }

int mgu_create(int device_id, mgu_ctx** out) {
  if (!out) return fail(nullptr, MGU_ERR_INVALID, "out == NULL");
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(nullptr, MGU_ERR_HIP, "no HIP device available (%s): libmgunet has no CPU fallback",
                e != hipSuccess ? hipGetErrorString(e) : "device count 0");
  if (device_id < 0 || device_id >= n) return fail(nullptr, MGU_ERR_INVALID, "device %d out of range [0,%d)", device_id, n);
  e = hipSetDevice(device_id);
  if (e != hipSuccess) return fail(nullptr, MGU_ERR_HIP, "hipSetDevice: %s", hipGetErrorString(e));
  mgu_ctx* c = new mgu_ctx();
  c->device = device_id;
  // kernel-selection switches live in the context (no process globals: two contexts never see each other's settings)
  auto flag = [](const char* name) { const char* v = getenv(name); return v && v[0] == '1'; };
  auto num = [](const char* name, int dflt) { const char* v = getenv(name); return v && v[0] ? atoi(v) : dflt; };
  Tuning& t = c->tn;
  t.first_mfma = !flag("MGU_NO_FIRST_MFMA");
  t.use_wino = !flag("MGU_NO_WINOGRAD");
  t.wino_prec = num("MGU_WINO_PREC", t.wino_prec) ? 1 : 0;
  t.wino_cp = !flag("MGU_NO_WINO_CP");
  t.convt_frag = !flag("MGU_NO_CONVT_FRAG");
  t.wino_ppb_cap = std::max(1, num("MGU_WINO_PPB_CAP", 32));
  t.wgrad_halo = !flag("MGU_NO_WGRAD_HALO");
  t.wino_wgrad = !flag("MGU_NO_WINO_WGRAD");
  t.wgrad_x3 = !flag("MGU_NO_WGRAD_X3");
  t.convt_dgrad_x3 = !flag("MGU_NO_CONVT_DGRAD_X3");
  t.wgrad_thin = !flag("MGU_NO_THIN_WGRAD");
  t.wino_dgrad = !flag("MGU_NO_WINO_DGRAD");
  t.gat_fused = !flag("MGU_NO_GAT_FUSED");
  t.wino_asm = num("MGU_WINO_ASM", 1) > 0;
  t.convt_asm = num("MGU_CONVT_ASM", 1) > 0;
  t.head_fused = num("MGU_HEAD_FUSED", 1) > 0;
  t.fwd_groups = num("MGU_FWD_GROUPS", t.fwd_groups) >= 2 ? 2 : 1;
  t.lovasz_passes = num("MGU_LOVASZ_PASSES", t.lovasz_passes) == 3 ? 3 : 4;
  *out = c;
  return MGU_OK;
}

void mgu_destroy(mgu_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();
  (void)mgu_comm_destroy(c);
  if (c->arena) (void)hipFree(c->arena);
  if (c->ws) (void)hipFree(c->ws);
  if (c->gws) (void)hipFree(c->gws);
  if (c->pmws) (void)hipFree(c->pmws);
  if (c->gbws) (void)hipFree(c->gbws);
  if (c->pack_dev) (void)hipFree(c->pack_dev);
  if (c->tws) (void)hipFree(c->tws);
  if (c->redws) (void)hipFree(c->redws);
  if (c->wuws) (void)hipFree(c->wuws);
  if (c->ncws) (void)hipFree(c->ncws);
  if (c->objws) (void)hipFree(c->objws);
  if (c->labtab) (void)hipFree(c->labtab);
  if (c->lossws) (void)hipFree(c->lossws);
  if (c->imgws) (void)hipFree(c->imgws);
  if (c->optws) (void)hipFree(c->optws);
  gat_destroy(c);
  if (c->err_word) (void)hipHostFree(c->err_word);
  for (auto e : c->ev) (void)hipEventDestroy(e);
  for (auto e : c->ev_total)
    if (e) (void)hipEventDestroy(e);
  for (auto e : c->fwd_ev)
    if (e) (void)hipEventDestroy(e);
  if (c->fwd_stream) (void)hipStreamDestroy(c->fwd_stream);
  delete c;
}

const char* mgu_last_error(mgu_ctx* c) { return c ? c->err.c_str() : g_create_err.c_str(); }

int mgu_unet_configure(mgu_ctx* c, int in_ch, int ncls, int feat, int depth, int dtype) {
  if (!c) return MGU_ERR_INVALID;
  if (in_ch < 1 || ncls < 1 || feat < 4 || (feat & 3) || depth < 1 || depth > 8)
    return fail(c, MGU_ERR_INVALID, "unsupported UNet(%d,%d,%d,%d): init_features must be a positive multiple of 4, depth 1..8",
                in_ch, ncls, feat, depth);
  if (dtype != MGU_DTYPE_F32 && dtype != MGU_DTYPE_BF16) return fail(c, MGU_ERR_INVALID, "unknown dtype %d", dtype);
  if (dtype == MGU_DTYPE_BF16 && ((feat & 7) || ncls > 4))
    return fail(c, MGU_ERR_INVALID, "bf16 storage needs init_features %% 8 == 0 (16-byte lanes of 8 bf16) and <= 4 classes");
  HIPCHK(c, hipSetDevice(c->device));
  c->in_ch = in_ch, c->ncls = ncls, c->feat = feat, c->depth = depth, c->dtype = dtype;
  c->Cp0 = rup(in_ch, dtype == MGU_DTYPE_BF16 ? 8 : 4);
  c->layers.clear();
  c->enc.clear();
  c->dec.clear();
  auto add = [&](const std::string& prefix, const char* conv, const char* bn, int cin, int cp, int cout, int KS, bool convt, int level) {
    Layer L = make_layer(dtype, cin, cp, cout, KS, convt);
    L.prefix = prefix, L.conv = conv, L.bn = bn, L.level = level;
    c->layers.push_back(L);
    return (int)c->layers.size() - 1;
  };
  auto add_block = [&](const std::string& prefix, int cin, int cp, int cout, int level, int up) {  // ConvBlock, unet_encoder.py:4-25
    Block b;
    b.up = up, b.level = level;
    b.conv1 = add(prefix, "conv1", "bn1", cin, cp, cout, 3, false, level);
    b.conv2 = add(prefix, "conv2", "bn2", cout, cout, cout, 3, false, level);
    return b;
  };
  int cin = in_ch, cp = c->Cp0, f = feat;
  for (int i = 0; i < depth; ++i) {  // unet_encoder.py:46-50
    c->enc.push_back(add_block("encoder.encoder_blocks." + std::to_string(i) + ".", cin, cp, f, i, -1));
    cin = cp = f;
    f *= 2;
  }
  c->bott = add_block("encoder.bottleneck.", cin, cp, f, depth, -1);  // :53
  int prev = f;
  for (int b = 0; b < depth; ++b) {  // unet_decoder.py:103-114
    const int i = depth - 1 - b, ci = feat << i;
    const std::string prefix = "decoder.decoder_blocks." + std::to_string(b) + ".";
    const int up = add(prefix, "upsample", "", prev, prev, prev / 2, 1, true, i + 1);
    c->dec.push_back(add_block(prefix + "conv_block.", ci + prev / 2, ci + prev / 2, ci, i, up));
    prev = ci;
  }
  c->head = add("decoder.", "final_conv", "", prev, prev, ncls, 1, false, 0);  // unet_decoder.py:117
  c->fwd.assign(c->layers.size(), FwdRecord{});
  // flat parameter order = the reference's named_parameters(): per ConvBlock conv1.{w,b}, conv2.{w,b},
  // bn1.{w,b}, bn2.{w,b} (unet_encoder.py:7-13); decoder block: upsample.{w,b} then its conv_block; final.
  {
    int64_t off = 0;
    auto conv = [&](Layer& L) {
      L.off_w = off, off += (int64_t)L.Cout * L.Cin * L.KS * L.KS * (L.convt ? 4 : 1);
      L.off_b = off, off += L.Cout;
    };
    auto bn = [&](Layer& L) {
      L.off_gamma = off, off += L.Cout;
      L.off_beta = off, off += L.Cout;
    };
    auto block = [&](const Block& b) {
      if (b.up >= 0) conv(c->layers[b.up]);
      conv(c->layers[b.conv1]), conv(c->layers[b.conv2]);
      bn(c->layers[b.conv1]), bn(c->layers[b.conv2]);
    };
    for (const Block& b : c->enc) block(b);
    block(c->bott);
    for (const Block& b : c->dec) block(b);
    conv(c->layers[c->head]);
    c->nparams = off;
  }
  // one walk over every layer's weight forms sizes the arena, a second hands out its pointers
  size_t total = 0;
  for (auto& L : c->layers) weight_forms(c, L, [&](float*&, size_t n) { total += n; });
  if (c->arena) HIPCHK(c, hipFree(c->arena));
  c->arena = nullptr;
  HIPCHK(c, hipMalloc((void**)&c->arena, total * sizeof(float)));
  HIPCHK(c, hipMemset(c->arena, 0, total * sizeof(float)));
  c->arena_floats = total;
  float* p = c->arena;
  for (auto& L : c->layers) weight_forms(c, L, [&](float*& form, size_t n) { form = p, p += n; });
  c->configured = true;
  c->have_train_fwd = false;
  c->loaded = false;
  return MGU_OK;
}

int64_t mgu_unet_param_count(mgu_ctx* c) {
  if (!c || !c->configured) return -1;
  return c->nparams;
}

int64_t mgu_unet_param_offset(mgu_ctx* c, const char* name) {
  if (!c || !c->configured || !name) return -1;
  const std::string key(name);
  for (auto& L : c->layers) {
    if (key == L.prefix + L.conv + ".weight") return L.off_w;
    if (key == L.prefix + L.conv + ".bias") return L.off_b;
    if (!L.bn.empty()) {
      if (key == L.prefix + L.bn + ".weight") return L.off_gamma;
      if (key == L.prefix + L.bn + ".bias") return L.off_beta;
    }
  }
  return -1;
}

int mgu_unet_load_weights(mgu_ctx* c, const mgu_tensor_desc* named, int n, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!c->configured) return fail(c, MGU_ERR_STATE, "mgu_unet_configure must precede mgu_unet_load_weights");
  if (!named || n <= 0) return fail(c, MGU_ERR_INVALID, "empty state_dict");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  std::map<std::string, const mgu_tensor_desc*> sd;
  for (int i = 0; i < n; ++i)
    if (named[i].name) sd[named[i].name] = &named[i];
  auto get = [&](const std::string& key, int64_t numel, const float** out) -> int {
    auto it = sd.find(key);
    if (it == sd.end()) return fail(c, MGU_ERR_INVALID, "state_dict is missing key '%s'", key.c_str());
    if (it->second->numel != numel)
      return fail(c, MGU_ERR_INVALID, "state_dict key '%s' has %lld elements, expected %lld", key.c_str(),
                  (long long)it->second->numel, (long long)numel);
    if (!it->second->ptr) return fail(c, MGU_ERR_INVALID, "state_dict key '%s' has a NULL pointer", key.c_str());
    *out = (const float*)it->second->ptr;
    return MGU_OK;
  };
  for (auto& L : c->layers) {
    const float *w, *b;
    const std::string cw = L.prefix + L.conv;
    int rc;
    if (L.convt) {
      if ((rc = get(cw + ".weight", (int64_t)L.Cin * L.Cout * 4, &w))) return rc;
      if ((rc = get(cw + ".bias", L.Cout, &b))) return rc;
      L.w_src = w, L.b_src = b;
    } else {
      if ((rc = get(cw + ".weight", (int64_t)L.Cout * L.Cin * L.KS * L.KS, &w))) return rc;
      if ((rc = get(cw + ".bias", L.Cout, &b))) return rc;
      L.w_src = w, L.b_src = b;
      if (!L.bn.empty()) {
        const float *g, *be, *rm, *rv;
        const std::string bn = L.prefix + L.bn;
        if ((rc = get(bn + ".weight", L.Cout, &g))) return rc;
        if ((rc = get(bn + ".bias", L.Cout, &be))) return rc;
        if ((rc = get(bn + ".running_mean", L.Cout, &rm))) return rc;
        if ((rc = get(bn + ".running_var", L.Cout, &rv))) return rc;
        L.gamma = g, L.beta = be, L.run_mean = const_cast<float*>(rm), L.run_var = const_cast<float*>(rv);
      }
    }
  }
  int rc = repack_weights(c, s);
  if (rc) return rc;
  c->loaded = true;
  return MGU_OK;
}

int mgu_unet_refresh_weights(mgu_ctx* c, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!c->configured || !c->loaded) return fail(c, MGU_ERR_STATE, "mgu_unet_refresh_weights needs a preceding mgu_unet_load_weights");
  HIPCHK(c, hipSetDevice(c->device));
  return repack_weights(c, (hipStream_t)hip_stream);
}

int mgu_unet_workspace_bytes(mgu_ctx* c, int B, int H, int W, int training, size_t* out) {
  if (!c || !out) return MGU_ERR_INVALID;
  if (!c->configured) return fail(c, MGU_ERR_STATE, "not configured");
  // eval: packed input, one conv1 temp, pooled tensors, bottleneck; training: every layer's z / y kept for backward,
  // gradient temporaries and the weight-gradient partial panels (mgunet_train.hip)
  *out = training ? train_ws_bytes(c, B, H, W) : plan_ws(c, B, H, W).total;
  return MGU_OK;
}

int mgu_unet_reserve(mgu_ctx* c, int B, int H, int W, int training) {
  size_t need = 0;
  int rc = mgu_unet_workspace_bytes(c, B, H, W, training, &need);
  if (rc) return rc;
  HIPCHK(c, hipSetDevice(c->device));
  return training ? ensure(c, &c->tws, &c->tws_bytes, need) : ensure(c, &c->ws, &c->ws_bytes, need);
}

}  // extern "C"

// Every packed weight form from the parameter tensors recorded by mgu_unet_load_weights (their CONTENTS may have changed: an
// optimizer step through the flat buffer).  All Winograd sets -- and, once the context has trained, the data-gradient sets --
// go out in one launch; the eval BatchNorm fold stays lazy.
int mgud::repack_weights(mgu_ctx* c, hipStream_t s) {
  std::vector<PackItem> items;   // every form goes out in the one pack_batch_kernel launch (pack.hip)
  for (auto& L : c->layers) {
    const float *w = L.w_src, *b = L.b_src;
    L.wxg_valid = false;
    if (L.convt) {
      // the generic panel is read by the fallback kernels only: built on first use when the layer runs on its three-piece fragments
      L.wp_dirty = L.ctx3;
      if (!L.ctx3) items.push_back(pack_convt_panel(w, L.wp, c->dtype, L.Cin, L.Cout, L.Kp));
      if (L.ctb) items.push_back(pack_convt_bf16f(w, L.wu, L.Cin, L.Cout));
      if (L.ctx3) items.push_back(pack_convt_x3(w, L.wu, L.Cin, L.Cout, 0));
      items.push_back(pack_bias_tile(b, L.shift, L.Cout, 4));   // scale unused (nullptr at launch)
      if (L.wxg && c->want_train && convt_x3_dgrad_layer(c->tn, L.Cin, L.Cout)) {
        items.push_back(pack_convt_x3(w, L.wxg, L.Cin, L.Cout, 1));
        L.wxg_valid = true;
      }
    } else {
      // a layer that runs as Winograd / first-conv / 1x1 head kernel reads wu / wf / w_src; its direct panel is packed lazily, only
      // if a launch ever falls back to the implicit-GEMM kernel (run_layer)
      L.wp_dirty = true;
      if (L.wu) items.push_back(pack_wino(w, L.wu, L.Cout, L.Cin, L.Cp, 0, c->tn.wino_prec));
      L.wug_valid = false;
      if (L.wug && c->want_train && wino_dgrad_layer(c->tn, L.KS, rup(L.Cout, 4))) {
        items.push_back(pack_wino(w, L.wug, L.Cin, L.Cout, rup(L.Cout, 4), 1, c->tn.wino_prec));
        L.wug_valid = true;
      }
      const bool head_kernel = L.bn.empty() && c->ncls <= 4;   // conv1x1_head_kernel reads the reference's (ncls, C) weight itself
      if (!L.wu && !L.first && !head_kernel) {
        items.push_back(pack_conv_panel(w, L.wp, c->dtype, L.Cout, L.Cin, L.Cp, L.KS, L.Kp));
        L.wp_dirty = false;
      }
      if (L.wf) items.push_back(pack_first_w(w, L.wf, L.Cout, L.Cin));
      if (L.wfm && L.Cout == 32 && L.Cin <= 3) items.push_back(pack_first_mfma(w, L.wfm, L.Cout, L.Cin));
      if (!L.bn.empty()) c->fold_dirty = true;   // eval scale/shift are folded lazily by the next eval forward (training never reads them)
      else items.push_back(pack_bias_tile(b, L.shift, L.Cout, 1));
      if (L.bn.empty() && L.wxg && c->want_train) {   // final conv: panel of its data gradient (mgu_unet_backward)
        const int Cop = rup(L.Cout, 4);
        items.push_back(pack_dgrad_panel(w, L.wxg, L.Cout, L.Cin, Cop, L.KS, rup(L.KS * L.KS * Cop, 32)));
        L.wxg_valid = true;
      }
    }
  }
  // batches of <= PACK_MAX items; the tables are uploaded only when they differ from what the device already holds (a
  // refresh after an optimizer step finds them unchanged: same tensors, same buffers)
  std::vector<PackBatch> batches;
  for (size_t i0 = 0; i0 < items.size(); i0 += PACK_MAX) {
    PackBatch b;
    memset(&b, 0, sizeof b);
    b.n = (int)std::min<size_t>(PACK_MAX, items.size() - i0);
    for (int i = 0; i < b.n; ++i) b.it[i] = items[i0 + i];
    if (!pack_batch_prepare(b)) return fail(c, MGU_ERR_STATE, "internal: a weight form is not packable");
    batches.push_back(b);
  }
  const bool same = batches.size() == c->pack_host.size() &&
                    (batches.empty() || memcmp(batches.data(), c->pack_host.data(), batches.size() * sizeof(PackBatch)) == 0);
  if (!same) {
    if ((int)batches.size() > c->pack_dev_cap) {
      if (c->pack_dev) HIPCHK(c, hipFree(c->pack_dev));
      c->pack_dev = nullptr;
      HIPCHK(c, hipMalloc((void**)&c->pack_dev, batches.size() * sizeof(PackBatch)));
      c->pack_dev_cap = (int)batches.size();
    }
    HIPCHK(c, hipStreamSynchronize(s));   // an earlier launch may still read the old table
    HIPCHK(c, hipMemcpy(c->pack_dev, batches.data(), batches.size() * sizeof(PackBatch), hipMemcpyHostToDevice));
    c->pack_host = batches;
  }
  for (size_t k = 0; k < batches.size(); ++k) HIPCHK(c, launch_pack_batch(c->pack_dev + k, batches[k].total_blocks, s));
  return MGU_OK;
}

int mgud::run_layer(mgu_ctx* c, const Layer& L, const ConvReq& q, hipStream_t s, const ConvFusions& f, ConvTaken* took) {
  IgemmDesc d = layer_desc(c, L, q.in, q.ldin, q.B, q.H, q.W, q.out, q.ldout, q.coff);
  d.scale = q.scale, d.shift = q.shift, d.relu = q.relu, d.Hout = q.Hout, d.Wout = q.Wout;
  ConvTaken t;
  if (took) *took = t;
  if (L.wfm && c->tn.first_mfma && q.ldin == L.Cp && first_mfma_applicable(c->dtype, L.Cin, L.Cp, L.Cout, q.ldout, q.coff, q.H, q.W)) {
    const double alg = 2.0 * d.M * 9.0 * L.Cin * L.Cout;
    ProfScope ps(c, s, "conv3x3_first_mfma_kernel", alg, 2.0 * d.M * 32.0 * 32.0 * (c->dtype == MGU_DTYPE_F32 ? 6.0 : 3.0), 1);
    HIPCHK(c, launch_first_mfma(c->dtype, q.in, L.wfm, q.scale, q.shift, q.out, q.B, q.H, q.W, q.ldout, q.coff, q.relu, s));
    return MGU_OK;
  }
  if (L.wf && q.ldin == L.Cp && first_conv_applicable(c->dtype, L.Cin, L.Cp, L.Cout, q.ldout, q.coff) &&
      (int64_t)q.B * q.H * q.W * std::max(q.ldout, 8) < (1ll << 31)) {
    ProfScope ps(c, s, "conv3x3_first_kernel", 2.0 * d.M * 9.0 * L.Cin * L.Cout, 0, -1);
    HIPCHK(c, launch_first_conv(c->dtype, q.in, L.wf, q.scale, q.shift, q.out, q.B, q.H, q.W, L.Cin, L.Cout, q.ldout, q.coff, q.relu, s));
    return MGU_OK;
  }
  ConvKernel k = pick_conv(d, c->dtype, f.head);
  // the Winograd epilogue also accumulates sum z, sum z^2: one accumulator row per workgroup, so only while the launch's grid fits
  // the table (>= 19 images of 512^2 or 5 of 1024^2 per GPU on the full-resolution 32-channel layer, or a small MGU_WINO_PPB_CAP, do
  // not: the caller then takes the separate statistics pass, launch_bn_stats)
  if (f.stat_slots && conv_is_wino(k) && wino_grid_blocks(d) <= STAT_ROWS) {
    d.stat_slots = f.stat_slots;
    t.stats = true, t.stat_rows = wino_grid_blocks(d);
  }
  if (f.pool && conv_fuses_pool(k)) {   // the Winograd / halo epilogue also writes the 2x2 max-pooled tensor
    d.pool = (float*)f.pool, d.ldpool = f.ldpool;
    t.pool = true;
  }
  if (d.stat_slots || d.pool) k = pick_conv(d, c->dtype, f.head);   // the fused epilogue narrows the choice (not every kernel form has it)
  t.head = conv_fuses_head(k);   // else the caller runs the head and the patch means in their own pass
  const WinoHead* head = t.head ? f.head : nullptr;
  if (took) *took = t;
  if (L.wp_dirty && conv_reads_panel(k)) {   // falling back to the direct kernel: build its panel now
    HIPCHK(c, launch_pack_one(L.convt ? pack_convt_panel(L.w_src, L.wp, c->dtype, L.Cin, L.Cout, L.Kp)
                                      : pack_conv_panel(L.w_src, L.wp, c->dtype, L.Cout, L.Cin, L.Cp, L.KS, L.Kp), s));
    L.wp_dirty = false;
    ++c->panel_packs;
  }
  // profiling record: algorithmic 2*MAC of the operator and what the matrix pipe really issues
  double alg = L.convt ? 2.0 * d.M * (double)L.Cin * L.Cout * 4.0 : 2.0 * d.M * (double)L.KS * L.KS * L.Cin * L.Cout;
  if (head) alg += 2.0 * d.M * (double)L.Cout * head->ncls;   // the 1x1 head's work rides in this launch
  const ConvCost cost = conv_cost(k, d);
  ProfScope ps(c, s, conv_kernel_name(k, d), alg, cost.mfma, cost.pipe);
  HIPCHK(c, launch_conv(d, k, c->dtype, s, head));
  c->convt_asm_launches += k == ConvKernel::ConvtX3Asm;
  return MGU_OK;
}

extern "C" {

int mgu_unet_forward(mgu_ctx* c, const void* x_dev, int B, int H, int W, int64_t xs_n, int64_t xs_c, int64_t xs_h,
                     int64_t xs_w, void* logits_dev, void* const* cat_dev, void* const* feat_dev, int training,
                     void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!c->configured || !c->loaded) return fail(c, MGU_ERR_STATE, "configure + load_weights must precede forward");
  if (!x_dev || !logits_dev || !cat_dev || !feat_dev) return fail(c, MGU_ERR_INVALID, "NULL buffer");
  const int depth = c->depth;
  if (B < 1 || H < (1 << depth) || W < (1 << depth))
    return fail(c, MGU_ERR_INVALID, "input %dx%dx%d too small for depth %d", B, H, W, depth);
  if ((int64_t)B * H * W >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "B*H*W must be < 2^31");
  for (int i = 0; i < depth; ++i)
    if (!cat_dev[i] || !feat_dev[i]) return fail(c, MGU_ERR_INVALID, "NULL cat/feat buffer %d", i);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  if (training && c->dtype != MGU_DTYPE_F32)
    return fail(c, MGU_ERR_STATE, "training runs in fp32 only (bf16 storage is an inference mode)");
  if (training) {  // batch-statistics BatchNorm, running-stat update, activations kept for mgu_unet_backward
    int rc = unet_forward_train(c, (const float*)x_dev, xs_n, xs_c, xs_h, xs_w, B, H, W, (float*)logits_dev, cat_dev, feat_dev, s);
    if (rc == MGU_OK && c->pm_out) {   // a pending patch-mean request is served by the stand-alone kernel
      ProfScope ps(c, s, "patch_mean_kernel", 0, 0, -1);
      HIPCHK(c, launch_patch_mean(feat_dev[0], 0, (float*)c->pm_out, B, H, W, c->feat, c->pm_patch, s));
      c->pm_out = nullptr;
    }
    return rc;
  }
  const WsPlan plan = plan_ws(c, B, H, W);
  int rc = ensure(c, &c->ws, &c->ws_bytes, plan.total);
  if (rc) return rc;
  // A pending patch-mean request at the graph's 16-pixel patch: the convolution that writes decoder feature 0 also applies the final
  // 1x1 conv and sums the graph patches in its finishing pass, if the pick admits it (wino_head_layer sizes the scratch, pick_conv
  // decides on the complete descriptor); the second pass over the 32-channel feature map and the head kernel then fall away
  const Layer& F = c->layers[c->head];
  WinoHead head_args{};
  bool head_done = false;
  const bool head_wanted = c->pm_out && F.w_src && F.b_src && wino_head_layer(c->tn, c->dtype, F.Cin, c->ncls, c->pm_patch, B, H, W);
  if (head_wanted) {
    if ((rc = ensure(c, &c->pmws, &c->pmws_bytes, wino_head_psum_bytes(B, H, W)))) return rc;
    head_args = WinoHead{F.w_src, F.b_src, (float*)logits_dev, (float*)c->pmws, c->ncls, (int)wino_head_psum_bytes(B, H, W)};
  }
  if (c->fold_dirty) {  // eval BatchNorm: y = scale * conv + shift with the CURRENT running statistics
    for (auto& L : c->layers)
      if (!L.bn.empty()) HIPCHK(c, launch_bn_fold(L.b_src, L.gamma, L.beta, L.run_mean, L.run_var, 1e-5f, L.scale, L.shift, L.Cout, s));
    c->fold_dirty = false;
  }
  char* ws = (char*)c->ws;
  const size_t es = c->dtype == MGU_DTYPE_BF16 ? 2 : 4;
  void* xin = ws + plan.xin;
  void* bott = ws + plan.bott;
  std::vector<int> hs, wsz;
  level_dims(H, W, depth, hs, wsz);

  if (c->prof) {
    for (auto& e : c->ev_total)
      if (!e) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(c->ev_total[0], s));
  }

  // odd sizes: F.pad (unet_decoder.py:46-47) leaves a zero row/column in the up-sampled half
  for (const Block& b : c->enc) {
    const int i = b.level;
    if (2 * hs[i + 1] != hs[i] || 2 * wsz[i + 1] != wsz[i])
      HIPCHK(c, hipMemsetAsync(cat_dev[i], 0, (size_t)B * hs[i] * wsz[i] * 2 * c->layers[b.conv2].Cout * es, s));
  }

  // the first convolution on the matrix cores reads the caller's image itself (first_mfma.hip): no packed copy of the input
  const Layer& L0 = c->layers[c->enc[0].conv1];
  const bool first_direct = L0.wfm && c->tn.first_mfma && first_mfma_applicable(c->dtype, L0.Cin, L0.Cp, L0.Cout, c->feat, 0, H, W) &&
                            (int64_t)B * H * W < (1ll << 31);
  if (!first_direct) HIPCHK(c, launch_pack_input((const float*)x_dev, xin, c->dtype, B, c->in_ch, c->Cp0, H, W, xs_n, xs_c, xs_h, xs_w, s));

  // One image group's walk of the network: images [img0, img0 + nb) on stream gs, the shared conv1 temporary in the group's own
  // slice `tmp` (images indexed locally).  Every other buffer is dedicated to its level and batch-major, so the group starts at its
  // first image; the head-fused launch gets the group's part of the logits and of the row-pair partial sums.
  auto walk = [&](hipStream_t gs, int img0, int nb, void* tmp, bool* head_done) -> int {
    auto at = [&](const void* base, int level, int ch) { return (char*)base + (size_t)img0 * hs[level] * wsz[level] * ch * es; };
    WinoHead head = head_args;
    if (head_wanted) {
      head.logits += (size_t)img0 * H * W * c->ncls;
      head.psum = (float*)((char*)head.psum + wino_head_psum_bytes(img0, H, W));
      head.psum_bytes = (int)wino_head_psum_bytes(nb, H, W);
    }
    // layer l on the group's images at grid level lvl, with its folded BatchNorm scale / shift
    auto conv = [&](int l, int lvl, ConvReq q, const ConvFusions& f = {}, ConvTaken* took = nullptr) {
      const Layer& L = c->layers[l];
      q.B = nb, q.H = hs[lvl], q.W = wsz[lvl], q.scale = L.bn.empty() ? nullptr : L.scale, q.shift = L.shift;
      return run_layer(c, L, q, gs, f, took);
    };
    const void* cur = at(xin, 0, c->Cp0);
    int cur_ld = c->Cp0;
    for (const Block& b : c->enc) {  // encoder, unet_encoder.py:67-70
      const int i = b.level, C = c->layers[b.conv1].Cout;
      if (&b == &c->enc.front() && first_direct) {
        if (c->fold_dirty) return fail(c, MGU_ERR_STATE, "internal: eval scale/shift not folded");
        const double alg = 2.0 * nb * H * W * 9.0 * L0.Cin * L0.Cout;
        ProfScope ps(c, gs, "conv3x3_first_mfma_kernel", alg, 2.0 * nb * H * W * 32.0 * 32.0 * (c->dtype == MGU_DTYPE_F32 ? 6.0 : 3.0), 1);
        HIPCHK(c, launch_first_mfma_direct(c->dtype, (const float*)x_dev + (int64_t)img0 * xs_n, xs_n, xs_c, xs_h, xs_w, c->in_ch, L0.wfm,
                                           L0.bn.empty() ? nullptr : L0.scale, L0.shift, tmp, nb, H, W, C, 0, 1, gs));
      } else if ((rc = conv(b.conv1, i, {.in = cur, .ldin = cur_ld, .out = tmp, .ldout = C, .relu = 1}))) return rc;
      void *cat = at(cat_dev[i], i, 2 * C), *pooled = at(ws + plan.pooled[i], i + 1, C);
      ConvTaken took;   // MaxPool2d(2) (unet_encoder.py:48) rides in the conv2 epilogue on the Winograd path
      if ((rc = conv(b.conv2, i, {.in = tmp, .ldin = C, .out = cat, .ldout = 2 * C, .relu = 1}, {.pool = pooled, .ldpool = C}, &took))) return rc;
      if (!took.pool) {   // (a pick without the fused epilogue: the tile kernels)
        ProfScope ps(c, gs, "maxpool2", 0, 0, -1);
        HIPCHK(c, launch_maxpool2(cat, 2 * C, pooled, c->dtype, nb, hs[i], wsz[i], C, gs));
      }
      cur = pooled, cur_ld = C;
    }
    {  // bottleneck, :72
      const Block& b = c->bott;
      const int i = b.level, C = c->layers[b.conv1].Cout;
      if ((rc = conv(b.conv1, i, {.in = cur, .ldin = cur_ld, .out = tmp, .ldout = C, .relu = 1}))) return rc;
      if ((rc = conv(b.conv2, i, {.in = tmp, .ldin = C, .out = at(bott, i, C), .ldout = C, .relu = 1}))) return rc;
      cur = at(bott, i, C), cur_ld = C;
    }
    for (const Block& b : c->dec) {  // decoder, unet_decoder.py:139-141
      const int i = b.level, C = c->layers[b.conv1].Cout;
      const bool last = head_wanted && i == 0;
      // ConvTranspose2d(k2,s2) -> pixel-shuffle store into channels [C, 2C) of the concat buffer (:36,:53)
      void *cat = at(cat_dev[i], i, 2 * C), *feat = at(feat_dev[i], i, C);
      if ((rc = conv(b.up, i + 1, {.in = cur, .ldin = cur_ld, .out = cat, .ldout = 2 * C, .coff = C, .Hout = hs[i], .Wout = wsz[i]}))) return rc;
      if ((rc = conv(b.conv1, i, {.in = cat, .ldin = 2 * C, .out = tmp, .ldout = C, .relu = 1}))) return rc;
      ConvTaken took;
      if ((rc = conv(b.conv2, i, {.in = tmp, .ldin = C, .out = feat, .ldout = C, .relu = 1}, {.head = last ? &head : nullptr}, &took))) return rc;
      if (last) *head_done = took.head;
      cur = feat, cur_ld = C;
    }
    return MGU_OK;
  };
  // Two image groups (Tuning::fwd_groups): group 0 on the caller's stream, group 1 on the side stream between a fork and a join event,
  // so that everything before and after this call on the caller's stream stays ordered against both.  With profiling on the batch
  // walks as one group: event pairs around overlapped launches would charge a kernel for the time it waits for CUs.
  const int G = c->prof ? 1 : fwd_groups(c, B);
  if (G == 1) {
    if ((rc = walk(s, 0, B, ws + plan.tmp, &head_done))) return rc;
  } else {
    if (!c->fwd_stream) HIPCHK(c, hipStreamCreateWithFlags(&c->fwd_stream, hipStreamNonBlocking));
    for (auto& e : c->fwd_ev)
      if (!e) HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    const int n0 = group_images(c, B), packs = c->panel_packs;
    bool done1 = false;
    HIPCHK(c, hipEventRecord(c->fwd_ev[0], s));
    HIPCHK(c, hipStreamWaitEvent(c->fwd_stream, c->fwd_ev[0], 0));
    rc = walk(s, 0, n0, ws + plan.tmp, &head_done);
    if (rc == MGU_OK && c->panel_packs != packs) {   // group 0 built a direct panel on first use: group 1 reads it too
      HIPCHK(c, hipEventRecord(c->fwd_ev[0], s));
      HIPCHK(c, hipStreamWaitEvent(c->fwd_stream, c->fwd_ev[0], 0));
    }
    const int rc1 = rc == MGU_OK ? walk(c->fwd_stream, n0, B - n0, ws + plan.tmp + plan.tmp_slice, &done1) : MGU_OK;
    HIPCHK(c, hipEventRecord(c->fwd_ev[1], c->fwd_stream));   // the join also closes a walk that failed half-way
    HIPCHK(c, hipStreamWaitEvent(s, c->fwd_ev[1], 0));
    if (rc || rc1) return rc ? rc : rc1;
    if (done1 != head_done) return fail(c, MGU_ERR_STATE, "internal: the image groups disagree on the head-fused kernel");
  }
  const void* cur = feat_dev[0];
  const int cur_ld = c->layers[c->dec.back().conv1].Cout;
  // final 1x1 conv (:143): a few output channels -> HBM-bound head kernel reading the reference's (ncls, C) weight
  {
    const int pm_dtype = c->dtype;   // decoder features are stored in the compute dtype
    if (head_done) {   // logits are written; the patch means are the fixed-order sum of the eight row-pair partials of every node
      ProfScope ps(c, s, "patch_sum_combine_kernel", 0, 0, -1);
      HIPCHK(c, launch_patch_sum_combine((const float*)c->pmws, (float*)c->pm_out, B * (H / 16) * (W / 16), s));
      c->pm_out = nullptr;
    } else if (c->pm_out && F.w_src && F.b_src && patch_mean_head_fusable(pm_dtype, F.Cin, c->ncls) && F.Cin <= 256) {
      // requested patch means + the 1x1 head in ONE pass over the decoder feature (both are pure bandwidth)
      ProfScope ps(c, s, "patch_mean_kernel (1x1 head + patch means)", 2.0 * B * H * W * F.Cin * c->ncls, 0, -1);
      HIPCHK(c, launch_patch_mean(cur, pm_dtype, (float*)c->pm_out, B, H, W, F.Cin, c->pm_patch, s, F.w_src, F.b_src,
                                  (float*)logits_dev, c->ncls));
      c->pm_out = nullptr;
    } else if (c->ncls <= 4 && F.w_src && F.b_src) {
      ProfScope ps(c, s, "conv1x1_head_kernel", 2.0 * B * H * W * F.Cin * c->ncls, 0, -1);
      HIPCHK(c, launch_conv1x1_head(cur, c->dtype, cur_ld, F.Cin, F.w_src, F.b_src, (float*)logits_dev, c->ncls, c->ncls,
                                    (int64_t)B * H * W, s));   // logits are always fp32
    } else if ((rc = run_layer(c, F, {.in = cur, .ldin = cur_ld, .B = B, .H = H, .W = W, .out = logits_dev, .ldout = c->ncls, .shift = F.shift}, s))) {
      return rc;
    }
  }
  if (c->pm_out) {   // request not served by the fused pass (head shape): separate kernel, same result
    ProfScope ps(c, s, "patch_mean_kernel", 0, 0, -1);
    HIPCHK(c, launch_patch_mean(cur, c->dtype, (float*)c->pm_out, B, H, W, F.Cin, c->pm_patch, s));
    c->pm_out = nullptr;
  }
  if (c->prof) HIPCHK(c, hipEventRecord(c->ev_total[1], s));
  return MGU_OK;
}

int mgu_unet_request_patch_mean(mgu_ctx* c, int patch, void* out_dev) {
  if (!c) return MGU_ERR_INVALID;
  if (!c->configured) return fail(c, MGU_ERR_STATE, "not configured");
  if (!out_dev) {   // cancel a pending request
    c->pm_out = nullptr;
    return MGU_OK;
  }
  if (patch < 1) return fail(c, MGU_ERR_INVALID, "bad patch_mean request");
  const int C = c->layers[c->head].Cin, vec = c->dtype == MGU_DTYPE_BF16 ? 8 : 4;
  if ((C % vec) || C > 256) return fail(c, MGU_ERR_INVALID, "patch means need init_features %% %d == 0 and <= 256 (got %d)", vec, C);
  c->pm_patch = patch;
  c->pm_out = out_dev;
  return MGU_OK;
}

// Packed forms of one Conv2d weight (direct panel and, for fp32 3x3 layers with Cin % 16 == 0, the Winograd U), owned by the
// library: built once by mgu_conv2d_prepare and reused by every mgu_conv2d_prepared_nhwc call until the weight changes.
struct mgu_conv_weights {
  Layer L;   // shape; L.wp, L.shift, L.wu in one allocation: [panel | bias-as-shift | U]
};

// the Conv2d launch of both building blocks on the packed forms of L (L.shift: room for the bias)
static int conv2d_launch(mgu_ctx* c, const Layer& L, const void* in_dev, int B, int H, int W, const void* bias_dev, const void* scale_dev,
                         const void* shift_dev, int relu, void* out_dev, int ld_out, int c_off, hipStream_t s) {
  IgemmDesc d = layer_desc(c, L, in_dev, L.Cin, B, H, W, out_dev, ld_out, c_off);
  d.relu = relu;
  if (scale_dev && shift_dev) {  // y = scale*(conv) + shift, bias folded by the caller into shift
    d.scale = (const float*)scale_dev;
    d.shift = (const float*)shift_dev;
  } else if (bias_dev) {
    HIPCHK(c, launch_pack_one(pack_bias_tile((const float*)bias_dev, L.shift, L.Cout, 1), s));
    d.shift = L.shift;
  }
  const ConvKernel k = pick_conv(d, 0);
  ProfScope ps(c, s, conv_kernel_name(k, d));   // the record names the kernel the pick chose, as run_layer's does
  HIPCHK(c, launch_conv(d, k, 0, s));
  return MGU_OK;
}

int mgu_conv2d_prepare(mgu_ctx* c, const void* w_dev, int Cout, int Cin, int ksize, mgu_conv_weights** out, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!w_dev || !out || Cout < 1 || (ksize != 1 && ksize != 3)) return fail(c, MGU_ERR_INVALID, "bad conv2d_prepare args (ksize must be 1 or 3)");
  if (Cin < 4 || (Cin & 3)) return fail(c, MGU_ERR_INVALID, "conv2d needs Cin %% 4 == 0 (got %d)", Cin);
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  mgu_conv_weights* p = new mgu_conv_weights();
  Layer& L = p->L;
  L = make_layer(MGU_DTYPE_F32, Cin, Cin, Cout, ksize, false);   // the building blocks run in fp32 on Cin % 4 == 0 channels
  const bool wino = wino_layer(c->tn, ksize, Cin);
  const size_t panel = (size_t)L.Np * L.Kp, total = panel + L.Np + (wino ? wino_u_floats(Cout, Cin) : 0);
  hipError_t e = hipMalloc((void**)&L.wp, total * sizeof(float));
  if (e != hipSuccess) {
    delete p;
    return fail(c, MGU_ERR_NOMEM, "hipMalloc(%zu) failed: %s", total * sizeof(float), hipGetErrorString(e));
  }
  L.shift = L.wp + panel;
  e = hipMemsetAsync(L.wp, 0, (panel + L.Np) * sizeof(float), s);
  if (e == hipSuccess) e = launch_pack_one(pack_conv_panel((const float*)w_dev, L.wp, 0, Cout, Cin, Cin, ksize, L.Kp), s);
  if (e == hipSuccess && wino) {
    L.wu = L.shift + L.Np;
    e = launch_pack_one(pack_wino((const float*)w_dev, L.wu, Cout, Cin, Cin, 0, c->tn.wino_prec), s);
  }
  if (e != hipSuccess) {
    (void)hipFree(L.wp);
    delete p;
    return fail(c, MGU_ERR_HIP, "conv2d_prepare: %s", hipGetErrorString(e));
  }
  *out = p;
  return MGU_OK;
}

void mgu_conv2d_release(mgu_ctx* c, mgu_conv_weights* p) {
  if (!p) return;
  if (c) (void)hipSetDevice(c->device);
  (void)hipDeviceSynchronize();   // launches that read the panels may still be in flight
  if (p->L.wp) (void)hipFree(p->L.wp);
  delete p;
}

int mgu_conv2d_prepared_nhwc(mgu_ctx* c, const mgu_conv_weights* p, const void* in_dev, int B, int H, int W, const void* bias_dev,
                             const void* scale_dev, const void* shift_dev, int relu, void* out_dev, int ld_out, int c_off,
                             void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!p || !in_dev || !out_dev || B < 1 || H < 1 || W < 1) return fail(c, MGU_ERR_INVALID, "bad conv2d args");
  if (ld_out < c_off + p->L.Cout) return fail(c, MGU_ERR_INVALID, "ld_out %d < c_off %d + Cout %d", ld_out, c_off, p->L.Cout);
  if ((int64_t)B * H * W >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  return conv2d_launch(c, p->L, in_dev, B, H, W, bias_dev, scale_dev, shift_dev, relu, out_dev, ld_out, c_off, (hipStream_t)hip_stream);
}

// One-shot form: packs the weight on EVERY call (parity tests, weights that change between calls) into the context's scratch, then
// the mgu_conv2d_prepared_nhwc launch; steady-state callers use mgu_conv2d_prepare + mgu_conv2d_prepared_nhwc.
int mgu_conv2d_nhwc(mgu_ctx* c, const void* in_dev, int B, int H, int W, int Cin, const void* w_dev, const void* bias_dev,
                    const void* scale_dev, const void* shift_dev, int Cout, int ksize, int relu, void* out_dev,
                    int ld_out, int c_off, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !w_dev || !out_dev || B < 1 || H < 1 || W < 1 || Cout < 1 || (ksize != 1 && ksize != 3))
    return fail(c, MGU_ERR_INVALID, "bad conv2d args (ksize must be 1 or 3)");
  if (Cin < 4 || (Cin & 3)) return fail(c, MGU_ERR_INVALID, "conv2d needs Cin %% 4 == 0 (got %d)", Cin);
  if (ld_out < c_off + Cout) return fail(c, MGU_ERR_INVALID, "ld_out %d < c_off %d + Cout %d", ld_out, c_off, Cout);
  if ((int64_t)B * H * W >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Layer L = make_layer(MGU_DTYPE_F32, Cin, Cin, Cout, ksize, false);
  const size_t need = ((size_t)L.Np * L.Kp + 2 * (size_t)L.Np) * sizeof(float);   // panel + scale/shift
  int rc = ensure(c, &c->gws, &c->gws_bytes, need);
  if (rc) return rc;
  L.wp = (float*)c->gws;
  L.shift = L.wp + (size_t)L.Np * L.Kp + L.Np;
  HIPCHK(c, hipMemsetAsync(c->gws, 0, need, s));
  HIPCHK(c, launch_pack_one(pack_conv_panel((const float*)w_dev, L.wp, 0, Cout, Cin, Cin, ksize, L.Kp), s));
  if (wino_layer(c->tn, ksize, Cin)) {   // same routing as the model's layers: Winograd F(2x2,3x3)
    if ((rc = ensure(c, &c->wuws, &c->wuws_bytes, wino_u_floats(Cout, Cin) * sizeof(float)))) return rc;
    L.wu = (float*)c->wuws;
    HIPCHK(c, launch_pack_one(pack_wino((const float*)w_dev, L.wu, Cout, Cin, Cin, 0, c->tn.wino_prec), s));
  }
  return conv2d_launch(c, L, in_dev, B, H, W, bias_dev, scale_dev, shift_dev, relu, out_dev, ld_out, c_off, s);
}

int mgu_conv_transpose2x2_nhwc(mgu_ctx* c, const void* in_dev, int B, int H, int W, int Cin, const void* w_dev,
                               const void* bias_dev, int Cout, void* out_dev, int ld_out, int c_off, void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !w_dev || !out_dev || B < 1 || H < 1 || W < 1 || Cout < 1) return fail(c, MGU_ERR_INVALID, "bad convT args");
  if (Cin < 4 || (Cin & 3)) return fail(c, MGU_ERR_INVALID, "convT needs Cin %% 4 == 0 (got %d)", Cin);
  if (ld_out < c_off + Cout) return fail(c, MGU_ERR_INVALID, "ld_out %d < c_off %d + Cout %d", ld_out, c_off, Cout);
  if ((int64_t)B * H * W * 4 >= (1ll << 31)) return fail(c, MGU_ERR_INVALID, "4*B*H*W must be < 2^31");
  HIPCHK(c, hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)hip_stream;
  Layer U = make_layer(MGU_DTYPE_F32, Cin, Cin, Cout, 1, true);
  // Two packed forms, each in a region of its own: the direct [4 Cout][Cin] panel the tile kernel reads (always built), and -- when
  // the layer shape is eligible and the context's switches allow it (MGU_NO_CONVT_FRAG, MGU_WINO_PREC) -- the fragment-order
  // three-piece weights of convt2x2_x3_kernel.  Which kernel runs is decided by pick_conv on the COMPLETE descriptor; a launch it
  // sends to the tile kernel finds a real panel in d.w.
  const bool x3_shape = convt_x3_layer(c->tn, Cin, Cout);
  const size_t panel = (size_t)U.Np * U.Kp + 2 * (size_t)U.Np;   // panel + scale/shift
  int rc = ensure(c, &c->gws, &c->gws_bytes, (panel + (x3_shape ? convt_x3_floats(Cin, Cout) : 0)) * sizeof(float));
  if (rc) return rc;
  U.wp = (float*)c->gws;
  U.shift = U.wp + (size_t)U.Np * U.Kp + U.Np;
  U.wu = x3_shape ? U.wp + panel : nullptr;
  HIPCHK(c, hipMemsetAsync(c->gws, 0, panel * sizeof(float), s));
  HIPCHK(c, launch_pack_one(pack_convt_panel((const float*)w_dev, U.wp, 0, Cin, Cout, U.Kp), s));
  IgemmDesc d = layer_desc(c, U, in_dev, Cin, B, H, W, out_dev, ld_out, c_off);
  d.Hout = 2 * H, d.Wout = 2 * W;
  if (bias_dev) {
    HIPCHK(c, launch_pack_one(pack_bias_tile((const float*)bias_dev, U.shift, Cout, 4), s));
    d.shift = U.shift;
  }
  const ConvKernel k = pick_conv(d, 0);
  if (conv_reads_convt_x3(k)) HIPCHK(c, launch_pack_one(pack_convt_x3((const float*)w_dev, U.wu, Cin, Cout, 0), s));
  ProfScope ps(c, s, conv_kernel_name(k, d));
  HIPCHK(c, launch_conv(d, k, 0, s));
  c->convt_asm_launches += k == ConvKernel::ConvtX3Asm;
  return MGU_OK;
}

int mgu_maxpool2x2_nhwc(mgu_ctx* c, const void* in_dev, int ld_in, int B, int H, int W, int Cc, void* out_dev,
                        void* hip_stream) {
  if (!c) return MGU_ERR_INVALID;
  if (!in_dev || !out_dev || B < 1 || H < 2 || W < 2 || Cc < 4 || (Cc & 3) || ld_in < Cc || (ld_in & 3))
    return fail(c, MGU_ERR_INVALID, "bad maxpool args (C and ld_in must be multiples of 4, H,W >= 2)");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_maxpool2(in_dev, ld_in, out_dev, 0, B, H, W, Cc, (hipStream_t)hip_stream));
  return MGU_OK;
}

int mgu_argmax_classes(mgu_ctx* c, const void* logits_dev, int64_t npix, int num_classes, int64_t* pred_dev,
                       void* hip_stream) {
  if (!c || !logits_dev || !pred_dev || num_classes < 1 || npix < 0) return fail(c, MGU_ERR_INVALID, "bad argmax args");
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_argmax((const float*)logits_dev, npix, num_classes, pred_dev, (hipStream_t)hip_stream));
  return MGU_OK;
}

int mgu_patch_mean(mgu_ctx* c, const void* feat_dev, int feat_dtype, int B, int H, int W, int C, int patch, void* out_dev,
                   void* hip_stream) {
  if (!c || !feat_dev || !out_dev || B < 1 || H < 1 || W < 1 || patch < 1)
    return fail(c, MGU_ERR_INVALID, "bad patch_mean args");
  if (feat_dtype != MGU_DTYPE_F32 && feat_dtype != MGU_DTYPE_BF16) return fail(c, MGU_ERR_INVALID, "unknown dtype %d", feat_dtype);
  const int vec = feat_dtype == MGU_DTYPE_BF16 ? 8 : 4;
  if ((C % vec) || C < vec || C > 256)
    return fail(c, MGU_ERR_INVALID, "patch_mean needs C %% %d == 0 and C <= 256 (got %d)", vec, C);
  HIPCHK(c, hipSetDevice(c->device));
  HIPCHK(c, launch_patch_mean(feat_dev, feat_dtype, (float*)out_dev, B, H, W, C, patch, (hipStream_t)hip_stream));
  return MGU_OK;
}

// FLOPs of the network on a B x H x W input: every layer at its level.  mfma: what the matrix pipe issues, the Winograd layers'
// 16 products per 2x2 tile instead of 36.  Every term is an integer far below 2^53: the sums are exact.
static double net_flops(const mgu_ctx* c, int B, int H, int W, bool mfma) {
  std::vector<int> hs, wsz;
  level_dims(H, W, c->depth, hs, wsz);
  double fl = 0;
  for (const Layer& L : c->layers) {
    const int h = hs[L.level], w = wsz[L.level];
    if (mfma && L.wino) fl += 2.0 * ((h + 1) / 2) * ((w + 1) / 2) * 16.0 * L.Cp * L.Cout;   // per 2x2 tile: 16 products
    else fl += 2.0 * h * w * L.KS * L.KS * L.Cin * L.Cout * (L.convt ? 4.0 : 1.0);
  }
  return fl * B;
}

double mgu_unet_flops(mgu_ctx* c, int B, int H, int W) { return c && c->configured ? net_flops(c, B, H, W, false) : -1.0; }

double mgu_unet_mfma_flops(mgu_ctx* c, int B, int H, int W) { return c && c->configured ? net_flops(c, B, H, W, true) : -1.0; }

int mgu_profile_enable(mgu_ctx* c, int on) {
  if (!c) return MGU_ERR_INVALID;
  c->prof = on != 0;
  c->ev_used = 0;
  return MGU_OK;
}

int mgu_profile_read_kernels(mgu_ctx* c, mgu_kernel_stat* out, int cap, int* n_out) {
  if (!c || !n_out || (cap > 0 && !out)) return MGU_ERR_INVALID;
  int n = 0;
  for (int i = 0; i < c->ev_used; ++i) {
    float ms = 0;
    HIPCHK(c, hipEventSynchronize(c->ev[2 * i + 1]));
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]));
    const mgu_ctx::ProfRec& r = c->prec[i];
    int k = 0;
    while (k < n && strcmp(out[k].name, r.name) != 0) ++k;
    if (k == n) {
      if (n == cap) continue;   // table full: the remaining families are dropped (cap >= 32 holds every family of a step)
      out[n].name = r.name, out[n].ms = 0, out[n].flops_alg = 0, out[n].flops_mfma = 0, out[n].launches = 0, out[n].pipe = r.pipe;
      ++n;
    }
    out[k].ms += ms, out[k].flops_alg += r.alg, out[k].flops_mfma += r.mfma, out[k].launches += 1;
  }
  *n_out = n;
  c->ev_used = 0;   // a read consumes the records: with profiling left on, the next window starts from an empty table
  return MGU_OK;
}

int64_t mgu_convt_asm_launches(mgu_ctx* c) { return c ? c->convt_asm_launches : 0; }

int mgu_profile_read(mgu_ctx* c, double* conv_ms, int* conv_launches, double* total_ms) {
  if (!c) return MGU_ERR_INVALID;
  if (c->ev_used == 0 || !c->ev_total[1]) return fail(c, MGU_ERR_STATE, "no profiled forward to read");
  HIPCHK(c, hipEventSynchronize(c->ev_total[1]));
  double sum = 0;
  for (int i = 0; i < c->ev_used; ++i) {
    float ms = 0;
    HIPCHK(c, hipEventSynchronize(c->ev[2 * i + 1]));
    HIPCHK(c, hipEventElapsedTime(&ms, c->ev[2 * i], c->ev[2 * i + 1]));
    sum += ms;
  }
  float tot = 0;
  HIPCHK(c, hipEventElapsedTime(&tot, c->ev_total[0], c->ev_total[1]));
  if (conv_ms) *conv_ms = sum;
  if (conv_launches) *conv_launches = c->ev_used;
  if (total_ms) *total_ms = tot;
  return MGU_OK;
}

}  // extern "C"
