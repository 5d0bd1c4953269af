// Internal: context and helpers shared by mgunet_api.hip and mgunet_train.hip (not part of the ABI).
#pragma once
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/mgunet.h"
#include "common.h"

struct Layer {
  std::string prefix;   // state_dict prefix, e.g. "encoder.encoder_blocks.0."
  std::string conv;     // "conv1" | "conv2" | "upsample" | "final_conv"
  std::string bn;       // "bn1" | "bn2" | ""
  int Cin = 0, Cp = 0, Cout = 0, KS = 3;
  bool convt = false;
  int K = 0, Kp = 0, N = 0, Np = 0;
  float *wp = nullptr, *scale = nullptr, *shift = nullptr;
  bool first = false;    // fp32 first convolution (<= 4 input channels): VALU kernel, weights kept in wf
  bool ctb = false;      // bf16-storage ConvTranspose for convt2x2_bf16_kernel (convt_bf16f_layer): bf16 fragment weights kept in wu
  bool ctx3 = false;     // fp32 ConvTranspose for convt2x2_x3_kernel (convt_x3_layer): three-piece fragment weights kept in wu
  bool wino = false;     // fp32 3x3 layer for the Winograd kernels (wino_layer): Winograd-transformed weights kept in wu
  mutable bool wp_dirty = false;   // direct panel wp not yet rebuilt from w_src (packed on first use)
  float* wu = nullptr;
  float* wug = nullptr;          // Winograd weights of the layer's DATA-GRADIENT convolution (training; same launch as wu)
  mutable bool wug_valid = false;   // wug holds the current weights
  float* wf = nullptr;   // first conv (Cp == 4): [9][4][Cout] weights for conv3x3_first_kernel
  float* wfm = nullptr;  // the same layer's three-piece fragment weights for conv3x3_first_mfma_kernel (Cin <= 3, Cout == 32)
  float* wxg = nullptr;  // data-gradient weights kept across the step (training; packed with everything else by the weight refresh):
                         // three-piece fragments of a ConvTranspose (convt_x3.hip) or the direct panel of the final 1x1 conv
  mutable bool wxg_valid = false;
  // caller-owned parameter tensors recorded by load_weights (used by the training path)
  const float *w_src = nullptr, *b_src = nullptr, *gamma = nullptr, *beta = nullptr;
  float *run_mean = nullptr, *run_var = nullptr;
  // offsets (elements) into the flat parameter / gradient vector, named_parameters() order
  int64_t off_w = 0, off_b = 0, off_gamma = 0, off_beta = 0;
  // batch statistics of the last training forward (library scratch)
  float *mean = nullptr, *invstd = nullptr, *tscale = nullptr, *tshift = nullptr;
  int level = 0;                  // grid level the layer runs on (input grid for convT): H >> level after `level` MaxPool2d(2)
};

// What a layer's backward reads of its training forward (mgu_ctx::fwd: the model's; bwd_blocks.hip builds one of the caller's tensors)
struct FwdRecord {
  const float* in = nullptr;  // conv input
  int ldin = 0;
  float* z = nullptr;         // raw conv output (dense, pitch Cout)
  float* y = nullptr;         // relu(bn(z)) with pitch ldy
  int ldy = 0;
  int B = 0, H = 0, W = 0;    // grid the conv ran on (input grid for convT)
};

// One ConvBlock of the network (unet_encoder.py:4-25) and, in a decoder block, the ConvTranspose2d in front of it: indices into
// mgu_ctx::layers.  Every walk over the network (parameter offsets, workspace plans, forwards, backward, FLOP counts) reads these.
struct Block {
  int up = -1;            // decoder: ConvTranspose2d (unet_decoder.py:36); -1 elsewhere
  int conv1 = 0, conv2 = 0;
  int level = 0;          // grid level of conv1 / conv2: also the skip connection's (cat_dev / feat_dev index)
};

struct mgu_ctx {
  int device = 0;
  mgu::Tuning tn;           // kernel-selection switches of THIS context (MGU_* environment at mgu_create)
  std::string err;
  bool configured = false, loaded = false;
  std::vector<mgu::PackBatch> pack_host;   // the pack tables as last uploaded (repack_weights)
  mgu::PackBatch* pack_dev = nullptr;
  int pack_dev_cap = 0;
  bool want_train = false;  // a training forward has run on this context: weight refreshes also build the data-gradient forms
  bool fold_dirty = false;  // BN running stats / affine changed since the eval scale/shift were folded
  int* err_word = nullptr;  // host-mapped word a kernel sets when it meets invalid DATA (e.g. a label out of range): read by
                            // mgu_sync_check and, without a sync, at the entry of the next training call
  void* redws = nullptr;    // per-channel reduction slots (self-cleaning: zero between launches)
  size_t redws_bytes = 0;
  void* pm_out = nullptr;   // one-shot request (mgu_unet_request_patch_mean): patch means of decoder feature 0
  int pm_patch = 0;
  void* pmws = nullptr;     // row-pair partial sums of the head-fused convolution (WinoHead::psum)
  size_t pmws_bytes = 0;
  void* wuws = nullptr;     // Winograd weight scratch of the mgu_conv2d_nhwc building block
  size_t wuws_bytes = 0;
  unsigned long long* gmaxbuf = nullptr;   // GAT: [64 slots][gmax_cap] per-(graph, head) max accumulators, (generation, value) words
  int gmax_cap = 0;
  unsigned gmax_gen = 0;                   // generation of the last layer call (gat_common.h)
  struct mgu_gat_weights* gat_tmp = nullptr;   // weights prepared by the one-shot mgu_gat_layer_forward
  void* lossws = nullptr;   // partial records of the auxiliary-loss reductions (losses.hip)
  size_t lossws_bytes = 0;
  void* optws = nullptr;    // per-workgroup partial sums and non-finite counts of the gradient norm (optim.hip): one fixed size
  size_t optws_bytes = 0;
  void* imgws = nullptr;    // resampling coefficient tables / histograms of the input pipeline (imageops.hip)
  size_t imgws_bytes = 0;
  void* ncws = nullptr;     // normalized-cut accumulators (mgu_ncut_forward)
  size_t ncws_bytes = 0;
  void* objws = nullptr;    // connected-component parents, areas, chunk counts and matching flags (objects.hip); the distance
                            // transform's column distances and the seed buckets and first-pixel tables of the split (split.hip);
                            // the pair hash table, row degrees and unsorted pairs of the overlap table (instances.hip); the uint8
                            // class maps between the stages, the background labels and the per-hole counters of clean.hip; the
                            // class planes, their distance transform and the site column distances of boundary.hip; the 16-bit
                            // plane sets between the iterations of refine.hip
  size_t objws_bytes = 0;
  void* labtab = nullptr;            // device copy of the fixed-point CIELAB tables (superpixels.hip) and the host bytes it was made from:
  std::vector<unsigned char> labtab_host;   // refreshed when a call brings other contents
  int in_ch = 0, ncls = 0, feat = 0, depth = 0, dtype = 0, Cp0 = 0;
  std::vector<Layer> layers;  // enc[i].conv1, enc[i].conv2 ..., bott.conv1, bott.conv2, dec[b].up, dec[b].conv1, dec[b].conv2 ..., final
  std::vector<Block> enc, dec;   // encoder blocks shallow -> deep (level i), decoder blocks deep -> shallow (level depth-1-b)
  Block bott;                    // bottleneck (level depth)
  int head = 0;                  // the final 1x1 conv
  int64_t nparams = 0;
  float* arena = nullptr;
  size_t arena_floats = 0;
  void* ws = nullptr;   // eval scratch
  size_t ws_bytes = 0;
  void* gbws = nullptr;     // GAT train forward / backward scratch (gat_bwd.hip)
  size_t gbws_bytes = 0;
  void* gws = nullptr;  // GAT / building-block scratch
  size_t gws_bytes = 0;
  void* tws = nullptr;  // training scratch (saved activations + backward temporaries)
  size_t tws_bytes = 0;
  // last training forward
  bool have_train_fwd = false;
  int tB = 0, tH = 0, tW = 0;
  std::vector<FwdRecord> fwd;   // one per layer
  // gradient exchange (comm.hip): RCCL communicator owned by this context, its stream and a small pool of ordering events
  void* comm = nullptr;     // ncclComm_t
  int comm_world = 1, comm_rank = 0;
  hipStream_t comm_stream = nullptr;
  hipEvent_t comm_ev[16] = {};
  int comm_ev_next = 0;
  // profiling: HIP event pairs on the launch stream around the launches recorded since mgu_profile_enable(ctx, 1)
  bool prof = false;
  std::vector<hipEvent_t> ev;  // pairs
  struct ProfRec {
    const char* name;     // kernel (family) name, static storage
    double alg, mfma;     // algorithmic FLOPs (2*MAC of the operator) / FLOPs issued on the matrix pipe
    int pipe;             // matrix pipe: 0 = fp32 MFMA, 1 = bf16 MFMA, -1 = none (VALU / bandwidth kernels)
  };
  std::vector<ProfRec> prec;
  int ev_used = 0;
  hipEvent_t ev_total[2] = {nullptr, nullptr};
  // grouped eval forward (Tuning::fwd_groups): the second image group's stream and the fork / join events that order it against the
  // caller's stream; created on first use
  hipStream_t fwd_stream = nullptr;
  hipEvent_t fwd_ev[2] = {nullptr, nullptr};
  int64_t convt_asm_launches = 0;   // ConvTranspose launches on mgu_convt_x3_gfx950 so far (mgu_convt_asm_launches)
  int panel_packs = 0;   // direct panels run_layer has packed on first use so far (a grouped forward orders its second group after one)
};

namespace mgud {

inline int rup(int v, int m) { return (v + m - 1) / m * m; }
extern std::string g_create_err;

// The shape of a Conv2d (KS 1 / 3) or ConvTranspose2d(2, 2) (convt, KS 1) layer on Cin channels stored as Cp: GEMM depth K and
// width N with their panel paddings (Kp: one 128-byte LDS row of k per pipeline step)
inline Layer make_layer(int dtype, int Cin, int Cp, int Cout, int KS, bool convt) {
  Layer L;
  L.Cin = Cin, L.Cp = Cp, L.Cout = Cout, L.KS = KS, L.convt = convt;
  L.K = KS * KS * Cp, L.Kp = rup(L.K, dtype == MGU_DTYPE_BF16 ? 64 : 32);
  L.N = convt ? 4 * Cout : Cout, L.Np = rup(L.N, 128);
  return L;
}

inline int fail(mgu_ctx* c, int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  if (c) c->err = buf; else g_create_err = buf;
  return code;
}

#define HIPCHK(c, call)                                                                                       \
  do {                                                                                                        \
    hipError_t e_ = (call);                                                                                   \
    if (e_ != hipSuccess) return mgud::fail(c, MGU_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_));   \
  } while (0)

inline int ensure(mgu_ctx* c, void** p, size_t* have, size_t need) {
  if (*have >= need) return MGU_OK;
  if (*p) {
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipFree(*p));
    *p = nullptr;
    *have = 0;
  }
  hipError_t e = hipMalloc(p, need);
  if (e != hipSuccess) return fail(c, MGU_ERR_NOMEM, "hipMalloc(%zu) failed: %s", need, hipGetErrorString(e));
  *have = need;
  return MGU_OK;
}

// device pointer of the context's host-mapped data-error word (allocated on first use).  Bits: 1 = a label outside [0, num_classes)
// reached a loss kernel; 2 = the GAT backward found no edge equal to the forward's graph-wide maximum (gat_bwd.hip)
inline int err_word_dev(mgu_ctx* c, int** dev) {
  if (!c->err_word) {
    HIPCHK(c, hipHostMalloc((void**)&c->err_word, sizeof(int), hipHostMallocMapped));
    *c->err_word = 0;
  }
  HIPCHK(c, hipHostGetDevicePointer((void**)dev, c->err_word, 0));
  return MGU_OK;
}
// message of a pending data error (word value w)
inline const char* err_word_message(int w) {
  return (w & 2) ? "the GAT backward found no edge whose score equals the forward's graph-wide maximum (mgu_gat_layer_backward): its "
                   "max term was not applied"
                 : "a label outside [0, num_classes) (and != ignore_index -100) reached a loss kernel of this context (mgu_cross_entropy / "
                   "mgu_dice_loss; F.one_hot / CrossEntropyLoss raise on it)";
}

// 256-byte aligned regions of one scratch buffer: take(bytes) returns the next region's offset, off is the size so far
struct Carve {
  size_t off = 0;
  size_t take(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) / 256 * 256;
    return o;
  }
};

struct ProfScope {  // records an event pair around one launch when profiling is on (c == nullptr: the caller records nothing)
  mgu_ctx* c;
  hipStream_t s;
  int idx = -1;
  ProfScope(mgu_ctx* c_, hipStream_t s_, const char* name = "conv/GEMM", double alg = 0, double mfma = 0, int pipe = -1) : c(c_), s(s_) {
    if (!c || !c->prof) return;
    if ((size_t)c->ev_used >= c->prec.size()) c->prec.resize(c->ev_used + 1);
    c->prec[c->ev_used] = {name, alg, mfma, pipe};
    if ((size_t)(2 * c->ev_used + 2) > c->ev.size()) {
      hipEvent_t a, b;
      if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return;
      c->ev.push_back(a);
      c->ev.push_back(b);
    }
    idx = c->ev_used++;
    (void)hipEventRecord(c->ev[2 * idx], s);
  }
  ~ProfScope() {
    if (idx >= 0) (void)hipEventRecord(c->ev[2 * idx + 1], s);
  }
};

inline void level_dims(int H, int W, int depth, std::vector<int>& hs, std::vector<int>& wsz) {
  hs.assign(depth + 1, 0);
  wsz.assign(depth + 1, 0);
  hs[0] = H;
  wsz[0] = W;
  for (int i = 1; i <= depth; ++i) {
    hs[i] = hs[i - 1] / 2;  // MaxPool2d(2,2) floor mode, unet_encoder.py:48
    wsz[i] = wsz[i - 1] / 2;
  }
}

// Descriptors of the three shapes the host code launches.  A forward Conv2d (KS 1 / 3) or ConvTranspose2d(2, 2) (out_mode 1) of
// layer L on a B x H x W grid, reading L's packed weights; the caller adds relu / scale / shift / output grid / fused epilogues.
inline mgu::IgemmDesc layer_desc(const mgu_ctx* c, const Layer& L, const void* in, int ldin, int B, int H, int W, void* out, int ldout, int coff) {
  mgu::IgemmDesc d;
  memset(&d, 0, sizeof d);
  d.tn = &c->tn;
  d.in = (const float*)in;   // element type follows c->dtype; the descriptor carries raw pointers
  d.w = L.wp, d.wu = L.wu, d.out = (float*)out;
  d.M = B * H * W, d.H = H, d.W = W;
  d.Cp = L.Cp, d.ldin = ldin, d.KS = L.KS, d.K = L.K, d.Kp = L.Kp;
  d.N = L.N, d.ldout = ldout, d.coff = coff;
  d.out_mode = L.convt ? 1 : 0, d.ct_cout = L.Cout;
  return d;
}
// The data gradient of layer L on the grid of its forward r as a gather over dz (pitch lddz): KS 1 / 3 is the
// conv with the flipped, transposed weights (Cout rounded up to 4 channels), a ConvTranspose the 2x2 stride-2 gather from its
// Hout x Wout output.  `panel` is the direct-panel form; the caller offers the other forms in d.wu.
inline mgu::IgemmDesc dgrad_desc(const mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dz, int lddz, const float* panel,
                            float* out, int ldout, int Hout = 0, int Wout = 0) {
  const int KS = L.convt ? 2 : L.KS, Cop = rup(L.Cout, 4);
  mgu::IgemmDesc d;
  memset(&d, 0, sizeof d);
  d.tn = &c->tn;
  d.in = dz, d.w = panel, d.out = out;
  d.M = r.B * r.H * r.W, d.H = r.H, d.W = r.W;
  d.Cp = Cop, d.ldin = lddz, d.KS = KS, d.K = KS * KS * Cop, d.Kp = rup(d.K, 32);
  d.N = L.Cin, d.ldout = ldout, d.Hout = Hout, d.Wout = Wout;
  return d;
}
// A plain GEMM out = in (M x K) * panel^T (N columns, row pitch Kp), columns >= split_n going to out2 (pitch ld2)
inline mgu::IgemmDesc gemm_desc(const mgu_ctx* c, const float* in, int M, int K, const float* panel, int Kp, int N, float* out, int ldout,
                           int split_n, float* out2, int ld2) {
  mgu::IgemmDesc d;
  memset(&d, 0, sizeof d);
  d.tn = &c->tn;
  d.in = in, d.w = panel, d.out = out;
  d.M = M, d.H = 1, d.W = M;
  d.Cp = K, d.ldin = K, d.KS = 1, d.K = K, d.Kp = Kp;
  d.N = N, d.ldout = ldout;
  d.split_n = split_n, d.out2 = out2, d.ld2 = ld2;
  return d;
}
// A weight gradient dW[n][k] = sum_m z[m][n] * gather(in)[m][k] over the B x H x W rows: KS 1 / 3 gathers a conv's input, KS 2 a
// ConvTranspose's output (stride 2 from Hs x Ws); partial panels in dw (dw_capacity floats)
inline mgu::WgradDesc wgrad_desc(const mgu_ctx* c, const float* z, int ldz, const float* in, int ldin, int inoff, int Cp, int KS, int B, int H,
                            int W, int Hs, int Ws, int N, float* dw, size_t dw_capacity) {
  mgu::WgradDesc d;
  memset(&d, 0, sizeof d);
  d.tn = &c->tn;
  d.z = z, d.ldz = ldz;
  d.in = in, d.ldin = ldin, d.inoff = inoff, d.Cp = Cp;
  d.KS = KS;
  d.M = B * H * W, d.H = H, d.W = W, d.Hs = Hs, d.Ws = Ws;
  d.N = N, d.K = KS * KS * Cp, d.Kp = rup(d.K, 32);
  d.dw = dw, d.dw_capacity = dw_capacity;
  return d;
}

// One fused conv / convT / 1x1 launch of a Layer: what it reads and writes (call sites name the fields they set, in this order) ...
struct ConvReq {
  const void* in = nullptr;   // pitch ldin, on a B x H x W grid
  int ldin = 0, B = 0, H = 0, W = 0;
  void* out = nullptr;        // pitch ldout, channels from coff
  int ldout = 0, coff = 0, relu = 0;
  const float *scale = nullptr, *shift = nullptr;   // chosen by the caller
  int Hout = 0, Wout = 0;     // output grid of a ConvTranspose
};
// ... the epilogues it may fuse where the kernel the pick chooses has them ...
struct ConvFusions {
  void* pool = nullptr;             // MaxPool2d(2) output
  int ldpool = 0;
  double* stat_slots = nullptr;     // BatchNorm batch statistics
  const mgu::WinoHead* head = nullptr;   // head-fused finishing pass (common.h)
};
// ... and which of them that kernel took: what it left out is the caller's to run in a pass of its own
struct ConvTaken {
  bool pool = false, stats = false, head = false;
  int stat_rows = 0;   // accumulator rows the statistics epilogue wrote
};
int run_layer(mgu_ctx* c, const Layer& L, const ConvReq& q, hipStream_t s, const ConvFusions& f = {}, ConvTaken* took = nullptr);
// Returns rc.  An error return may have come between a pass that leaves sums in the (otherwise self-cleaning) reduction slots and their
// fold: clear the slots then, or rows would stay non-zero for every later reduction
inline int red_cleared_on_error(mgu_ctx* c, int rc, hipStream_t s) {
  if (rc != MGU_OK && c && c->redws) (void)hipMemsetAsync(c->redws, 0, c->redws_bytes, s);
  return rc;
}

// GAT layer host code (gat_api.hip)
void gat_destroy(mgu_ctx* c);
// Fin, Fout_head (multiples of 4) and heads of a call to `fn`.  The eval schedules take 1..32 heads and heads * Fout_head <= 1024;
// the train forward and the backward (train) any number of heads, heads * Fout_head <= 256 and N * heads * Fout_head < 2^31.
int gat_check_layer(mgu_ctx* c, const char* fn, int Fin, int heads, int Fh, bool train = false, int N = 0);
// the graphs of a layer call (no graph_ptr or num_graphs < 1: one graph, graph_ptr NULL) and their per-(graph, head) max accumulators
int gmax_buffer(mgu_ctx* c, const int32_t** graph_ptr, int* num_graphs, int heads, unsigned long long** buf, unsigned* gen);
// the gather schedule's GEMM panel [W | W^T a_src | W^T a_tgt] (rup(HF + 2H, 128) rows of rup(Fin, 32)); `clear` zeroes its padding
size_t gat_panel_floats(int heads, int Fh, int Fin);
int gat_pack_panel(mgu_ctx* c, const float* W, const float* a, float* panel, int heads, int Fh, int Fin, bool clear, hipStream_t s);
// (gat_bwd.hip) The gather schedule's prologue: Wh (N, HF) and the attention scalars st (N, 2H) = [s | t] from ONE GEMM on `panel`,
// the node -> graph table (G > 1), the per-graph max into the accumulators (gmax, gen) and, when gm != NULL, the max decoded into
// a plain (G, H) float table.  `record` adds the eval forward's profiling records.
int gat_prologue(mgu_ctx* c, const float* X, int N, int Fin, const float* panel, int heads, int Fh, const int32_t* rowptr, const int32_t* col,
                 int64_t E, const int32_t* gp, int G, float alpha, unsigned long long* gmax, unsigned gen, float* wh, float* st,
                 int32_t* node_graph, float* gm, bool record, hipStream_t s);

// object labelling (objects.hip), shared with split.hip and clean.hip.  cc_roots_i32: P[g] = the smallest linear index (over the whole
// batch) of the 8-connected (conn8 false: 4-connected) same-value component of g in an int32 map (B, H, W), -1 where the map is 0.  cc_number_roots: given P with every
// foreground pixel pointing (directly or through a chain) at its object's first pixel, the tail of mgu_connected_components: objects
// numbered per image in raster order of that pixel, the min_area filter (area: n counters, or nullptr with min_area 0), counts and
// offsets.  cnt: cc_chunks(HW) * B ints, choff: as many int64.  (The device and host helpers the object-level files share beyond
// these two entry points are in objects_common.h.)
int64_t cc_chunks(int64_t HW);
int cc_roots_i32(mgu_ctx* c, const int32_t* map, int B, int H, int W, int* P, hipStream_t s, bool conn8 = true);
int cc_number_roots(mgu_ctx* c, int* P, unsigned* area, int min_area, int B, int64_t HW, int* cnt, long long* choff, int32_t* labels,
                    int64_t* counts, int64_t* offsets, hipStream_t s);

// gradient exchange (comm.hip)
int comm_bucket(mgu_ctx* c, float* flat, int64_t lo, int64_t hi, hipStream_t s);
int comm_join(mgu_ctx* c, hipStream_t s);

int repack_weights(mgu_ctx* c, hipStream_t s);   // mgunet_api.hip: every packed weight form from the recorded parameter tensors
// training path (mgunet_train.hip)
// Scratch of the backward launches: partial weight-gradient panels, the data-gradient weight form, reduction slots
struct BwdScratch {
  float *dwp = nullptr, *dgp = nullptr;
  size_t dwp_floats = 0, dgp_floats = 0;
  double *red = nullptr, *sums = nullptr;
  bool clear = false;   // zero a direct panel before packing it (the building blocks)
};
// The four backward operations of layer L on the forward recorded in r (mgu_unet_backward on mgu_ctx::fwd, the building blocks of
// bwd_blocks.hip on the caller's tensors).  Each picks its kernel once, packs the weight form that kernel reads -- unless the layer
// keeps a current one (L.wug, L.wxg) -- and launches; `record` adds a profiling record.
int conv_dgrad(mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dz, float* out, int ldout, const BwdScratch& w, bool record,
               hipStream_t s);
int convt_dgrad(mgu_ctx* c, const Layer& U, const FwdRecord& r, const float* dout, int ld_d, int Hout, int Wout, float* out,
                const BwdScratch& w, bool record, hipStream_t s);
// dz dense with pitch rup(Cout, 4); fold_rows != nullptr: also folds the bias-gradient column sums pending in w.red (conv_bn_relu_backward)
int conv_wgrad(mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dz, float* dw, const BwdScratch& w, bool record, hipStream_t s,
               int* fold_rows = nullptr, float* dbias = nullptr);
int convt_wgrad(mgu_ctx* c, const Layer& U, const FwdRecord& r, const float* dout, int ld_d, int c_off, int Hout, int Wout, float* dw,
                const BwdScratch& w, hipStream_t s);
// the context's reduction slots (mgu_ctx::redws) sized for layers of up to Cmax channels; a fresh allocation is cleared, once
int ensure_red(mgu_ctx* c, int Cmax);
// One conv -> BatchNorm(train) -> ReLU of the training forward on layer L and the tensors of r: the batch statistics come from the
// convolution's epilogue where its kernel accumulates them (took->stats), else from a pass over z.  pooled != nullptr: also
// MaxPool2d(2) of y, in the apply pass for even H and W (took->pool), else by the pool kernel on y.
int conv_bn_relu_train(mgu_ctx* c, const Layer& L, const FwdRecord& r, double* sums, double* red, hipStream_t s, float* pooled = nullptr,
                       ConvTaken* took = nullptr);
// Where the backward of that half block writes the layer's parameter gradients
struct LayerGrads {
  float *dw = nullptr, *dbias = nullptr, *dgamma = nullptr, *dbeta = nullptr;
};
// ... and its backward on the same record: BatchNorm + ReLU backward (dy with pitch lddy -> dz dense; the column sums of dz stay in the
// reduction slots), the weight gradient, whose unpack launch folds those sums into the bias gradient, and -- din != nullptr -- the
// data gradient (pitch ld_din)
int conv_bn_relu_backward(mgu_ctx* c, const Layer& L, const FwdRecord& r, const float* dy, int lddy, float* dz, const LayerGrads& g,
                          float* din, int ld_din, const BwdScratch& w, hipStream_t s);
size_t train_ws_bytes(const mgu_ctx* c, int B, int H, int W);
int unet_forward_train(mgu_ctx* c, const float* x, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w, int B, int H,
                       int W, float* logits, void* const* cat_dev, void* const* feat_dev, hipStream_t s);

}  // namespace mgud
