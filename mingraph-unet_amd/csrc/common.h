// Internal declarations shared by the HIP translation units of libmgunet.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device.h"

namespace mgu {

// ---- host launch helpers ----
// workgroups of a grid-stride kernel: one per `threads` items of work, at least 1, at most `cap`
inline int grid_for(int64_t work, int threads, int cap) {
  int64_t b = (work + threads - 1) / threads;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (int)b;
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM descriptor.  D[m][n] = act(scale[n] * sum_k A(m,k) * Wp[n][k] + shift[n])
//   A(m,k) is gathered on the fly from an NHWC activation tensor:
//     k = tap*Cp + c, tap = (r*KS + s); A = in[img, oy + r - KS/2, ox + s - KS/2, c]  (0 outside)
//   Wp is the packed weight panel [Np][Kp] (k contiguous), zero padded.
// out_mode 0: D row m -> out[m*ldout + coff + n]                       (conv3x3 / 1x1 / linear)
// out_mode 1: ConvTranspose2d k2 s2 pixel-shuffle: n = (dy*2+dx)*ct_cout + co,
//             m = (img, y, x) over the INPUT grid H x W,
//             -> out[((img*Hout + 2y+dy)*Wout + 2x+dx)*ldout + coff + co]
// ---------------------------------------------------------------------------------------------
// Kernel-selection switches of ONE context (mgu_ctx::tn, filled from the MGU_* environment in mgu_create).  They ride in
// the launch descriptors, so two contexts of a process never see each other's settings.  The convolution switches are read
// only by the picks (pick_conv, pick_wgrad) and by the layer-level predicates next to pick_conv that size weight forms.
struct Tuning {
  bool first_mfma = true;   // MGU_NO_FIRST_MFMA=1: the first convolution on the VALU kernel (conv3x3_first_kernel) instead of the matrix cores (A/B)
  bool use_wino = true;     // MGU_NO_WINOGRAD=1: direct kernels for the fp32 3x3 layers
  int wino_prec = 1;        // MGU_WINO_PREC: 1 = three exact bf16 pieces per fp32 operand on the bf16 MFMA (default),
                            //                0 = fp32 MFMA operands
  bool convt_frag = true;   // MGU_NO_CONVT_FRAG=1: ConvTranspose on the generic tile kernel instead of convt_x3.hip's kernels (A/B)
  bool wino_cp = true;      // MGU_NO_WINO_CP=1: the four-components-per-wave kernel instead of the component-pair split (A/B)
  int wino_ppb_cap = 32;    // MGU_WINO_PPB_CAP: patches a Winograd workgroup walks at most
  bool wgrad_halo = true;   // MGU_NO_WGRAD_HALO=1
  bool wino_wgrad = true;   // MGU_NO_WINO_WGRAD=1
  bool convt_dgrad_x3 = true;   // MGU_NO_CONVT_DGRAD_X3=1: ConvTranspose data gradient on the generic fp32 tile kernel
  bool wgrad_x3 = true;     // MGU_NO_WGRAD_X3=1: Winograd weight gradient on the fp32 MFMA instead of the three-piece bf16 products
  bool wgrad_thin = true;   // MGU_NO_THIN_WGRAD=1
  bool wino_dgrad = true;   // MGU_NO_WINO_DGRAD=1
  bool gat_fused = true;    // MGU_NO_GAT_FUSED=1
  bool head_fused = true;   // MGU_HEAD_FUSED=0: the 1x1 head and the patch means in their own pass over decoder feature 0 (patch_mean_kernel)
                            // instead of the finishing pass of the convolution that writes it (WinoHead below; A/B and tests)
  bool wino_asm = true;     // MGU_WINO_ASM=0: the C++ component-pair kernels instead of their hand-scheduled assembly forms (wino_asm.hip; bitwise
                            // equal results)
  bool convt_asm = true;    // MGU_CONVT_ASM=0: the C++ ConvTranspose kernel instead of its hand-scheduled assembly form (convt_x3.hip,
                            // asm/gen_convt_x3.py; bitwise equal results)
  int fwd_groups = 2;       // MGU_FWD_GROUPS: 2 (default) = the eval U-Net forward of a batch of >= 2 images as two half-batch walks, the
                            // second on the context's side stream, so that one half's workgroups fill the CUs while the other half's
                            // kernel drains and its next packet is handed over; 1 = the whole batch on the caller's stream
                            // (mgu_unet_forward; bitwise equal results, profiles/forward_groups_ab.txt)
  int lovasz_passes = 4;    // MGU_LOVASZ_PASSES: 4 (default) = the Lovasz sort's 31 key bits as 8 + 8 + 8 + 7, 3 = as 10 + 10 + 11 (lovasz.hip;
                            // bitwise equal results, 2 - 3 % slower: profiles/lovasz_bench.txt)
};
const Tuning& default_tuning();
// The >64 KB dynamic-LDS opt-in is a per-DEVICE function attribute: set it once per (kernel, device).
hipError_t ensure_dyn_lds(const void* func, size_t bytes, bool (&done)[64]);

struct IgemmDesc {
  const Tuning* tn;    // nullptr = default_tuning()
  const float* in;
  const float* w;
  const float* wu;     // optional: Winograd-transformed 3x3 weights (pack_wino, pack.hip); enables wino_f32.hip
  const float* scale;  // may be nullptr (== 1)
  const float* shift;  // may be nullptr (== 0)
  float* out;
  int M;        // rows = B*H*W
  int H, W;     // spatial grid that M enumerates
  int Cp;       // channels gathered per tap (multiple of 4)
  int ldin;     // channel pitch of `in` (elements between pixels)
  int KS;       // 1 or 3
  int K;        // KS*KS*Cp
  int Kp;       // row pitch of w (multiple of 32)
  int N;        // valid output columns
  int ldout;    // channel pitch of out
  int coff;     // channel offset inside the out pixel
  int relu;
  int out_mode;
  int ct_cout;     // out_mode 1: Cout (N == 4*Cout)
  int Hout, Wout;  // out_mode 1: output grid (>= 2H, 2W)
  // optional fused MaxPool2d(2) of the output (Winograd kernel only): pool[(img, y/2, x/2)*ldpool + n], floor semantics
  float* pool;
  int ldpool;
  // optional (Winograd kernel, training forward): per-channel sum / sum of squares of the stored output accumulated into the
  // row-per-workgroup double accumulator [STAT_ROWS][2 * N] (train_kernels.hip), folded by launch_bn_finalize_slots
  double* stat_slots;
  // optional split epilogue (out_mode 0): columns n >= split_n go to out2[m*ld2 + (n - split_n)] (0 = off)
  int split_n;
  float* out2;
  int ld2;
};

// Optional head-fused finishing pass of the narrow component-pair Winograd kernel (the launch that writes decoder feature 0, 32
// channels): every pixel's 32 outputs also go through the final 1x1 conv (unet_decoder.py:117,143), and each wave adds its 2 x 16
// pixels into the per-channel sum of their 16 x 16 graph patch -- one partial per row pair, plain stores into
// psum[node][8 row pairs][32], which launch_patch_sum_combine adds in a fixed order (bit-repeatable; no atomics).
struct WinoHead {
  const float* w;     // (ncls, 32), the reference's layout
  const float* b;     // (ncls)
  float* logits;      // NHWC fp32 (B, H, W, ncls)
  float* psum;        // scratch, wino_head_psum_bytes(B, H, W) bytes
  int ncls;           // 1..4
  int psum_bytes;
};
inline size_t wino_head_psum_bytes(int B, int H, int W) { return (size_t)B * (H / 16) * (W / 16) * 8 * 32 * sizeof(float); }

inline const Tuning& tun(const IgemmDesc& d) { return d.tn ? *d.tn : default_tuning(); }
// The kernel a convolution descriptor runs on.  pick_conv makes the choice once (it alone reads the conv switches of Tuning, through
// the descriptor-level *_applicable tests in igemm.hip); the launch, the profiling label and cost, the fused epilogues and the weight
// form a caller packs all follow from the returned value.
enum class ConvKernel {
  None,                                       // no kernel takes the descriptor: the launch returns hipErrorInvalidValue
  WinoAsmWide, WinoAsmCp1r2, WinoAsmCp1r4,    // mgu_wino_cp2 / cp1r2 / cp1r4_gfx950 (wino_asm.hip)
  WinoAsmCp1r2Head,                           // mgu_wino_cp1r2h_gfx950: cp1r2 with the head-fused finishing pass (WinoHead)
  WinoCp2, WinoCp1, WinoCp2Stats, WinoCp1Stats,   // wino3x3_cp_kernel<2|1, STATS> (wino_f32.hip)
  WinoCp1Head,                                // wino3x3_cp_kernel<1, HEAD>: the C++ twin of the head-fused form
  WinoF32Wide, WinoF32Narrow,                 // wino3x3_f32_kernel<0|1, 0>: fp32 MFMA operands (MGU_WINO_PREC=0)
  WinoX3Wide, WinoX3Narrow,                   // wino3x3_f32_kernel<0|1, 1>: three-piece bf16 operands
  HaloF32, HaloBf16Np8, HaloBf16Np4,          // conv3x3_halo_kernel
  TilesF32, TilesBf16,                        // igemm_kernel (KS, out_mode from the descriptor)
  ConvtX3, ConvtBf16f, ConvtX3Dgrad,          // convt2x2_x3_kernel, convt2x2_bf16_kernel, convt2x2_x3_kernel in its gather mode
  ConvtX3Asm,                                 // mgu_convt_x3_gfx950: the assembly form of convt2x2_x3_kernel's forward (same weight form)
};
// dtype: 0 = fp32, 1 = bf16 storage (in / w / out point to bf16, sizes in elements).  head: the caller would like the head-fused
// finishing pass; the pick returns one of the *Head kernels only if the descriptor and the switches admit it
ConvKernel pick_conv(const IgemmDesc& d, int dtype, const WinoHead* head = nullptr);
hipError_t launch_conv(const IgemmDesc& d, ConvKernel k, int dtype, hipStream_t s, const WinoHead* head = nullptr);   // k = pick_conv(d, dtype, head)
inline bool conv_fuses_head(ConvKernel k) { return k == ConvKernel::WinoAsmCp1r2Head || k == ConvKernel::WinoCp1Head; }
inline hipError_t launch_igemm_f32(const IgemmDesc& d, hipStream_t s) { return launch_conv(d, pick_conv(d, 0), 0, s); }
inline hipError_t launch_igemm_bf16(const IgemmDesc& d, hipStream_t s) { return launch_conv(d, pick_conv(d, 1), 1, s); }
const char* conv_kernel_name(ConvKernel k, const IgemmDesc& d);   // profiling label of a forward launch
const char* conv_dgrad_name(ConvKernel k, const IgemmDesc& d);    // ... of a data-gradient launch
struct ConvCost {
  double mfma;   // FLOPs issued on the matrix pipe
  int pipe;      // 0 = fp32 MFMA, 1 = bf16 MFMA
};
ConvCost conv_cost(ConvKernel k, const IgemmDesc& d);
inline bool conv_is_wino(ConvKernel k) { return k >= ConvKernel::WinoAsmWide && k <= ConvKernel::WinoX3Narrow; }
inline bool conv_fuses_pool(ConvKernel k) {   // the epilogue can also write the 2x2 max-pooled tensor (IgemmDesc::pool)
  return conv_is_wino(k) || (k >= ConvKernel::HaloF32 && k <= ConvKernel::HaloBf16Np4);
}
inline bool conv_reads_panel(ConvKernel k) {   // the kernel reads the direct panel d.w (the others read d.wu)
  return !conv_is_wino(k) && k != ConvKernel::ConvtX3 && k != ConvKernel::ConvtX3Asm && k != ConvKernel::ConvtBf16f &&
         k != ConvKernel::ConvtX3Dgrad;
}
inline bool conv_reads_convt_x3(ConvKernel k) {   // the forward kernels on pack_convt_x3's fragment-ordered pieces
  return k == ConvKernel::ConvtX3 || k == ConvKernel::ConvtX3Asm;
}
// Layer-level forms of the same choice, for the places that size or pack a weight form before a descriptor exists: the layer's
// shape and switches admit the kernel (the descriptor-level test in pick_conv checks the rest; a caller that holds no such form
// leaves d.wu null)
bool wino_layer(const Tuning& t, int KS, int Cp);             // fp32 3x3 conv on the Winograd kernels (U: pack_wino)
bool wino_dgrad_layer(const Tuning& t, int KS, int Cop);      // its data gradient too (Cop = Cout rounded up to 4)
bool convt_x3_layer(const Tuning& t, int Cin, int Cout);      // fp32 ConvTranspose on convt2x2_x3_kernel (pack_convt_x3)
bool convt_x3_dgrad_layer(const Tuning& t, int Cin, int Cout);   // its data gradient too (pack_convt_x3, dgrad = 1)
bool convt_bf16f_layer(const Tuning& t, int Cin, int Cout);   // bf16-storage ConvTranspose on convt2x2_bf16_kernel
// the convolution that writes a B x H x W x Cin feature may take the head-fused finishing pass (WinoHead) for a 1x1 head of ncls
// classes and patch means at `patch`: the caller sizes WinoHead::psum on it, pick_conv repeats it on the descriptor
bool wino_head_layer(const Tuning& t, int dtype, int Cin, int ncls, int patch, int B, int H, int W);
// wino_f32.hip: work split of the Winograd kernels.  8 x 32 pixel patches; a workgroup covers 64 output channels of a wide layer
// (N > 32), 32 of a narrow one, and walks ppb patches; item (n block, patch group) of XCD x is x * per_xcd + (workgroup / 8)
inline bool wino_wide(const IgemmDesc& d) { return d.N > 32; }
struct WinoPlan {
  int tiles_x, tiles_y, total, nblk, ppb, ngroups, per_xcd;
};
WinoPlan wino_plan(const IgemmDesc& d);
int wino_grid_blocks(const IgemmDesc& d);   // workgroups of the Winograd launch for d (= accumulator rows of its statistics)
// convt_x3.hip: fp32 ConvTranspose2d(k2,s2) on the bf16 matrix cores with exact three-way operand splits (IgemmDesc::wu =
// fragment-ordered weight pieces)
hipError_t launch_convt_x3(const IgemmDesc& d, hipStream_t s);
// its hand-scheduled assembly form (asm/gen_convt_x3.py; bitwise equal results) and the shapes it covers
bool convt_x3_asm_shape(const IgemmDesc& d);
hipError_t launch_convt_x3_asm(const IgemmDesc& d, hipStream_t s);
// convt_bf16.hip: the bf16-storage ConvTranspose2d(k2,s2) on fragment-ordered bf16 weights (IgemmDesc::wu), 16-byte transposed stores
hipError_t launch_convt_bf16f(const IgemmDesc& d, hipStream_t s);
// the same kernel as the layer's data gradient (KS = 2 gather descriptors whose d.wu holds pack_convt_x3's data-gradient form)
hipError_t launch_convt_x3_dgrad(const IgemmDesc& d, hipStream_t s);
// first_mfma.hip: the same layer on the bf16 matrix cores (Cin <= 3, Cout == 32)
bool first_mfma_applicable(int dtype, int Cin, int Cp, int Cout, int ldout, int coff, int64_t H, int64_t W);
hipError_t launch_first_mfma(int dtype, const void* in, const float* wfm, const float* scale, const float* shift, void* out, int B, int H,
                             int W, int ldout, int coff, int relu, hipStream_t s);
hipError_t launch_first_mfma_direct(int dtype, const float* x, int64_t sn, int64_t sc, int64_t sh, int64_t sw, int cin, const float* wfm,
                                    const float* scale, const float* shift, void* out, int B, int H, int W, int ldout, int coff, int relu,
                                    hipStream_t s);
// elementwise.hip: first convolution (<= 4 input channels on the packed NHWC4 input), VALU + scalar-cache weights
bool first_conv_applicable(int dtype, int Cin, int Cp, int Cout, int ldout, int coff);
hipError_t launch_first_conv(int dtype, const void* in, const float* wf, const float* scale, const float* shift, void* out, int B, int H, int W,
                             int Cin, int Cout, int ldout, int coff, int relu, hipStream_t s);
// wino_f32.hip: Winograd F(2x2,3x3) for fp32 3x3 layers with Cp % 16 == 0
hipError_t launch_wino_f32(const IgemmDesc& d, ConvKernel k, hipStream_t s, const WinoHead* head = nullptr);   // k: one of the C++ Winograd kernels
// patch means from the head-fused kernels' partial sums: out[node][c] = (psum[node][0][c] + ... + psum[node][7][c]) / 256
hipError_t launch_patch_sum_combine(const float* psum, float* out, int nodes, hipStream_t s);
// wino_asm.hip: the assembly forms of wino3x3_cp_kernel<2> and <1> (bitwise equal results; k: one of the WinoAsm* kernels)
hipError_t launch_wino_cp_asm(const IgemmDesc& d, ConvKernel k, hipStream_t s, const WinoHead* head = nullptr);

// pack.hip: every packed weight form.  A PackItem names one form to write: built by the form's constructor, run alone
// (launch_pack_one) or as an entry of a PackBatch table, many forms in one launch (launch_pack_batch).  w: the parameter tensor in the
// reference's layout, Conv2d (Cout, Cin, KS, KS) or ConvTranspose2d (Cin, Cout, 2, 2); dtype: MGU_DTYPE_* of a typed panel.
struct PackItem {
  const float* w;
  float* U;
  int Cout, Cin, Cp, Np, dgrad;   // as the Winograd set reads them; the other forms' use: their constructors (pack.hip)
  unsigned blk0;   // first workgroup of the item in its batch (pack_batch_prepare)
  int kind;
  int mode;        // Winograd prec / dtype of a typed panel.  No padding bytes: repack_weights compares the tables with memcmp to skip the upload
};
static_assert(sizeof(PackItem) == 48, "PackItem must have no padding");
PackItem pack_wino(const float* w, float* U, int Cout, int Cin, int Cp, int dgrad, int prec);   // dgrad: roles swapped, see pack_wino_w_body
PackItem pack_first_w(const float* w, float* wf, int Cout, int Cin);
PackItem pack_first_mfma(const float* w, float* wfm, int Cout, int Cin);
PackItem pack_convt_x3(const float* w, float* Wx, int Cin, int Cout, int dgrad);
PackItem pack_bias_tile(const float* bias, float* shift, int C, int reps);
PackItem pack_dgrad_panel(const float* w, float* wp, int Cout, int Cin, int Cop, int KS, int Kp);
PackItem pack_conv_panel(const float* w, void* wp, int dtype, int Cout, int Cin, int Cp, int KS, int Kp);
PackItem pack_convt_panel(const float* w, void* wp, int dtype, int Cin, int Cout, int Kp);
PackItem pack_convt_bf16f(const float* w, float* Wf, int Cin, int Cout);
PackItem pack_convt_dgrad_panel(const float* w, float* wp, int Cin, int Cout, int Kp);
size_t wino_u_floats(int Cout, int Cp);
size_t convt_x3_floats(int Cin, int Cout);
size_t convt_x3_dgrad_floats(int Cin, int Cout);
size_t convt_bf16f_floats(int Cin, int Cout);
size_t first_mfma_floats();
constexpr int PACK_MAX = 64;
struct PackBatch {
  int n;
  unsigned total_blocks;
  PackItem it[PACK_MAX];
};
bool pack_batch_prepare(PackBatch& b);   // fills blk0 / total_blocks; false if an item's shape does not fit its form
hipError_t launch_pack_batch(const PackBatch* batch_dev, unsigned total_blocks, hipStream_t s);
hipError_t launch_pack_one(const PackItem& it, hipStream_t s);   // hipErrorInvalidValue: the item's shape does not fit its form

// wgrad_f32.hip:  Dw[n][k] += sum_m Z[m][n] * A(m,k)   (A = the forward kernels' im2col gather)
struct WgradDesc {
  const Tuning* tn;  // nullptr = default_tuning()
  const float* z;   // Z[m][n] at z[m*ldz + zoff + n]
  int ldz, zoff;
  const float* in;  // gather source (NHWC), channels [inoff, inoff+Cp) of a pixel with pitch ldin
  int ldin, inoff, Cp;
  int KS;           // 1 | 3 (pad 1) | 2 (stride-2 2x2 gather from an Hs x Ws grid: ConvTranspose2d)
  int M, H, W;      // rows enumerate (img, y, x) over H x W
  int Hs, Ws;       // KS == 2 source grid
  int N, K, Kp;     // Dw panel [>=N][Kp]
  float* dw;        // [groups][>=N][Kp] partial panels; the launcher sets `groups`.  Plain stores, every element (n < N, k < K)
                    // of every partial panel written (no zeroing needed, no atomics); the caller sums the panels in order
  size_t dw_capacity;  // floats available at dw
  int groups;          // set by the launcher
  int rows_per_split;  // set by the launcher
};
inline const Tuning& tun(const WgradDesc& d) { return d.tn ? *d.tn : default_tuning(); }
// The weight-gradient kernel of a descriptor, picked once (it alone reads the weight-gradient switches of Tuning): the launch and
// the profiling label and cost follow from it
enum class WgradKernel {
  Thin,     // wgrad_thin.hip: the first 3x3 conv (Cin 3) and the 1x1 head
  WinoX3,   // wino_wgrad_f32_kernel<.., X3 = true>: three-piece bf16 products
  Wino,     // wino_wgrad_f32_kernel<.., X3 = false>: fp32 MFMA
  Halo,     // wgrad3x3_halo_f32_kernel
  Tiles,    // the generic tile kernels
};
WgradKernel pick_wgrad(const WgradDesc& d);
const char* wgrad_kernel_name(WgradKernel k);
struct WgradCost {
  double mfma;   // FLOPs issued on the matrix pipe for `alg` algorithmic FLOPs
  int pipe;      // 0 = fp32 MFMA, 1 = bf16 MFMA, -1 = none
};
WgradCost wgrad_cost(WgradKernel k, double alg);
hipError_t launch_wgrad_f32(WgradDesc& d, hipStream_t s);
// wino_wgrad_f32.hip: Winograd F(3x3,2x2) weight gradient (Cp % 32 == 0, N % 32 == 0); same partial-panel output as the halo kernel
hipError_t launch_wino_wgrad_f32(WgradDesc& d, bool x3, hipStream_t s);
// wgrad_thin.hip: the first 3x3 conv (Cin 3) and the 1x1 head: HBM-bound streaming kernels, same partial-panel output
hipError_t launch_wgrad_thin(WgradDesc& d, hipStream_t s);

// train_kernels.hip
// Per-channel reductions meet in a table of double rows [rows][2 * C]; every workgroup adds into a row of its OWN (row =
// blockIdx.x: one adder per element, onto zero), and the reader folds the rows in a fixed order and clears them -- so a sum is
// bitwise reproducible from run to run (64 shared slots with several adders each were not: the order of double atomics moved
// the last bit of a BatchNorm statistic about once in a thousand steps).  STAT_ROWS bounds the grid of the Winograd kernels
// that accumulate statistics in their epilogue (one round of <= 2 x 256 workgroups + rounding).
constexpr int STAT_ROWS = 576;
constexpr int CHAN_REDUCE_ROWS = 512;   // workgroups (= table rows) of a per-channel reduction: 2 per CU, each streaming with 4 loads in flight per thread
size_t chan_reduce_work_bytes(int Cmax);
hipError_t launch_bn_stats(const float* z, int ldz, int64_t M, int C, double* work, double* sums, hipStream_t s);
hipError_t launch_bn_finalize(const double* sum, const double* sumsq, int64_t M, float eps, float momentum,
                              const float* gamma, const float* beta, float* mean, float* invstd, float* scale,
                              float* shift, float* run_mean, float* run_var, int C, hipStream_t s);
hipError_t launch_bn_finalize_slots(double* slots, int nrows, double* sums, int64_t M, float eps, float momentum, const float* gamma,
                                    const float* beta, float* mean, float* invstd, float* scale, float* shift, float* run_mean,
                                    float* run_var, int C, hipStream_t s);
hipError_t launch_bn_apply_relu(const float* z, const float* scale, const float* shift, float* y, int ldy, int64_t M, int C,
                                hipStream_t s);
hipError_t launch_bn_apply_relu_pool(const float* z, const float* scale, const float* shift, float* y, int ldy, float* pooled, int B, int H,
                                     int W, int C, hipStream_t s);
hipError_t launch_bn_bwd_reduce(const float* dy, int lddy, const float* fwd_scale, const float* fwd_shift, const float* z, int ldz,
                                const float* mean, const float* invstd, int64_t M, int C, double* work, double* sums,
                                float* dbeta, float* dgamma, hipStream_t s);
hipError_t launch_bn_bwd_apply(const float* dy, int lddy, const float* fwd_scale, const float* fwd_shift, const float* z, const float* mean,
                               const float* invstd, const float* gamma, const double* sums, int64_t M, int C, float* dz,
                               double* work, float* dbias, hipStream_t s);
hipError_t launch_bn_bwd_apply_deferred(const float* dy, int lddy, const float* fsc, const float* fsh, const float* z, const float* mean,
                                        const float* invstd, const float* gamma, const double* sums, int64_t M, int C, float* dz,
                                        double* work, int* rows, hipStream_t s);
hipError_t launch_colsum(const float* z, int ldz, int64_t M, int C, double* work, float* out, hipStream_t s);
hipError_t launch_maxpool2_bwd_add(const float* y, int ldy, const float* dpool, float* dskip, int ldd, int B, int H, int W,
                                   int C, hipStream_t s);
hipError_t launch_zero_pad_region(float* buf, int ld, int coff, int C, int B, int H, int W, int h2, int w2, hipStream_t s);
hipError_t launch_ce(const float* logits, const int64_t* labels, int64_t M, int C, long long ignore_index, float grad_scale,
                     float* dlogits, int ldd, double* acc, int* err_word, float* loss_out, hipStream_t s);
hipError_t launch_unpack_conv_grad(const float* dwp, int groups, size_t panel_stride, float* g, int Cout, int Cin, int Cp, int KS,
                                   int Kp, hipStream_t s, double* fold_slots = nullptr, int fold_rows = 0, int fold_n = 0, float* fold_out = nullptr);
hipError_t launch_unpack_convt_grad(const float* dwp, int groups, size_t panel_stride, float* g, int Cin, int Cout, int Kp, hipStream_t s);
hipError_t launch_sgd(float* p, const float* g, float* buf, int64_t n, float lr, float momentum, float wd, int step, float grad_scale,
                      hipStream_t s);
hipError_t launch_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, double b1, double b2, float eps,
                       float wd, int step, float grad_scale, hipStream_t s);

// elementwise.hip
// dtype: 0 = fp32, 1 = bf16 storage (MGU_DTYPE_*); void* buffers hold that type
hipError_t launch_pack_input(const float* x, void* out, int dtype, int B, int C, int Cp, int H, int W, int64_t sn, int64_t sc,
                             int64_t sh, int64_t sw, hipStream_t s);
hipError_t launch_maxpool2(const void* in, int ldin, void* out, int dtype, int B, int H, int W, int C, hipStream_t s);
bool patch_mean_head_fusable(int dtype, int C, int ncls);
hipError_t launch_patch_mean(const void* feat, int dtype, float* out, int B, int H, int W, int C, int patch, hipStream_t s,
                             const float* head_w = nullptr, const float* head_b = nullptr, float* logits = nullptr, int ncls = 0);
hipError_t launch_bn_fold(const float* bias, const float* gamma, const float* beta, const float* mean, const float* var,
                          float eps, float* scale, float* shift, int C, hipStream_t s);
hipError_t launch_conv1x1_head(const void* in, int dtype, int ldin, int C, const float* w, const float* bias, float* out,
                               int ldout, int ncls, int64_t npix, hipStream_t s);
hipError_t launch_argmax(const float* logits, int64_t npix, int C, int64_t* pred, hipStream_t s);

// gat.hip
hipError_t launch_gat_wa_rows(const float* W, const float* a, float* panel, int row0, int heads, int Fh, int Fin, int Kp, hipStream_t s);
// gat_fused.hip: aggregate-first path (Fin <= F')
bool gat_fused_applicable(int Fin, int heads, int Fh, int64_t E);
size_t gat_fused_scratch_floats(int Fin, int heads, int Fh);
hipError_t launch_gat_prep(const float* W, const float* a, float* wa, unsigned* Wx, int heads, int Fh, int Fin, hipStream_t s);
hipError_t launch_gat_stmax(const float* x, const float* wa, int N, int Fin, int heads, const int32_t* rowptr, const int32_t* col,
                            const int32_t* gp, int G, float alpha, float* st, int32_t* node_graph, unsigned long long* gmax, int gstride,
                            unsigned gen, hipStream_t s);
hipError_t launch_gat_fused(const float* x, int Fin, const float* st, const int32_t* rowptr, const int32_t* col, const int32_t* gp, int G,
                            const unsigned long long* gmax, const unsigned* Wx, int N, int heads, int Fh, int concat, float alpha, float* out,
                            int gstride, unsigned gen, hipStream_t s);
hipError_t launch_gat_node_graph(const int32_t* gp, int G, int nodes_per_graph, int N, int32_t* node_graph, hipStream_t s);
hipError_t launch_gat_edge_max(const float* st, const int32_t* rowptr, const int32_t* col, const int32_t* node_graph, int N,
                               int heads, float alpha, unsigned long long* gmax_enc, int gstride, unsigned gen, hipStream_t s);
hipError_t launch_gat_aggregate(const float* wh, int P, const float* st, const int32_t* rowptr, const int32_t* col,
                                const int32_t* node_graph, const unsigned long long* gmax_enc, int N, int64_t E, int heads, int Fh,
                                int concat, float alpha, float* out, int gstride, unsigned gen, hipStream_t s);

}  // namespace mgu
