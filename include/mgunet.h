/*
 * mgunet.h -- C-ABI of libmgunet.so: the MI355X (gfx950) MinGraph-UNet segmentation hot path.
 *
 * The reference (agent-charon/MinGraph-UNet) has no FFI, plugin or operator registry: its hot
 * path sits behind three Python classes.  Each entry point below names the reference interface
 * it replaces (paths relative to MinGraph-UNet/).  A maintainer binds these with ctypes -- see
 * INTEGRATION.md for the stub that swaps them in under the reference's own nn.Modules.
 *
 * Conventions
 *   - every pointer named *_dev / documented "device" is a HIP device pointer owned by the caller;
 *   - activations are NHWC ("channels_last") fp32 in device memory; logical shapes stay NCHW;
 *   - all work is enqueued on `hip_stream` (a hipStream_t passed as void*); no hidden syncs
 *     except inside mgu_*_reserve / the first call that has to grow the library-owned workspace;
 *   - every function returns MGU_OK (0) or a negative error code; mgu_last_error(ctx) gives text;
 *   - a ctx is bound to one device and is not thread-safe.
 */
#ifndef MGUNET_H
#define MGUNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MGU_OK 0
#define MGU_ERR_INVALID -1   /* bad argument / unsupported shape (shim raises ValueError)   */
#define MGU_ERR_HIP -2       /* a HIP runtime call failed (shim raises RuntimeError)          */
#define MGU_ERR_STATE -3     /* call order violated, e.g. forward before load_weights         */
#define MGU_ERR_NOMEM -4

#define MGU_DTYPE_F32 0
#define MGU_DTYPE_BF16 1     /* bf16 storage + fp32 accumulate, inference only (BASELINE config 3) */

typedef struct mgu_ctx mgu_ctx;

/* One named parameter/buffer of a state_dict(); `ptr` is a device pointer to contiguous fp32
 * (int64 for num_batches_tracked, which is ignored).  Names are the reference's state_dict keys
 * (SURVEY.md 8b): "encoder.encoder_blocks.0.conv1.weight", "gat_layers.0.heads.2.a.weight", ... */
typedef struct {
  const char* name;
  const void* ptr;
  int64_t numel;
} mgu_tensor_desc;

/* ---- context ------------------------------------------------------------------------------ */
int mgu_create(int device_id, mgu_ctx** out);
void mgu_destroy(mgu_ctx* ctx);
const char* mgu_last_error(mgu_ctx* ctx); /* ctx may be NULL: returns the last create() error */
const char* mgu_version(void);

/* ---- U-Net: replaces model/unet/unet_model.py:6-36 (UNet.__init__/forward) ------------------- */
/* = UNet(in_channels, num_classes, init_features, depth) (unet_model.py:7).  init_features must be
 * a multiple of 4 (NHWC 16-byte lanes).  dtype MGU_DTYPE_BF16 (init_features % 8 == 0, <= 4 classes): every
 * activation the forward writes (cat_dev, feat_dev) and the packed weights are bf16, accumulation and the
 * bias/BatchNorm epilogue stay fp32, x_dev and logits_dev stay fp32; eval mode only. */
int mgu_unet_configure(mgu_ctx* ctx, int in_channels, int num_classes, int init_features, int depth, int dtype);
/* Number of fp32 elements of all trainable parameters, in state_dict order (7 766 018 for (3,2,32,4)). */
int64_t mgu_unet_param_count(mgu_ctx* ctx);
/* = load_state_dict: repacks OIHW conv weights to the kernels' [Cout][tap][Cin] panels, and for
 * eval folds bias + BatchNorm running stats (unet_encoder.py:12-13, eps 1e-5) into a per-channel
 * scale/shift applied in the conv epilogue.  Must be re-called after the parameters change. */
int mgu_unet_load_weights(mgu_ctx* ctx, const mgu_tensor_desc* named, int n, void* hip_stream);
/* The parameter tensors recorded by the last mgu_unet_load_weights were modified IN PLACE (same addresses: an optimizer step
 * through the flat parameter buffer, scripts/train_segmentation.py:134): rebuild every packed weight form from them -- one launch
 * for all Winograd sets (forward and, once the context has trained, data-gradient), the eval BatchNorm fold stays lazy.  The
 * train step calls this instead of going through the named state_dict again. */
int mgu_unet_refresh_weights(mgu_ctx* ctx, void* hip_stream);

/* Bytes of library-owned scratch a forward of this shape uses (allocated on first use).  training = 1: the train-mode
 * forward + backward scratch (every layer's pre-activation and activation, gradient temporaries, weight-gradient partial
 * panels: about 1.9 GB at 4 x 3x512x512), a separate allocation from the eval scratch. */
int mgu_unet_workspace_bytes(mgu_ctx* ctx, int B, int H, int W, int training, size_t* out);
/* Pre-allocate that scratch (synchronous); forward does it lazily otherwise. */
int mgu_unet_reserve(mgu_ctx* ctx, int B, int H, int W, int training);
/* = logits, skips, dec_feats = UNet.forward(x)  (unet_model.py:34-36); training=0: eval mode (BatchNorm folded),
 * training=1: train mode (see "training step" below).
 *   x_dev      : input, element (n,c,y,x) at x_dev[n*xs_n + c*xs_c + y*xs_h + x*xs_w] (fp32; any layout)
 *   logits_dev : (B,H,W,num_classes) NHWC
 *   cat_dev[i] : i = 0..depth-1 shallow->deep, NHWC buffer (B,H_i,W_i,2*C_i), C_i = init_features<<i,
 *                H_i = H>>i.  Channels [0,C_i) receive skip connection i (unet_encoder.py:69); channels
 *                [C_i,2*C_i) receive the up-sampled decoder input (unet_decoder.py:36-53), i.e. the
 *                buffer IS torch.cat([skip, up], 1) and no concat kernel ever runs.
 *   feat_dev[i]: decoder feature i shallow->deep, NHWC dense (B,H_i,W_i,C_i) (unet_decoder.py:141,149)
 * All outputs stay valid after the call (caller-owned). */
int mgu_unet_forward(mgu_ctx* ctx, const void* x_dev, int B, int H, int W,
                     int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w,
                     void* logits_dev, void* const* cat_dev, void* const* feat_dev,
                     int training, void* hip_stream);
/* Building blocks (also used by the kernel-level parity tests): one fused Conv2d(k=1|3, pad=k/2, bias)
 * [+ per-channel scale/shift] [+ ReLU] on an NHWC fp32 tensor, = nn.Conv2d.forward as used at
 * unet_encoder.py:7-8,16-24 and unet_decoder.py:117; weights in the reference's OIHW layout (device).
 * scale_dev/shift_dev may be NULL (then y = conv + bias).  in: (B,H,W,Cin) with Cin % 4 == 0; out: pixel
 * pitch ld_out >= c_off + Cout floats (lets the result land in a channel slice of a wider buffer). */
int mgu_conv2d_nhwc(mgu_ctx* ctx, const void* in_dev, int B, int H, int W, int Cin, const void* w_oihw_dev,
                    const void* bias_dev, const void* scale_dev, const void* shift_dev, int Cout, int ksize,
                    int relu, void* out_dev, int ld_out, int c_off, void* hip_stream);
/* Steady-state form of mgu_conv2d_nhwc: mgu_conv2d_nhwc repacks the OIHW weight into the kernels' panels (and the Winograd
 * transform) on EVERY call; a caller whose weights are constant between calls (an eval-mode nn.Conv2d, e.g. the two
 * convolutions of DetectionHead, detection_head.py:33,36) packs them once.  The handle is owned by the library and stays
 * valid until mgu_conv2d_release; re-prepare after the weight tensor changes.  bias/scale/shift as for mgu_conv2d_nhwc. */
typedef struct mgu_conv_weights mgu_conv_weights;
int mgu_conv2d_prepare(mgu_ctx* ctx, const void* w_oihw_dev, int Cout, int Cin, int ksize, mgu_conv_weights** out, void* hip_stream);
void mgu_conv2d_release(mgu_ctx* ctx, mgu_conv_weights* w);
int mgu_conv2d_prepared_nhwc(mgu_ctx* ctx, const mgu_conv_weights* w, const void* in_dev, int B, int H, int W, const void* bias_dev,
                             const void* scale_dev, const void* shift_dev, int relu, void* out_dev, int ld_out, int c_off,
                             void* hip_stream);
/* ConvTranspose2d(Cin, Cout, kernel_size=2, stride=2) + bias (unet_decoder.py:25,36); weight (Cin,Cout,2,2).
 * in (B,H,W,Cin) NHWC -> out (B,2H,2W,*) NHWC with pixel pitch ld_out, channels [c_off, c_off+Cout). */
int mgu_conv_transpose2x2_nhwc(mgu_ctx* ctx, const void* in_dev, int B, int H, int W, int Cin, const void* w_iohw_dev,
                               const void* bias_dev, int Cout, void* out_dev, int ld_out, int c_off, void* hip_stream);
/* MaxPool2d(2,2) floor mode (unet_encoder.py:48) on NHWC, input pixel pitch ld_in >= C. */
int mgu_maxpool2x2_nhwc(mgu_ctx* ctx, const void* in_dev, int ld_in, int B, int H, int W, int C, void* out_dev,
                        void* hip_stream);
/* argmax over classes of NHWC logits -> int64 (B,H,W): experiments/segmentation_performance.py:141 */
int mgu_argmax_classes(mgu_ctx* ctx, const void* logits_dev, int64_t npix, int num_classes,
                       int64_t* pred_dev, void* hip_stream);

/* ---- training step: replaces the autograd graph of scripts/train_segmentation.py:121-134 ---------- */
/* mgu_unet_forward(training=1) is the train-mode forward: BatchNorm uses batch statistics (biased
 * variance), updates running_mean/var IN PLACE in the tensors given to mgu_unet_load_weights (momentum
 * 0.1, unbiased variance; unet_encoder.py:12-13) and keeps the activations backward needs in library
 * scratch.  The forward's caller-owned outputs must stay alive until mgu_unet_backward returns.
 *
 * Offset (elements) of a parameter in the flat parameter/gradient vector; the order is the reference's
 * named_parameters() order.  name = state_dict key of a weight/bias; -1 if unknown. */
int64_t mgu_unet_param_offset(mgu_ctx* ctx, const char* name);
/* nn.CrossEntropyLoss() (mean reduction, ignore_index = -100: torch's defaults) forward + gradient
 * (train_segmentation.py:91,127): logits_dev (npix, C) NHWC fp32, labels_dev int64 (npix).
 * Writes *loss_dev = mean over the counted pixels of -log softmax(l_i)[y_i] and dlogits_dev (npix, 4*ceil(C/4)) =
 * grad_scale * npix/count * (softmax - onehot), pad columns zero: grad_scale = 1/npix reproduces loss.backward() of the
 * mean loss.  A pixel labelled -100 is not counted and gets a zero gradient (torch semantics).  Any other label outside
 * [0, C) is invalid DATA, which the host cannot see without a synchronisation: the label is never used as an index, the
 * loss comes out NaN, and the NEXT mgu_cross_entropy / mgu_unet_backward / mgu_sync_check on this ctx that runs after the
 * kernel has executed returns MGU_ERR_INVALID (torch raises IndexError / device-asserts at the same point). */
int mgu_cross_entropy(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int64_t npix, int num_classes,
                      float grad_scale, void* dlogits_dev, float* loss_dev, void* hip_stream);
/* Synchronise hip_stream and report invalid data met by kernels of this ctx since the last check (MGU_ERR_INVALID). */
int mgu_sync_check(mgu_ctx* ctx, void* hip_stream);
/* loss.backward() (train_segmentation.py:133) for the last mgu_unet_forward(training=1): dlogits_dev as
 * produced by mgu_cross_entropy; every element of flat_grad_dev (mgu_unet_param_count floats) is written. */
int mgu_unet_backward(mgu_ctx* ctx, const void* dlogits_dev, void* flat_grad_dev, void* hip_stream);
/* Test hooks: what mgu_unet_backward reads of the last mgu_unet_forward(training=1) of this ctx, per layer, read-only.  `layer` is the
 * state_dict prefix of a convolution: "encoder.encoder_blocks.0.conv1", "encoder.bottleneck.conv2",
 * "decoder.decoder_blocks.1.conv_block.conv1", "decoder.decoder_blocks.1.upsample", "decoder.final_conv".
 * mgu_unet_train_record_dims: the grid the layer ran on (a ConvTranspose's INPUT grid) and its channel counts.
 * mgu_unet_train_record_copy: copies (pitched device-to-device copies on hip_stream) into caller-owned DENSE fp32 device tensors, each
 * skipped when NULL: in (B,H,W,Cin) the layer's input (the first Cin channels of its pixels), z (B,H,W,Cout) the convolution's output
 * in front of the BatchNorm, y (B,H,W,Cout) = relu(bn(z)), mean / invstd (Cout) the batch statistics.  An up-convolution and the final
 * conv record their input only: asking them for z / y / mean / invstd is MGU_ERR_INVALID, as is an unknown or NULL name; without a
 * train-mode forward both return MGU_ERR_STATE.  Neither allocates anything that outlives the call nor changes any state. */
int mgu_unet_train_record_dims(mgu_ctx* ctx, const char* layer, int* B_out, int* H_out, int* W_out, int* Cin_out, int* Cout_out);
int mgu_unet_train_record_copy(mgu_ctx* ctx, const char* layer, void* in_dev, void* z_dev, void* y_dev, void* mean_dev, void* invstd_dev,
                               void* hip_stream);
/* ---- backward building blocks: ONE stage of loss.backward() each, through exactly the launchers mgu_unet_backward uses,
 *      on caller-provided NHWC fp32 tensors (kernel-level parity tests against float64; also usable on their own) ------
 * Weight gradient of Conv2d(k=1|3, pad=k/2) (unet_encoder.py:7-8): dw[co][ci][r][s] = sum_{b,y,x} dz[b,y,x,co] *
 * in[b, y+r-k/2, x+s-k/2, ci].  in: (B,H,W,ld_in), ld_in % 4 == 0, channels [Cin, ld_in) zero; dz: (B,H,W,ceil4(Cout)) with
 * zero pad columns; dw_oihw_dev: (Cout,Cin,k,k), every element written. */
int mgu_conv2d_wgrad_nhwc(mgu_ctx* ctx, const void* in_dev, int ld_in, const void* dz_dev, int B, int H, int W, int Cin, int Cout,
                          int ksize, void* dw_oihw_dev, void* hip_stream);
/* Data gradient of the same layer: din[b,y,x,ci] = sum dz[b, y-r+k/2, x-s+k/2, co] * w[co][ci][r][s];
 * dz as above, din_dev: (B,H,W,ld_out >= Cin). */
int mgu_conv2d_dgrad_nhwc(mgu_ctx* ctx, const void* dz_dev, const void* w_oihw_dev, int B, int H, int W, int Cin, int Cout, int ksize,
                          void* din_dev, int ld_out, void* hip_stream);
/* ConvTranspose2d(Cin, Cout, 2, stride 2) (unet_decoder.py:25,36): in (B,H,W,Cin); dout = channels [c_off, c_off+Cout) of a
 * (B,2H,2W,ld_d) tensor; dw_iohw_dev (Cin,Cout,2,2); dbias_dev (Cout) or NULL. */
int mgu_conv_transpose2x2_wgrad_nhwc(mgu_ctx* ctx, const void* in_dev, const void* dout_dev, int ld_d, int c_off, int B, int H, int W,
                                     int Cin, int Cout, void* dw_iohw_dev, void* dbias_dev, void* hip_stream);
int mgu_conv_transpose2x2_dgrad_nhwc(mgu_ctx* ctx, const void* dout_dev, int ld_d, int c_off, const void* w_iohw_dev, int B, int H,
                                     int W, int Cin, int Cout, void* din_dev /* (B,H,W,Cin) */, void* hip_stream);
/* Train-mode BatchNorm2d (eps 1e-5, momentum 0.1, unet_encoder.py:12-13) + ReLU over an (M, C) view: batch mean / 1/sqrt(biased
 * var + eps) to mean_dev / invstd_dev, running stats updated in place (unbiased var), y = relu(bn(z)) with pitch ld_y. */
int mgu_bn_relu_train_nhwc(mgu_ctx* ctx, const void* z_dev, const void* gamma_dev, const void* beta_dev, int64_t M, int C, void* y_dev,
                           int ld_y, void* mean_dev, void* invstd_dev, void* run_mean_dev, void* run_var_dev, void* hip_stream);
/* ... and its backward: dy (M, ld_dy) -> dz (M, C) dense, dgamma, dbeta (C), dbias = column sums of dz (the conv bias in front
 * of the BatchNorm: analytically 0).  The ReLU mask is recomputed from z. */
int mgu_bn_relu_backward_nhwc(mgu_ctx* ctx, const void* dy_dev, int ld_dy, const void* z_dev, const void* gamma_dev, const void* beta_dev,
                              const void* mean_dev, const void* invstd_dev, int64_t M, int C, void* dz_dev, void* dgamma_dev,
                              void* dbeta_dev, void* dbias_dev, void* hip_stream);
/* ---- train-step building blocks: half a ConvBlock (unet_encoder.py:7-25) exactly as the training step runs it -- the functions
 *      mgu_unet_forward(training=1) / mgu_unet_backward call per layer, on caller-provided tensors ----------------------------------
 * Conv2d(k=3, pad=1, bias) -> BatchNorm2d(train: eps 1e-5, momentum 0.1) -> ReLU [-> MaxPool2d(2)].  in: (B,H,W,ld_in) NHWC, ld_in % 4 ==
 * 0, channels [Cin, ld_in) zero; w (Cout,Cin,3,3); Cout % 4 == 0.  Writes z = conv + bias (B,H,W,Cout) dense, y = relu(bn(z)) with
 * pitch ld_y, pooled_dev (B,H/2,W/2,Cout) dense unless NULL, the batch mean / 1/sqrt(biased var + eps), and updates run_mean / run_var
 * in place (unbiased variance).  *stats_fused_out (may be NULL): 1 if the batch statistics were accumulated by the convolution's
 * epilogue, 0 if by a pass over z; *pool_fused_out: 1 if the pooled tensor was written by the BatchNorm apply pass (even H and W), 0 if
 * by the pool kernel (or not at all). */
int mgu_conv_bn_relu_train_nhwc(mgu_ctx* ctx, const void* in_dev, int ld_in, int B, int H, int W, int Cin, const void* w_oihw_dev,
                                const void* bias_dev, const void* gamma_dev, const void* beta_dev, int Cout, void* z_dev, void* y_dev,
                                int ld_y, void* pooled_dev, void* mean_dev, void* invstd_dev, void* run_mean_dev, void* run_var_dev,
                                int* stats_fused_out, int* pool_fused_out, void* hip_stream);
/* ... and its backward: BatchNorm + ReLU backward (dy (B,H,W,ld_dy) -> dz (B,H,W,Cout) dense, dgamma, dbeta; the ReLU mask is recomputed
 * from z), the weight gradient dw (Cout,Cin,3,3), whose unpack launch also folds the column sums of dz into dbias (analytically 0), and
 * -- din_dev != NULL -- the data gradient din (B,H,W,ld_din >= Cin).  in / z / mean / invstd: the forward's tensors. */
int mgu_bn_relu_conv_backward_nhwc(mgu_ctx* ctx, const void* in_dev, int ld_in, const void* z_dev, const void* dy_dev, int ld_dy,
                                   const void* gamma_dev, const void* beta_dev, const void* mean_dev, const void* invstd_dev,
                                   const void* w_oihw_dev, int B, int H, int W, int Cin, int Cout, void* dz_dev, void* dgamma_dev,
                                   void* dbeta_dev, void* dbias_dev, void* dw_oihw_dev, void* din_dev, int ld_din, void* hip_stream);
/* Test hook: synchronises hip_stream and writes the largest |value| in the ctx's per-channel reduction slots to *absmax_out (host).
 * Every reduction clears the rows it folded, so between calls of this ABI the answer is 0 (0 also before the first reduction). */
int mgu_reduction_slots_absmax(mgu_ctx* ctx, double* absmax_out, void* hip_stream);
/* MaxPool2d(2,2) backward ACCUMULATED into dskip (the skip tensor also receives the decoder-side gradient): y (B,H,W,ld_y) the
 * pooled tensor's input, dpool (B,H/2,W/2,C) dense, dskip (B,H,W,ld_d) += routed gradient (first maximum wins, as aten). */
int mgu_maxpool2x2_backward_nhwc(mgu_ctx* ctx, const void* y_dev, int ld_y, const void* dpool_dev, void* dskip_dev, int ld_d, int B, int H,
                                 int W, int C, void* hip_stream);

/* torch.optim.Adam.step() with L2 weight decay folded into the gradient (train_segmentation.py:96):
 * g = grad_scale*grad + wd*p; m,v moments; p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps).  step t >= 1.
 * grad_scale lets the caller fold the 1/world_size of an all-reduce SUM into the update.  The betas are doubles, as torch keeps them:
 * 1 - beta and 1 - beta^t are formed in double on the host and cast once (a beta2 rounded to fp32 puts both 1.3e-5 off). */
int mgu_adam_step(mgu_ctx* ctx, void* flat_param_dev, const void* flat_grad_dev, void* exp_avg_dev, void* exp_avg_sq_dev,
                  int64_t n, float lr, double beta1, double beta2, float eps, float weight_decay, int step,
                  float grad_scale, void* hip_stream);

/* torch.optim.SGD(lr, momentum, weight_decay).step() on the flat buffers -- the other optimizer branch of the reference's train loop
 * (scripts/train_segmentation.py:97-98, selected by configs/training.yaml:5-6; dampening 0, no Nesterov): g = grad_scale*grad + wd*p;
 * momentum != 0: buf = (step == 1 ? g : momentum*buf + g), p -= lr*buf; momentum == 0: p -= lr*g (momentum_buf_dev may be NULL). */
int mgu_sgd_step(mgu_ctx* ctx, void* flat_param_dev, const void* flat_grad_dev, void* momentum_buf_dev, int64_t n, float lr,
                 float momentum, float weight_decay, int step, float grad_scale, void* hip_stream);

/* ---- the optimizer step with its decisions on the device: AdamW, norm clipping, skip of a non-finite step, weight EMA,
 *      gradient accumulation (csrc/optim.hip).  mgu_adam_step / mgu_sgd_step above stay what they are. ----
 * All buffers are flat fp32 vectors of n elements on the device; a pointer needs 4-byte alignment only (16-byte accesses are used
 * where the buffers of a call share their offset within 16 bytes, with a peeled head and tail).
 *
 * The control record `ctrl`: 64 bytes on the device, 8-byte aligned, owned by the caller.  A zeroed record is a fresh optimizer.
 *   offset  0  int64   step       steps applied so far (the t of the bias corrections; a skipped step does not advance it)
 *           8  int64   skipped    steps skipped because the gradient held an inf or a NaN
 *          16  double  sumsq      sum of the squares of the gradient's elements (unscaled), of the last call
 *          24  double  norm       |grad_scale| * sqrt(sumsq): the L2 norm of the scaled gradient
 *          32  float   scale      grad_scale * coef, the factor the update kernel puts on every gradient element
 *          36  float   bc1        1 - beta1^step
 *          40  float   bc2_sqrt   sqrt(1 - beta2^step)
 *          44  float   ema_d      the EMA decay of this step
 *          48  int32   apply      1: the update kernel runs; 0: every workgroup of it returns
 *          52  int32   nonfinite  elements of the gradient that are inf or NaN
 *          56  8 bytes reserved (left as they are)
 * mgu_grad_norm and mgu_optim_step write the record with plain stores from one workgroup; nothing reads it on the host. */
#define MGU_OPTIM_CTRL_BYTES 64
#define MGU_OPTIM_ADAM 0  /* torch.optim.Adam: L2 decay folded into the gradient */
#define MGU_OPTIM_ADAMW 1 /* torch.optim.AdamW: decoupled decay, p *= 1 - lr * wd before the step */
#define MGU_OPTIM_SGD 2   /* torch.optim.SGD(momentum, weight_decay), dampening 0, no Nesterov */
typedef struct {
  int kind;                /* MGU_OPTIM_* */
  float lr;
  double beta1, beta2;     /* doubles, as mgu_adam_step takes them */
  float eps, weight_decay;
  float momentum;          /* kind 2; the momentum buffer is exp_avg_dev (exp_avg_sq_dev may be NULL) */
  float grad_scale;        /* factor on the gradient (1 / (world * accumulated steps)) */
  float max_norm;          /* > 0: clip the scaled gradient to this L2 norm; 0: off */
  int skip_nonfinite;      /* != 0: a gradient with an inf or a NaN leaves everything but ctrl->skipped as it is */
  float ema_decay;         /* in [0, 1); 0: off, ema_dev may then be NULL */
  int ema_warmup;          /* != 0: the decay of step t is min(ema_decay, (1 + t) / (10 + t)) */
} mgu_optim_desc;
/* Workgroups the partial-sums launch of mgu_grad_norm / mgu_optim_step runs for n elements, and the elements each of them owns:
 * workgroup b sums [b * chunk, min(n, (b + 1) * chunk)).  Both depend on n alone (host routines; n < 1: 0). */
int64_t mgu_grad_norm_chunk(int64_t n);
int mgu_grad_norm_blocks(int64_t n);
/* sumsq, norm and nonfinite of ctrl from the gradient; the other fields keep their contents.  Two launches: per workgroup the
 * sum of (double)g * (double)g over its chunk -- a fixed element -> lane assignment whatever the pointer's alignment, a fixed tree
 * over lanes, waves and the workgroup -- and the count of non-finite elements, written to context scratch; then one workgroup adds
 * the partial sums in index order in double.  No atomics: two calls on the same bytes give the same bits. */
int mgu_grad_norm(mgu_ctx* ctx, const void* grad_dev, int64_t n, float grad_scale, void* ctrl_dev, void* hip_stream);
/* One optimizer step in exactly three launches whatever n and the options: the two of mgu_grad_norm, whose second also decides
 *   coef  = max_norm > 0 ? min(1, max_norm / (norm + 1e-6)) : 1     (torch.nn.utils.clip_grad_norm_ on the scaled gradient; double)
 *   scale = (float)(grad_scale * coef)
 *   skip_nonfinite && nonfinite > 0:  apply = 0, skipped += 1;   else  apply = 1, step += 1
 *   bc1 = 1 - beta1^step, bc2_sqrt = sqrt(1 - beta2^step)            (double, cast once; from the record's step)
 *   ema_d = ema_warmup ? min(ema_decay, (1 + step) / (10 + step)) : ema_decay
 * and the update kernel, per element with g' = scale * g:
 *   kind 0  g' += wd * p;  m, v moments;  p -= lr / bc1 * m / (sqrt(v) / bc2_sqrt + eps)          (as mgu_adam_step)
 *   kind 1  p *= 1 - lr * wd;  the same moments and step on g' alone                               (torch.optim.AdamW)
 *   kind 2  g' += wd * p;  momentum != 0: buf = step == 1 ? g' : momentum * buf + g', p -= lr * buf;  else p -= lr * g'
 *   ema_decay > 0:  ema = ema_d * ema + (1 - ema_d) * p_new
 * With apply == 0 param, exp_avg, exp_avg_sq and ema keep their bits.  exp_avg_dev: Adam's first moment / SGD's momentum buffer
 * (NULL allowed for kind 2 with momentum 0); exp_avg_sq_dev: NULL allowed for kind 2. */
int mgu_optim_step(mgu_ctx* ctx, const mgu_optim_desc* desc, void* flat_param_dev, const void* flat_grad_dev, void* exp_avg_dev,
                   void* exp_avg_sq_dev, void* ema_dev, void* ctrl_dev, int64_t n, void* hip_stream);
/* acc = first ? grad : acc + grad (fp32, one launch). */
int mgu_grad_accumulate(mgu_ctx* ctx, void* acc_dev, const void* grad_dev, int64_t n, int first, void* hip_stream);

/* ---- gradient exchange of the data-parallel train step: RCCL over xGMI (the reference is single-process and has no
 *      collective; BASELINE configs[4] adds exactly this one, SURVEY sections 5 / 8b / 8e) -------------------------------
 * librccl is bound at run time inside libmgunet.so.  The host only moves 128 bytes: rank 0 calls mgu_comm_get_unique_id,
 * hands the bytes to every rank through its launcher's store, and each rank calls mgu_comm_init_rank on its own ctx
 * (= ncclCommInitRank on the ctx's device).  The communicator belongs to the ctx (freed by mgu_comm_destroy /
 * mgu_destroy). */
#define MGU_COMM_ID_BYTES 128
int mgu_comm_get_unique_id(void* id_out /* host, MGU_COMM_ID_BYTES */);
int mgu_comm_init_rank(mgu_ctx* ctx, const void* id /* host, MGU_COMM_ID_BYTES */, int rank, int world_size);
int mgu_comm_destroy(mgu_ctx* ctx);
void* mgu_comm_handle(mgu_ctx* ctx);     /* the ncclComm_t of this ctx, or NULL */
int mgu_comm_world_size(mgu_ctx* ctx);   /* 1 without a communicator */
/* In-place MEAN over the ranks of flat_grad_dev (n fp32, device) on hip_stream: one ncclAllReduce(ncclAvg).
 * rccl_comm: an ncclComm_t of the caller, or NULL for the ctx's own communicator. */
int mgu_allreduce_grads(mgu_ctx* ctx, void* flat_grad_dev, int64_t n, void* rccl_comm, void* hip_stream);
/* mgu_unet_backward + the gradient exchange, overlapped: the flat gradient is mean-all-reduced in buckets (>= 4 MB, in
 * the order backward finishes them: decoder first, encoder last) on the ctx's own communicator stream while the remaining
 * layers are still being differentiated; when the call returns, work enqueued on hip_stream afterwards (mgu_adam_step)
 * sees the averaged gradient.  Needs mgu_comm_init_rank. */
int mgu_unet_backward_allreduce(mgu_ctx* ctx, const void* dlogits_dev, void* flat_grad_dev, void* hip_stream);

/* One-shot request: the NEXT mgu_unet_forward on this ctx also writes the per-patch means of the shallowest decoder
 * feature -- exactly what mgu_patch_mean(decoder_feats[0], ...) returns, (B*nph*npw, init_features) fp32 -- to out_dev.
 * In eval mode with <= 4 classes the means and the final 1x1 conv share ONE pass over the feature map (it is read once
 * instead of twice: both consumers are bandwidth bound).  The node features of the 'full forward' (SURVEY 8a row L3).
 * out_dev == NULL cancels a pending request (e.g. after a forward that failed validation). */
int mgu_unet_request_patch_mean(mgu_ctx* ctx, int patch, void* out_dev);

/* ---- patch graph: replaces preprocessing/graph_construction/patch_graph_construction.py:49-102 -- */
/* ---- GAT training (the reference puts the graph branch's parameters in the optimizer, scripts/train_end_to_end.py:219-226, and
 * differentiates through GraphAttentionLayer.forward with loss.backward(), :478; eval-mode dropout here, train-mode below) ----------
 * DEVICE: transpose of a CSR-by-target: rowptr_src (N+1) / eid_src (E) list, per SOURCE node and in target-CSR order, the positions
 * of its out-edges in col[]; tgt_of_edge (E) is the target row of every edge.  Stable radix sort: every sum of the backward has a
 * fixed order.  Static per graph: build once, reuse for every step. */
int mgu_csr_transpose_device(mgu_ctx* ctx, const int32_t* rowptr_dev, const int32_t* col_dev, int64_t E, int num_nodes,
                             int32_t* rowptr_src_dev, int32_t* eid_src_dev, int32_t* tgt_of_edge_dev, void* hip_stream);
/* Backward of mgu_gat_layer_forward (same arguments; the forward's intermediates are recomputed from X, W, a): given dout
 * (N, heads*Fout_head if concat else Fout_head) writes dW (heads*Fout_head, Fin), da (heads, 2*Fout_head) and, if dX_dev is not
 * NULL, dX (N, Fin).  Includes the gradient through the graph-wide max of graph_attention.py:86 (torch.max()'s backward: to the
 * arg-max edge, evenly over ties).  heads*Fout_head <= 256. */
int mgu_gat_layer_backward(mgu_ctx* ctx, const void* X_dev, int N, int Fin, const int32_t* rowptr_dev, const int32_t* col_dev, int64_t E,
                           const int32_t* rowptr_src_dev, const int32_t* eid_src_dev, const int32_t* tgt_of_edge_dev,
                           const int32_t* graph_ptr_dev, int num_graphs, const void* W_dev, const void* a_dev, int heads, int Fout_head,
                           int concat, float alpha, const void* dout_dev, void* dX_dev, void* dW_dev, void* da_dev, void* hip_stream);
/* ---- GAT in TRAIN mode with dropout (model/gat/graph_attention.py:97: nn.Dropout on every head's attention coefficients; :160:
 * nn.Dropout on the layer output; default p = 0.1, configs/model.yaml:18).  The random draw is an explicit MASK (0 or 1 / (1 - p)):
 *   edge_mask (E, heads) fp32 in the CSR-by-target edge order of col[] (head h's mask of edge k at [k * heads + h]); NULL = none
 *   out_mask  (N, heads*Fout_head if concat else Fout_head) fp32; NULL = none
 * so that the same draw can be fed to the reference (a patched nn.Dropout: tests/golden/gat_dropout.npz).  mgu_dropout_mask fills a
 * mask from the library's own counter-based generator (Philox-4x32-10: element i of stream `stream` under `seed` depends on
 * (seed, stream, i) only).  Forward: one GEMM [Wh | s | t], the per-graph max, then one wavefront per target row; the backward is
 * mgu_gat_layer_backward with the masks applied where the forward applies them.  heads*Fout_head <= 256. */
int mgu_dropout_mask(mgu_ctx* ctx, unsigned long long seed, unsigned long long stream, int64_t n, float p, void* mask_dev, void* hip_stream);
int mgu_gat_layer_forward_train(mgu_ctx* ctx, const void* X_dev, int N, int Fin, const int32_t* rowptr_dev, const int32_t* col_dev, int64_t E,
                                const int32_t* graph_ptr_dev, int num_graphs, const void* W_dev, const void* a_dev, int heads, int Fout_head,
                                int concat, float alpha, const void* edge_mask_dev, const void* out_mask_dev, void* out_dev, void* hip_stream);
int mgu_gat_layer_backward_train(mgu_ctx* ctx, const void* X_dev, int N, int Fin, const int32_t* rowptr_dev, const int32_t* col_dev, int64_t E,
                                 const int32_t* rowptr_src_dev, const int32_t* eid_src_dev, const int32_t* tgt_of_edge_dev,
                                 const int32_t* graph_ptr_dev, int num_graphs, const void* W_dev, const void* a_dev, int heads, int Fout_head,
                                 int concat, float alpha, const void* edge_mask_dev, const void* out_mask_dev, const void* dout_dev,
                                 void* dX_dev, void* dW_dev, void* da_dev, void* hip_stream);

/* HOST routine (index maps are tiny and static per image size).  Emits the COO edge_index in the
 * reference's exact order (:77-92) into coo[0..E) (sources) and coo[E..2E) (targets), and the
 * CSR-by-target (rowptr[N+1], col[E]) that keeps each target's sources in COO order.  Any output
 * pointer may be NULL.  *E_out = 2*(nph*(npw-1)+(nph-1)*npw); nodes = nph*npw with ceil-div grid. */
int mgu_patch_graph_build(int H, int W, int patch, int64_t* coo, int32_t* rowptr, int32_t* col,
                          int64_t* E_out, int* nph_out, int* npw_out);
/* HOST: stable COO(2,E int64) -> CSR-by-target for an arbitrary graph (order[k] = COO position). */
int mgu_coo_to_csr(const int64_t* coo, int64_t E, int num_nodes, int32_t* rowptr, int32_t* col);
/* DEVICE: the same for a graph that already lives in device memory (the reference's forward takes any (2, E) int64 edge_index,
 * model/gat/graph_attention.py:40-58): stable sort by target, so each target's sources keep their COO order.  *status_dev (device
 * int) becomes non-zero if an id lies outside [0, num_nodes) -- torch's indexing raises IndexError there; the caller decides when
 * to look at it (one synchronisation per NEW graph, none per forward).  E < 2^31. */
int mgu_coo_to_csr_device(mgu_ctx* ctx, const int64_t* coo_dev, int64_t E, int num_nodes, int32_t* rowptr_dev, int32_t* col_dev,
                          int* status_dev, void* hip_stream);
/* Node features of the 'full forward' (SURVEY 8a row L3): mean over each patch x patch window of an
 * NHWC feature map, zero padded bottom/right as image_to_patches does (:26-47).
 * out_dev: (B*nph*npw, C) fp32. */
int mgu_patch_mean(mgu_ctx* ctx, const void* feat_dev, int feat_dtype /* MGU_DTYPE_* */, int B, int H, int W, int C,
                   int patch, void* out_dev, void* hip_stream);

/* ---- GAT: replaces model/gat/graph_attention.py:40-118, 150-160 (one MultiHeadGATLayer, eval) -- */
/* X_dev (N,Fin) fp32, Fin % 4 == 0; CSR by target on device (rowptr int32[N+1], col int32[E]);
 * W_dev (heads*Fout_head, Fin) = the heads' W.weight stacked; a_dev (heads, 2*Fout_head) = a.weight
 * stacked.  graph_ptr_dev int32[num_graphs+1] gives the node range of each graph of a block-diagonal
 * batch (the reference's exp(e - max(e)) at :86 is per graph and per head); NULL = one graph.
 * concat=1: out (N, heads*Fout_head) = cat of ELU(head) (:155); concat=0: out (N,Fout_head) = mean (:158). */
int mgu_gat_layer_forward(mgu_ctx* ctx, const void* X_dev, int N, int Fin,
                          const int32_t* rowptr_dev, const int32_t* col_dev, int64_t E,
                          const int32_t* graph_ptr_dev, int num_graphs,
                          const void* W_dev, const void* a_dev, int heads, int Fout_head,
                          int concat, float alpha, void* out_dev, void* hip_stream);

/* Steady-state form: the weight-only preparation (W^T a rows, MFMA-fragment-order W^T or the GEMM panel) runs once per weight
 * version, and a layer call is 2 launches when Fin <= Fout_head (st + per-graph max, then gather + aggregate + linear + ELU) or 3
 * otherwise (GEMM [Wh | s | t], per-graph max, row gather).  has_edges: whether the graphs the handle will be used on have edges
 * (a graph without edges -- e.g. a one-node region graph -- takes the gather schedule, whose rows come out exactly 0). */
typedef struct mgu_gat_weights mgu_gat_weights;
int mgu_gat_prepare(mgu_ctx* ctx, const void* W_dev, const void* a_dev, int heads, int Fout_head, int Fin, int has_edges,
                    mgu_gat_weights** out, void* hip_stream);
void mgu_gat_release(mgu_ctx* ctx, mgu_gat_weights* w);
int mgu_gat_layer_forward_prepared(mgu_ctx* ctx, const mgu_gat_weights* w, const void* X_dev, int N, const int32_t* rowptr_dev,
                                   const int32_t* col_dev, int64_t E, const int32_t* graph_ptr_dev, int num_graphs, int concat,
                                   float alpha, void* out_dev, void* hip_stream);

/* ---- MinCut stage of the patch-graph branch: replaces
 *      model/graph_partition/mincut_refinement.py:30-52 (edge weights), :55-160 (normalized-cut loss), :188-205
 *      (softmax of the segment logits + loss), scripts/train_end_to_end.py:356 (hard labels) ---------------------- */
/* w[e] = exp(-|f_src - f_tgt|^2 / 2) for the reference's COO int64 (2,E) edge list (row 0 sources, row 1 targets),
 * in edge order (MinCutRefinement.compute_edge_weights_for_ncut). */
int mgu_ncut_edge_weights(mgu_ctx* ctx, const float* feats_dev, int N, int D, const int64_t* edge_index_dev, int64_t E,
                          float* w_dev, void* hip_stream);
/* loss = sum_k cut_k / assoc_k (segments with assoc_k <= 1e-8 skipped), feats (N,D) fp32, CSR BY SOURCE
 * (rowptr int32[N+1], col int32[E] = targets: the reference sums the degree over the source index, :96).
 * assign_dev (N,K): segment logits (assign_is_logits = 1: softmax over K written to soft_dev, first-arg-max labels to
 * hard_dev if not NULL -- MinCutRefinement.forward) or soft assignments (0: normalized_cut_loss called directly;
 * soft_dev / hard_dev unused).  1 <= K <= 16.  loss_dev: one float. */
int mgu_ncut_forward(mgu_ctx* ctx, const float* feats_dev, int N, int D, const int32_t* rowptr_src_dev,
                     const int32_t* col_tgt_dev, int64_t E, const float* assign_dev, int K, int assign_is_logits,
                     float* soft_dev, int32_t* hard_dev, float* loss_dev, void* hip_stream);
/* loss.backward() through that loss (scripts/train_end_to_end.py:348-356 with :472-479; the reference differentiates through
 * the edge weights as well, mincut_refinement.py:79).  soft_dev (N,K): the assignments the forward used (its soft_dev, or its
 * assign_dev when that already held probabilities); CSR BY SOURCE as in the forward plus CSR BY TARGET (rowptr_tgt, col = sources:
 * mgu_coo_to_csr_device of the unflipped list, or mgu_csr_transpose_device).  gloss_dev: upstream gradient of the loss (one
 * float, NULL = 1); gsoft_dev (N,K) or NULL: upstream gradient of the returned soft assignments (logits only).  Writes
 * dassign_dev (N,K) -- w.r.t. the logits when assign_is_logits, else w.r.t. the probabilities -- and dfeats_dev (N,D) (may be
 * NULL).  Every element is written; both are gathers (no atomics: bitwise reproducible).  D <= 1024, 1 <= K <= 16. */
int mgu_ncut_backward(mgu_ctx* ctx, const float* feats_dev, int N, int D, const int32_t* rowptr_src_dev, const int32_t* col_tgt_dev,
                      const int32_t* rowptr_tgt_dev, const int32_t* col_src_dev, int64_t E, const float* soft_dev, int K,
                      int assign_is_logits, const float* gloss_dev, const float* gsoft_dev, float* dassign_dev, float* dfeats_dev,
                      void* hip_stream);
/* dz[i] = y[i] > 0 ? dy[i] : 0 -- the ReLU of the MLP segment predictor (scripts/train_end_to_end.py:59-63) in its backward. */
int mgu_relu_backward(mgu_ctx* ctx, const float* dy_dev, const float* y_dev, int64_t n, float* dz_dev, void* hip_stream);

/* ---- Region stage + fusion of the e2e forward: replaces scripts/train_end_to_end.py:366-373
 *      (label-mean pooling), :403-421 (region embedding -> patches -> nearest upsample) and the concat of
 *      FeatureFusion.forward (model/fusion_detection/feature_fusion.py:78,145-150) ------------------------------------ */
/* out (B*K, D)[b*K + k] = mean of feats (B*Np, D) rows of image b whose hard label is k; zeros for an empty segment.
 * D % 4 == 0, D <= 1024. */
int mgu_region_mean_pool(mgu_ctx* ctx, const float* feats_dev, const int32_t* hard_dev, int B, int Np, int D, int K,
                         float* out_dev, void* hip_stream);
/* out NHWC (B,H,W,Cu+D): channels [0,Cu) = fu_nhwc (B,H,W,Cu) (Cu may be 0), channels [Cu,Cu+D) = the region embedding
 * (B*K, D) of the segment of the patch the pixel maps to under torch's 'nearest' interpolation of the (nph, npw) grid
 * to (H, W): label = hard[b][min(floor(y*nph/H), nph-1)][min(floor(x*npw/W), npw-1)].  Cu, D multiples of 4. */
int mgu_region_fuse_nhwc(mgu_ctx* ctx, const float* fu_nhwc_dev, int Cu, const float* region_emb_dev, const int32_t* hard_dev,
                         int B, int H, int W, int nph, int npw, int K, int D, float* out_nhwc_dev, void* hip_stream);

/* ---- auxiliary losses of the training loops: forward values, one device float each ---------------------------
 * Streaming reductions in double precision with a fixed summation order (bitwise reproducible); every tensor is addressed by
 * ELEMENT strides so NCHW and NHWC storage both work without a copy. */
/* TVLoss.forward (scripts/train_end_to_end.py:73-89): weight * (sum (x[y+1]-x[y])^2 / ((H-1) W) + sum (x[x+1]-x[x])^2 / (H (W-1))) / B
 * over x (B,C,H,W), element (n,c,y,x) at x_dev[n*xs_n + c*xs_c + y*xs_h + x*xs_w]. */
int mgu_tv_loss(mgu_ctx* ctx, const void* x_dev, int B, int C, int H, int W, int64_t xs_n, int64_t xs_c, int64_t xs_h, int64_t xs_w,
                float weight, float* loss_dev, void* hip_stream);
/* dice_loss (scripts/train_segmentation.py:29-40): softmax over the classes, one-hot target, Dice with additive smoothing per
 * (image, class), 1 - mean.  logits element (b, c, pixel p) at logits_dev[b*ls_n + c*ls_c + p*ls_p]; labels int64 (B, HW);
 * num_classes <= 8.  A label outside [0, num_classes) (F.one_hot raises) is reported like mgu_cross_entropy's. */
int mgu_dice_loss(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                  int64_t ls_c, int64_t ls_p, float smooth, float* loss_dev, void* hip_stream);
/* FeatureConsistencyLoss.forward (model/unet/feature_loss.py:88-125), the (B, N, D) / (B, N) form: f_unet, f_graph (B,N,D) fp32
 * contiguous, y (B,N) fp32 (the reference casts y.float()): mean_b sum_n [ y d^2 + (1-y) relu(margin - sqrt(d^2 + 1e-8))^2 ]. */
int mgu_feature_consistency_loss(mgu_ctx* ctx, const void* f_unet_dev, const void* f_graph_dev, const void* y_dev, int B, int N, int D,
                                 float margin, float* loss_dev, void* hip_stream);
/* ---- gradients of the differentiable auxiliary losses ---------------------------------------------------------------------------
 * The reference obtains them from autograd (loss.backward(): scripts/train_segmentation.py:133, scripts/train_end_to_end.py:478).
 * Each entry multiplies the gradient of the scalar loss by grad_scale and, when grad_scale_dev is not NULL, by that device float
 * too (an autograd grad_output never has to visit the host).  EllipticalShapeLoss has no gradient w.r.t. its input: it is a
 * function of the arg-max pixel COORDINATES (shape_loss.py:61-98) -- and the reference loop pins loss_shape to 0 (:287). */
/* d TVLoss / dx into dx_dev, element (n,c,y,x) at dx_dev[n*ds_n + c*ds_c + y*ds_h + x*ds_w]. */
int mgu_tv_loss_backward(mgu_ctx* ctx, const void* x_dev, int B, int C, int H, int W, int64_t xs_n, int64_t xs_c, int64_t xs_h,
                         int64_t xs_w, float weight, float grad_scale, const float* grad_scale_dev, void* dx_dev, int64_t ds_n,
                         int64_t ds_c, int64_t ds_h, int64_t ds_w, void* hip_stream);
/* d dice_loss / d logits (through the softmax), element (b, c, p) at dlogits_dev[b*ds_n + c*ds_c + p*ds_p]; accumulate != 0 ADDS to
 * what is there -- the trainer's `loss_ce + loss_dice` (scripts/train_segmentation.py:126-133) is mgu_cross_entropy followed by this
 * call on the same dlogits.  loss_dev (optional) receives the loss value of the same pass. */
int mgu_dice_loss_backward(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                           int64_t ls_n, int64_t ls_c, int64_t ls_p, float smooth, float grad_scale, const float* grad_scale_dev,
                           void* dlogits_dev, int64_t ds_n, int64_t ds_c, int64_t ds_p, int accumulate, float* loss_dev, void* hip_stream);
/* d FeatureConsistencyLoss / d f_unet and / d f_graph ((B,N,D) contiguous each; either may be NULL). */
int mgu_feature_consistency_loss_backward(mgu_ctx* ctx, const void* f_unet_dev, const void* f_graph_dev, const void* y_dev, int B, int N,
                                          int D, float margin, float grad_scale, const float* grad_scale_dev, void* d_f_unet_dev,
                                          void* d_f_graph_dev, void* hip_stream);
/* Synchronise the stream and report (MGU_ERR_INVALID) a label outside [0, num_classes) met by mgu_dice_loss[_backward] on this
 * context since the last check: the place F.one_hot would have raised. */
int mgu_loss_sync_check(mgu_ctx* ctx, void* hip_stream);
/* Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018; the build's own addition), the convex
 * surrogate of 1 - IoU.  logits / labels / strides as mgu_dice_loss, num_classes <= 8.  A segment is one class over the batch
 * (per_image 0) or one (image, class) pair (per_image 1); a pixel labelled ignore_index belongs to none (no rank, no term, zero
 * gradient); any other label outside [0, num_classes) is flagged as mgu_dice_loss flags it (mgu_loss_sync_check) and the loss is
 * NaN.  Per segment the errors e = 1 - p[c] (label c) / p[c] (else), p the fp32 softmax, are ranked in DESCENDING order, equal fp32
 * errors in ascending pixel order (b, y, x): part of the interface.  With G the segment's foreground pixels, k the rank from 1 and
 * F_k the foreground pixels among ranks 1..k, U_k = G + k - F_k: g_k = 1 / U_k (foreground), (G - F_k) / (U_k (U_k - 1))
 * (background), G == 0: g_1 = 1, else 0 -- from the integer counts in double, rounded once.  Segment loss = sum_k e_(k) g_k in
 * double in a fixed order (bitwise reproducible); loss = mean over the counted segments (classes_mode 0 "present": G > 0 only;
 * 1 "all"), with per_image the mean over an image's counted classes, then over the B images (an image without one adds 0).
 * errors_dev fp32 / ranks_dev int32, each (num_classes, B*HW), optional test hooks: the errors and the 0-based rank inside the
 * segment (ignored pixel: error 0, rank -1).  Stream-ordered, no host synchronisation.
 * Launches: 16 for the value, 17 with the gradient (four sort passes of histogram + scan + scatter over 8 + 8 + 8 + 7 key bits,
 * foreground count, its scan, the closed forms, the finishing kernel, the per-pixel softmax backward), whatever num_classes,
 * per_image and B are.  Scratch (the context's, grown on first use): with P = B*HW, G = per_image ? B : 1 and
 * T = num_classes * G * ceil(P / G / mgu_lovasz_tile()) tiles: 16 * num_classes * P bytes of key / payload planes + 1024 * T
 * of digit counts + 12 * T + 1040 * num_classes * G, each of the eleven regions rounded up to 256 bytes (68 172 544 bytes = 65.0 MiB
 * at 8 x 512 x 512, 2 classes, over the batch).  num_classes > 8, an empty shape or B*HW >= 2^30 return MGU_ERR_INVALID and launch nothing. */
int mgu_lovasz_softmax(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                       int64_t ls_c, int64_t ls_p, int classes_mode, int per_image, int64_t ignore_index, float* loss_dev,
                       float* errors_dev, int32_t* ranks_dev, void* hip_stream);
/* d Lovasz-Softmax / d logits: dL/dp_i[c] = -+ g_rank / (counted segments of that mean [* B with per_image]) (foreground -,
 * background +), through the softmax, times grad_scale (* *grad_scale_dev if given); element (b, c, p) at
 * dlogits_dev[b*ds_n + c*ds_c + p*ds_p], accumulate != 0 ADDS (the trainer's "ce+lovasz": after mgu_cross_entropy on the same
 * dlogits).  loss_dev (optional) receives the loss value of the same pass. */
int mgu_lovasz_softmax_backward(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                                int64_t ls_n, int64_t ls_c, int64_t ls_p, int classes_mode, int per_image, int64_t ignore_index,
                                float grad_scale, const float* grad_scale_dev, void* dlogits_dev, int64_t ds_n, int64_t ds_c, int64_t ds_p,
                                int accumulate, float* loss_dev, void* hip_stream);
/* Keys one workgroup ranks per sort pass of the Lovasz kernels (the tests size their segments around it). */
int mgu_lovasz_tile(void);
/* Imbalance-aware pixel-wise cross-entropy (the build's own: INTEGRATION.md section S): class weights, label smoothing, the focal
 * term (Lin et al., ICCV 2017) and hard-pixel mining (bootstrapped cross-entropy, Wu et al. 2016; OHEM) in one loss.  Logits element
 * (b, c, p) at logits_dev[b*ls_n + c*ls_c + p*ls_p] (fp32, num_classes <= 8), labels (B, HW) int64.  A pixel labelled ignore_index is
 * not counted; any other label outside [0, num_classes) is never used as an index, makes the loss NaN and is flagged as mgu_dice_loss
 * flags it (mgu_loss_sync_check).  class_weight_dev: num_classes floats >= 0 on the device, NULL = ones.  Per counted pixel, lp the
 * fp32 log-softmax and p the softmax:
 *   focal_gamma == 0:  l = (1 - label_smoothing) w_y (-lp_y) + (label_smoothing / C) sum_c w_c (-lp_c)   [F.cross_entropy per pixel]
 *   focal_gamma >= 1:  l = w_y (1 - p_y)^focal_gamma (-lp_y), label_smoothing must be 0; 1 - p_y is formed without cancellation
 * clamped to >= +0.0f; its fp32 bits are the ranking key.  A group is the batch (per_image 0) or one image; with n its counted pixels
 * K = min(n, max(min_kept, ceil(keep_fraction * n))) (product and ceil in IEEE double) and KEPT are the K pixels of largest l, among
 * equal fp32 l the lower pixel index (b, y, x) first: part of the interface.  keep_fraction == 1 keeps every counted pixel (no select).
 *   loss = sum_kept l / sum_kept w_y    one numerator and one denominator over all groups, both in double in a fixed order (bitwise
 * reproducible); a denominator of 0 gives NaN.  Without mining and with focal_gamma 0 this is torch's mean reduction with weights.
 * pixel_loss_dev fp32 (B*HW) / kept_dev int32 (B*HW), optional test hooks: l (0 where not counted) and 1 kept / 0 dropped / -1 not
 * counted.  Stream-ordered, no host synchronisation, no host read of n or K.
 * Launches, whatever B, num_classes, per_image and the data are: keep_fraction == 1: 2 for the value, 3 with the gradient;
 * keep_fraction < 1: 8 / 9 (pixel losses + top digit counts, three counting passes over 8 + 8 + 8 + 7 key bits, tie counts, tie scan,
 * sums, finish, gradient rows) after one memset of the digit counters.  Scratch (the context's, grown on first use), P = B*HW,
 * G = per_image ? B : 1, T = G * ceil(P / G / mgu_pixel_ce_tile()): 16 * T + 16 bytes, with the select also 4 * P + 4096 * G + 4 * T
 * + 8 * G, every region rounded up to 256 bytes (8 403 456 bytes = 8.0 MiB at 8 x 512 x 512 over the batch).
 * num_classes > 8, an empty shape, B*HW >= 2^30, label_smoothing outside [0, 1), focal_gamma in (0, 1) or < 0, focal_gamma > 0 with
 * label_smoothing > 0, keep_fraction outside (0, 1] or min_kept < 0 return MGU_ERR_INVALID and launch nothing. */
int mgu_pixel_ce(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                 int64_t ls_c, int64_t ls_p, const float* class_weight_dev, float label_smoothing, float focal_gamma,
                 double keep_fraction, int64_t min_kept, int per_image, int64_t ignore_index, float* loss_dev, float* pixel_loss_dev,
                 int32_t* kept_dev, void* hip_stream);
/* d loss / d logits of exactly that expression with the kept set held fixed, times grad_scale (* *grad_scale_dev if given; no
 * npix / count rescaling as in mgu_cross_entropy: grad_scale 1 is L.backward()): element (b, c, p) at dlogits_dev[b*ds_n + c*ds_c +
 * p*ds_p].  Pixels that are not counted or not kept get exact zeros.  accumulate != 0 ADDS to dlogits_dev; with accumulate == 0 and
 * zero_to > num_classes the classes [num_classes, zero_to) of every pixel are written 0 at the same strides (the trainer's 4-padded
 * rows).  loss_dev (optional) receives the loss value of the same pass. */
int mgu_pixel_ce_backward(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                          int64_t ls_n, int64_t ls_c, int64_t ls_p, const float* class_weight_dev, float label_smoothing,
                          float focal_gamma, double keep_fraction, int64_t min_kept, int per_image, int64_t ignore_index,
                          float grad_scale, const float* grad_scale_dev, void* dlogits_dev, int64_t ds_n, int64_t ds_c, int64_t ds_p,
                          int accumulate, int zero_to, float* loss_dev, void* hip_stream);
/* The pixel cross-entropy with a per-pixel weight map m: the arguments of mgu_pixel_ce /
 * mgu_pixel_ce_backward plus pixel_weight_dev, fp32 (B, HW), dense, every entry >= 0 (mgu_border_weights' weight_dev is one).  The
 * pixel's loss becomes m(p) l(p), l exactly as above; that product, clamped to >= +0.0f, is the key the hard-pixel select ranks (the
 * tie rule is unchanged) and what pixel_loss_dev receives.
 *   loss = sum_kept m l / sum_kept m w_y
 * and the gradient is that of this expression with the kept set and m held fixed (m gets no gradient; a pixel with m == 0 gets a zero
 * row).  pixel_weight_dev == NULL, or a map of ones, gives the bits of mgu_pixel_ce / mgu_pixel_ce_backward.  The same kernels and
 * launch counts (2 / 3, with the select 8 / 9), reported in the profile as pixel_ce_map ...; the same limits and scratch. */
int mgu_pixel_ce_map(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes, int64_t ls_n,
                     int64_t ls_c, int64_t ls_p, const float* class_weight_dev, const float* pixel_weight_dev, float label_smoothing,
                     float focal_gamma, double keep_fraction, int64_t min_kept, int per_image, int64_t ignore_index, float* loss_dev,
                     float* pixel_loss_dev, int32_t* kept_dev, void* hip_stream);
int mgu_pixel_ce_map_backward(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                              int64_t ls_n, int64_t ls_c, int64_t ls_p, const float* class_weight_dev, const float* pixel_weight_dev,
                              float label_smoothing, float focal_gamma, double keep_fraction, int64_t min_kept, int per_image,
                              int64_t ignore_index, float grad_scale, const float* grad_scale_dev, void* dlogits_dev, int64_t ds_n,
                              int64_t ds_c, int64_t ds_p, int accumulate, int zero_to, float* loss_dev, void* hip_stream);
/* Keys one workgroup counts per pass of the pixel cross-entropy's select (the tests size their groups around it). */
int mgu_pixel_ce_tile(void);
/* EllipticalShapeLoss.forward (model/unet/shape_loss.py:17-180).  _masks: the object_masks_list form, all masks of the batch
 * stacked (num_objects, H, W) uint8 (non-zero = object pixel).  _probs: the form without masks -- per image, the pixels whose
 * arg-max class is 1 are ONE object (:61-98); probabilities (B,C,H,W) at probs_dev[b*ps_n + c*ps_c + p*ps_p].  Objects under 10
 * pixels are skipped; the loss is the mean over the processed objects of mean_pixels (p^T (cov + eps I)^-1 p - 1)^2, 0 if none. */
int mgu_elliptical_shape_loss_masks(mgu_ctx* ctx, const uint8_t* masks_dev, int num_objects, int H, int W, float epsilon, float* loss_dev,
                                    void* hip_stream);
int mgu_elliptical_shape_loss_probs(mgu_ctx* ctx, const void* probs_dev, int B, int num_classes, int H, int W, int64_t ps_n, int64_t ps_c,
                                    int64_t ps_p, float epsilon, float* loss_dev, void* hip_stream);

/* ---- segmentation evaluation: replaces the scoring loop of experiments/segmentation_performance.py:125-151 (forward -> argmax ->
 *      .view(-1).cpu() of predictions and masks -> experiments/metrics.py:6-69 segmentation_metrics, whose sklearn confusion matrix
 *      is the only data it needs) and the validation loss scripts/train_segmentation.py:145-151 leaves commented out ---------------
 * ONE read of logits (B,H,W,C) NHWC fp32 -- what mgu_unet_forward writes -- and int64 labels (B, HW): per pixel the first maximal
 * class (bit-identical to mgu_argmax_classes; = torch.argmax, :141, on finite input, ties included) and confusion_dev[y][pred] += 1
 * when 0 <= y < C -- sklearn's confusion_matrix(labels=range(C)) (metrics.py:21), which drops any other label.  confusion_dev: int64
 * (C, C), ACCUMULATED with integer atomics (exact, order-free: a whole test set adds up without a host synchronisation).
 * pred_dev: int64 (B, HW) predictions, NULL = not written.  loss_kind 0: counts only (no exp / log); 1: nn.CrossEntropyLoss()
 * (mean, ignore_index -100; an out-of-range label as mgu_cross_entropy: NaN loss + the ctx's data-error word); 2: that + dice_loss
 * (train_segmentation.py:29-40, smoothing dice_smooth; any label outside [0, C) flagged as mgu_dice_loss does; num_classes <= 8).
 * With a loss, loss_acc_dev (double[2]) is ACCUMULATED: [0] += (double)batch_loss (fp32 CE [+ fp32 dice], summed in fp32: :130),
 * [1] += 1 -- the reference's val_loss += loss.item() and its batch count; the partials are added in a fixed order (bitwise
 * reproducible).  mgu_loss_sync_check reports a flagged label.  loss_acc_dev must be NULL iff loss_kind == 0. */
int mgu_segmentation_eval(mgu_ctx* ctx, const void* logits_dev, const int64_t* labels_dev, int B, int64_t HW, int num_classes,
                          int64_t* confusion_dev, int64_t* pred_dev, int loss_kind, float dice_smooth, double* loss_acc_dev,
                          void* hip_stream);
/* Confusion counts of given predictions (segmentation_metrics takes two label tensors, metrics.py:6): confusion_dev[t][p] += 1 for
 * every i with t = true_dev[i], p = pred_dev[i] both in [0, num_classes); other pairs are dropped, as sklearn drops them.  int64
 * (num_classes, num_classes), accumulated. */
int mgu_confusion_matrix(mgu_ctx* ctx, const int64_t* true_dev, const int64_t* pred_dev, int64_t n, int num_classes,
                         int64_t* confusion_dev, void* hip_stream);

/* ---- object counting: the instance step model/unet/shape_loss.py:43-91 leaves commented out (skimage.measure.label(mask,
 *      connectivity=2, background=0)) and the object matching of experiments/metrics.py:160-253 yield_estimation_metrics -------------
 * Connected components of B images of H x W.  src_kind 0: int64 class map (B, H*W); 1: NHWC fp32 logits (B,H,W,C) -- what
 * mgu_unet_forward writes -- whose per-pixel class is the first maximal one (bit-identical to mgu_argmax_classes), computed in the
 * first pass (no class map is written).  Two pixels join when they are neighbours (connectivity 1: 4-neighbours, 2: 8-neighbours),
 * hold the same value and that value is foreground: != background and, when num_classes > 0, inside [0, num_classes) (so -100
 * ignore labels are background).  Images never join.  labels_dev: int32 (B,H,W), 0 = background, objects 1..n_b per image in raster
 * order of their first pixel (skimage.measure.label / scipy.ndimage.label numbering); deterministic.  Objects of fewer than
 * min_area pixels become background and the rest are renumbered 1..n'.  counts_dev: int64 (B) objects per image; offsets_dev:
 * int64 (B+1) exclusive prefix of counts (object k of image b has the batch-wide index offsets[b] + k - 1).  B*H*W < 2^31. */
int mgu_connected_components(mgu_ctx* ctx, const void* src_dev, int src_kind, int B, int H, int W, int C, int connectivity, int64_t background,
                             int64_t num_classes, int min_area, int32_t* labels_dev, int64_t* counts_dev, int64_t* offsets_dev,
                             void* hip_stream);
/* Per-object statistics of mgu_connected_components' labels (same src, src_kind, B, H, W, C; its offsets_dev), at batch-wide object
 * index i < capacity (objects past capacity are skipped): class_dev int64 (the pixels' value / argmax class), area_dev int64,
 * bbox_dev int32 (4): [xmin, ymin, xmax, ymax] with EXCLUSIVE max edges (w*h is the box area), sums_dev int64 (2): [sum x, sum y]
 * (centroid = sums / area).  Integer atomics: exact and order-free.  area_dev and sums_dev may be NULL. */
int mgu_object_stats(mgu_ctx* ctx, const int32_t* labels_dev, const void* src_dev, int src_kind, int B, int H, int W, int C,
                     const int64_t* offsets_dev, int64_t capacity, int64_t* class_dev, int64_t* area_dev, int32_t* bbox_dev, int64_t* sums_dev,
                     void* hip_stream);
/* The greedy matching of metrics.py:215-240, one workgroup per image: predictions in object order (every confidence 1.0), each
 * matched to the unused GT object of its class with the first strictly largest IoU (fp64 inter / (a1 + a2 - inter), 0.0 when they do
 * not overlap) if that IoU is > 0 and >= iou_thresh.  Objects as mgu_object_stats writes them (offsets, class, bbox; capacity = the
 * arrays' length; an image whose objects pass the capacity is skipped).  totals_dev int64 (3) ACCUMULATED: [GT objects, predicted
 * objects, matched GT objects]. */
int mgu_match_objects(mgu_ctx* ctx, int B, const int64_t* gt_offsets_dev, const int64_t* gt_class_dev, const int32_t* gt_bbox_dev,
                      int64_t gt_capacity, const int64_t* pred_offsets_dev, const int64_t* pred_class_dev, const int32_t* pred_bbox_dev,
                      int64_t pred_capacity, double iou_thresh, int64_t* totals_dev, void* hip_stream);
/* Per-object confidence: scores_dev[i] (fp32) = the mean over object i's pixels of probs[pixel][class_dev[i]], for the objects of
 * mgu_connected_components' labels_dev / offsets_dev and mgu_object_stats' class_dev / area_dev at batch-wide index i < capacity.
 * probs_dev: NHWC fp32 (B,H,W,C), values clamped to [0, 1]; an object whose class lies outside [0, C) scores 0.  Each pixel adds
 * round_half_even(p * 2^32) to a uint64 sum with integer atomics (exact and order-free: deterministic); the score is
 * (sum * 2^-32) / area in fp64, rounded to fp32.  B*H*W < 2^31. */
int mgu_object_scores(mgu_ctx* ctx, const int32_t* labels_dev, const float* probs_dev, int B, int H, int W, int C, const int64_t* offsets_dev,
                      int64_t capacity, const int64_t* class_dev, const int64_t* area_dev, float* scores_dev, void* hip_stream);

/* ---- splitting touching objects: exact distance transform, one seed per inscribed disc, power diagram of the discs -----------------
 * Two fruits whose masks touch are one connected component; this stage sits between "label" and "count".  All in exact integers (no
 * float anywhere), so the results are deterministic: bitwise repeatable whatever order the atomics land in.  It is not a flooding
 * watershed: cells are cut along radical axes, not along grey-level ridges.
 * labels_dev: int32 (B,H,W) as mgu_connected_components writes it, 0 = background; a "component" is the set of pixels of one image
 * holding the same non-zero label (it need not be connected).
 * Squared Euclidean distance transform.  d2_dev int32 (B,H,W): for a foreground pixel p the minimum of |p - q|^2 over the pixels q of
 * the same image with labels[q] != labels[p] -- background counts, a touching object with another label counts, pixels outside the
 * image do not (scipy.ndimage.distance_transform_edt of the label's mask); MGU_D2_NONE when the image holds no such q; 0 on
 * background.  Any int32 label map is legal here.  Two launches (columns, then rows with the row in LDS).  H, W <= 16384 (the row
 * buffer is 8 bytes of LDS per pixel, and every real distance stays below MGU_D2_NONE), B <= 65535, B*(H*W+1) < 2^31. */
#define MGU_D2_NONE (1 << 30)
int mgu_distance_transform(mgu_ctx* ctx, const int32_t* labels_dev, int B, int H, int W, int32_t* d2_dev, void* hip_stream);
/* Split every component at the necks between its inscribed discs (limits as above; labels outside [0, H*W] read as background).
 *   Seeds.  With r = min_distance (1..16), a foreground pixel p is a seed iff D2(p) >= min_radius_sq (>= 1) and D2(p) >= D2(q) for
 *     every q of p's label within Chebyshev distance r (pixels outside the image and other labels take no part).
 *   Seed groups.  h = (r + 1) / 2; the zone map Z(p) = labels[p] if a seed of p's label lies within Chebyshev distance h of p, else 0;
 *     the groups are the 8-connected same-value components of Z, and a seed belongs to the group that contains it.  Equal peaks of one
 *     component closer than about r are one object, peaks farther apart are two.
 *   Assignment.  A pixel p of a component with seeds goes to the group of the seed s of its component minimising |p - s|^2 - D2(s)
 *     (int64), ties to the smaller y*W + x of s: the power diagram of the inscribed discs, whose cell boundary between two
 *     overlapping discs is the chord through their intersection points.  A component without a seed (thinner than min_radius_sq)
 *     stays one object.
 *   Output.  labels_out_dev int32 (B,H,W) (may be labels_dev itself): the new objects 1..n'_b per image in raster order of their
 *     first pixel (a cell need not be connected); objects of fewer than min_area pixels become background and the rest are
 *     renumbered; counts_dev int64 (B), offsets_dev int64 (B+1) as mgu_connected_components writes them.  d2_out_dev int32 (B,H,W)
 *     and seeds_out_dev uint8 (B,H,W) (1 = seed) receive the distance transform and the seed mask; either may be NULL.
 * 16 kernel launches and 2 fills (3 with a min_area), whatever B, the objects and the seeds; no host synchronisation; scratch from
 * the context (about 45 bytes per pixel). */
int mgu_split_objects(mgu_ctx* ctx, const int32_t* labels_dev, int B, int H, int W, int min_distance, int64_t min_radius_sq, int min_area,
                      int32_t* labels_out_dev, int64_t* counts_dev, int64_t* offsets_dev, int32_t* d2_out_dev, uint8_t* seeds_out_dev,
                      void* hip_stream);

/* ---- border weight map: the per-pixel loss weight of the U-Net paper (Ronneberger et al., MICCAI 2015, eq. 2) ------------------------
 *   w(p) = w_c(p) + w0 exp(-(d1(p) + d2(p))^2 / (2 sigma^2))
 * d1, d2 the distances to the nearest and to the second-nearest object: the thin background gaps between two touching fruits get a
 * large weight in training (mgu_pixel_ce_map takes the map).  Built on the device from the masks of each step, no host synchronisation.
 * labels_dev: int32 (B,H,W), 0 = background, every other int32 value an object, compared by value (it need not be connected, ids need
 * not be dense): what mgu_connected_components / mgu_split_objects write, or a dataset's instance map.
 * For every pixel p (foreground or background) and every object label k present in p's image, D_k(p) = min |p - q|^2 over the pixels
 * q of that image with label k, an exact integer; pixels outside the image take no part.  The pairs (D_k(p), k) are ordered
 * lexicographically, k as a signed int32.  d1sq(p) = the distance of the first pair (0 on an object's own pixels), nearest(p) = its
 * label, d2sq(p) = the distance of the second pair: the nearest object other than nearest(p).  d1sq and d2sq do not depend on the tie
 * rule, nearest does: ties go to the smaller label.  MGU_D2_NONE where the image holds no object, for d2sq also where it holds fewer
 * than two; nearest is 0 where there is no object.
 * Outputs, each optional (NULL = not written): d1sq_dev, d2sq_dev, nearest_dev int32 (B,H,W); weight_dev fp32 (B,H,W),
 *   weight = class_weight[cls(p)] + w0 * exp(-(sqrt(d1sq) + sqrt(d2sq))^2 / (2 sigma^2))
 * evaluated in fp64 from the exact integers and rounded to fp32 once; the exponential term is exactly 0 where d2sq is MGU_D2_NONE.
 * cls(p) = classes_dev[p], an optional int64 (B,H,W) class map; a class outside [0, num_classes) (-100) gets class term 0; without
 * classes_dev or without class_weight_dev (fp32, num_classes entries) the class term is 1.  target_dev int64 (B,H,W): a copy of
 * classes_dev in which an object pixel with a 4-neighbour holding a different non-zero label is set to background_class -- the
 * one-pixel separation between touching instances the U-Net recipe assumes; it needs classes_dev.
 * Exactly two launches, whatever B, the objects and the outputs asked for (columns: a lane per column keeps the two nearest distinct
 * labels above and below every pixel; rows: a workgroup per row with the row's two candidates per column in LDS, every pixel walking
 * outward until dx^2 passes its d2sq); no host synchronisation; all outputs are pure functions of the input (no float atomics,
 * bitwise repeatable).  An image with fewer than two objects makes every pixel walk its whole row, O(W^2) per row.  Scratch: 16 bytes
 * per pixel of the context's.  Limits: H, W <= 16384 and 16 * W bytes of LDS within what the device gives one workgroup (W <= 10240
 * at 160 KiB), B <= 65535, B*H*W < 2^31; every real distance stays below MGU_D2_NONE.  sigma <= 0, w0 < 0, an empty shape,
 * target_dev without classes_dev, class weights with num_classes outside 1..8 or a size past the limits return MGU_ERR_INVALID
 * and launch nothing. */
int mgu_border_weights(mgu_ctx* ctx, const int32_t* labels_dev, int B, int H, int W, const int64_t* classes_dev, const float* class_weight_dev,
                       int num_classes, double w0, double sigma, int64_t background_class, int32_t* d1sq_dev, int32_t* d2sq_dev,
                       int32_t* nearest_dev, float* weight_dev, int64_t* target_dev, void* hip_stream);

/* ---- mask cleanup: close gaps, fill holes, open away spurs --------------------------------------------------------------------------
 * The stage between "argmax" and "label": a pin hole inside an object collapses its inscribed disc and mgu_split_objects then counts
 * the object several times.  Integer and bit arithmetic only: bitwise repeatable.
 * Input: src_dev / src_kind / C as mgu_connected_components takes them (0: int64 class map (B,H,W) with num_classes given; 1: NHWC
 * fp32 logits with the argmax fused, first maximal class, bit-identical to mgu_argmax_classes; num_classes is then C).  Foreground
 * classes are 1 .. num_classes-1 (2 <= num_classes <= 32); every other value (0, -100, out of range) reads as background, and
 * background is written as 0.  out_dev: int64 (B,H,W) class map; it must not overlap the input.  Images never interact.
 * A disc of squared radius r2 is D = {d in Z^2 : |d|^2 <= r2}, 0 <= r2 <= 64; r2 = 0 skips the stage.  Three stages, in this order:
 *   1. Close (close_radius_sq).  For each foreground class c, A_c = {m = c}, on an infinite plane whose pixels outside the image are
 *      background: Dil_c = A_c (+) D, Clo_c = {p inside the image : p + D inside Dil_c}.  A background pixel takes the smallest c
 *      with p in Clo_c; foreground pixels never change.
 *   2. Fill holes (fill_holes != 0).  The 4-connected components of the background of the stage-1 result (the complement of
 *      8-connected foreground, as scipy.ndimage.binary_fill_holes).  A component is a hole when it has no pixel on the image border,
 *      its area is <= max_hole_area (when max_hole_area > 0) and every foreground 4-neighbour of its pixels holds one class c; a
 *      hole becomes c.  A pocket bordered by two classes stays; an island inside a hole is untouched.
 *   3. Open (open_radius_sq).  For each class c of the stage-2 result, E_c = {p in A_c : no pixel q of the image with value != c has
 *      |p - q|^2 <= r2}: pixels outside the image do not erode, as in mgu_distance_transform, so an object cut by the frame keeps
 *      its edge.  A pixel p of A_c stays c iff some q in E_c has |p - q|^2 <= r2, else it becomes 0.
 * counts_dev (may be NULL): int64 (B,3), set to the pixels [gained by closing, filled, removed by opening] of every image.
 * Close and open work on 64-pixel words of one class plane (tiles with a halo in LDS, below 64 KiB); fill labels the background with
 * mgu_connected_components' union-find.  At most 8 kernel launches and 1 fill, whatever B, the classes and the holes; no host
 * synchronisation; scratch from the context (18 bytes per pixel with fill_holes, else 2).  B <= 65535, B*H*W < 2^31. */
int mgu_clean_masks(mgu_ctx* ctx, const void* src_dev, int src_kind, int B, int H, int W, int C, int64_t num_classes, int close_radius_sq,
                    int fill_holes, int64_t max_hole_area, int open_radius_sq, int64_t* out_dev, int64_t* counts_dev, void* hip_stream);

/* ---- boundary evaluation: surface-distance histograms and band counts behind the BF score, Boundary IoU, Hausdorff, HD95, ASSD -----
 * How well the outline of every class in a predicted map follows the outline of the same class in the target map: what region IoU
 * barely registers.  The reference has no boundary metric; the definitions below are this build's own (after Csurka et al. 2013 and
 * Cheng et al. 2021, with the two deviations stated).  All in exact integers: bitwise repeatable, comparable with ==.
 * Input: pred_dev / pred_kind / C as mgu_clean_masks reads its source (0: int64 class map (B,H,W); 1: NHWC fp32 logits with the argmax
 * fused, first maximal class, bit-identical to mgu_argmax_classes; num_classes must then equal C).  target_dev: int64 class map
 * (B,H,W).  Foreground classes are 1 .. num_classes-1 (2 <= num_classes <= 32); on both sides every other value (0, -100, out of
 * range) reads as background.  Images never interact.  With X one of the maps P (prediction) and G (target) of one image:
 *   Boundary.  dX_c = the pixels of class c in X that have a 4-neighbour INSIDE THE IMAGE holding another value.  Pixels outside the
 *     image do not count, as in mgu_distance_transform and the opening of mgu_clean_masks: a fruit cut by the frame has no contour
 *     along the frame, and a map that is entirely class c has an empty boundary.  (The published Boundary IoU code pads the mask with
 *     background, so there an object keeps a contour along the frame: it differs here.)  Equivalently: D2_X(p) == 1.
 *   Surface distance.  Direction 0 (prediction to target): for every p in dP_c, d2(p) = min |p - q|^2 over q in dG_c, exact, int32; p
 *     is UNMATCHED when dG_c is empty in that image.  Direction 1 (target to prediction) is the converse.
 *   Band.  X_c^r = {p of class c in X : D2_X(p) <= band_r2} (band_r2 >= 1), D2_X = mgu_distance_transform of X's class map: the pixels
 *     within a Euclidean disc of the other values -- not the paper's iterated 3x3 erosion.
 * Outputs, all int64 and SET (not accumulated), with K = num_classes-1 and class c at index c-1:
 *   hist_dev  (B, K, 2, max_d2 + 2), 1 <= max_d2 <= 4096: bin k <= max_d2 counts the source boundary pixels of that direction with
 *             d2 == k; the last bin counts those with d2 > max_d2 plus the unmatched ones.
 *   stats_dev (B, K, 2, 4): [n = source boundary pixels, n_unmatched, the max d2 over the matched pixels (0 if none), the sum over the
 *             matched pixels of floor(sqrt(d2 * 2^32)) = floor(2^16 sqrt(d2))].  The last is defined on integers (math.isqrt(d2 << 32));
 *             the kernel's fp64 root is only a first guess that integer comparisons correct, so no rounding mode enters.
 *   band_dev  (B, K, 3): [|P_c^r & G_c^r|, |P_c^r|, |G_c^r|].
 * 6 kernel launches and 3 fills whatever B, the classes and the boundaries (class planes; the two launches of the distance transform;
 * site columns; site rows, where only the boundary pixels walk and a row without any leaves at once; bands); no host synchronisation;
 * scratch from the context: 24 + 4 K bytes per pixel of B*H*W.  The site rows keep 4 bytes of LDS per pixel of a row plus 4 per
 * bin (at most 80 KiB).  H, W <= 16384, B <= 32767 (2B planes are a grid dimension), 2B*(H*W+1) < 2^31.  B*H*W == 0: MGU_OK, nothing
 * is touched. */
int mgu_boundary_tables(mgu_ctx* ctx, const void* pred_dev, int pred_kind, const int64_t* target_dev, int B, int H, int W, int C,
                        int64_t num_classes, int max_d2, int band_r2, int64_t* hist_dev, int64_t* stats_dev, int64_t* band_dev,
                        void* hip_stream);

/* ---- instance evaluation: mask overlaps of two label maps, mask-IoU matching, panoptic totals ---------------------------------------
 * The objects of both sides are what mgu_connected_components / mgu_split_objects (labels, offsets) and mgu_object_stats (class,
 * area) write for the same B images: "gt" and "pred".  Object capacities are the lengths of the per-object arrays; an image whose
 * objects pass one of them (offsets[b+1] > capacity) is skipped as a whole, as mgu_object_stats / mgu_match_objects skip it.
 * Overlap table.  For every pair (GT object g, predicted object p) sharing at least one pixel, the number of shared pixels, in CSR
 * form by predicted object, all indices batch-wide:
 *   pair_ptr_dev    int64 (pred_capacity + 1): row p is [pair_ptr[p], pair_ptr[p+1]); every entry is written, rows of no object are
 *                   empty, pair_ptr[pred_capacity] = the number of distinct pairs (the true prefix sums, also on overflow)
 *   pair_gt_dev     int64 (pair_capacity): GT index, ASCENDING inside a row
 *   pair_inter_dev  int64 (pair_capacity): pixels carrying both labels, >= 1
 *   status_dev      int32 scalar, OR-ed (the caller clears it): 1 = more distinct pairs than pair_capacity -- entries whose place is
 *                   >= pair_capacity are dropped, nothing is written past the arrays, and mgu_match_masks / mgu_panoptic_totals
 *                   given the same pair_capacity read only what exists; 2 = an image was skipped (it contributes no pairs)
 * Entries [0, min(pairs, pair_capacity)) of pair_gt / pair_inter are written.  Distinct pairs <= B*H*W, so pair_capacity = B*H*W
 * never overflows; there is no dense n_gt x n_pred table.  Labels outside 1..n_b of their image read as background.  Every output
 * word is a pure function of the inputs: counts are integer atomics and the order inside a row is a rank, so the result is bitwise
 * repeatable.  Construction: an open-addressing hash table of 2*B*H*W + 64 slots keyed by (p << 32 | g) (64-bit compare-and-swap
 * insert, integer add of pixel counts, combined over 4 pixels per lane and over runs of lanes inside a wave before the atomic), a
 * scan of the row degrees, a pour into the rows and a rank pass.  6 kernel launches and 2 fills whatever the objects; no host
 * synchronisation; scratch from the context, about 40 bytes per pixel plus 4 per pair_ptr entry.  B*H*W < 2^31, capacities < 2^31. */
int mgu_object_overlaps(mgu_ctx* ctx, const int32_t* gt_labels_dev, const int64_t* gt_offsets_dev, int64_t gt_capacity,
                        const int32_t* pred_labels_dev, const int64_t* pred_offsets_dev, int64_t pred_capacity, int B, int H, int W,
                        int64_t pair_capacity, int64_t* pair_ptr_dev, int64_t* pair_gt_dev, int64_t* pair_inter_dev, int32_t* status_dev,
                        void* hip_stream);
/* The greedy matching of metrics.py:215-240 on MASK IoU, in confidence order, for T thresholds at once (1 <= T <= 16;
 * thresholds_dev: T doubles on the device), every threshold with its own used flags as COCO evaluates.  Per image: the predictions
 * are visited by descending scores_dev (fp32 as mgu_object_scores writes them; equal scores, -0 = +0 included: the smaller object
 * index first; NaN last; scores_dev NULL: list order).  Each scans its row of the overlap table; candidates are the GT objects of
 * its class not yet used at that threshold; IoU = (double)inter / (double)(area_p + area_g - inter), the fp64 expression of
 * mgu_match_objects (= Python's int / int); the strictly larger IoU wins, an equal IoU goes to the smaller GT index; it is a match
 * if IoU > 0 and IoU >= t.  One workgroup per image; 2 launches (1 without scores).
 *   match_gt_dev   int64 (T, pred_capacity): the batch-wide GT index, or -1
 *   match_iou_dev  double (T, pred_capacity): the matched IoU, else 0
 *   totals_dev     int64 (T, 3) ACCUMULATED: [GT objects, predicted objects, matched], as mgu_match_objects accumulates
 * Only the rows of the objects present (of images not skipped) are written.  Uses the context's object scratch (T bytes per GT
 * capacity row, 4 per predicted one).  B <= 65535. */
int mgu_match_masks(mgu_ctx* ctx, int B, const int64_t* pair_ptr_dev, const int64_t* pair_gt_dev, const int64_t* pair_inter_dev,
                    int64_t pair_capacity, const int64_t* gt_offsets_dev, const int64_t* gt_class_dev, const int64_t* gt_area_dev,
                    int64_t gt_capacity, const int64_t* pred_offsets_dev, const int64_t* pred_class_dev, const int64_t* pred_area_dev,
                    int64_t pred_capacity, const float* scores_dev, const double* thresholds_dev, int T, int64_t* match_gt_dev,
                    double* match_iou_dev, int64_t* totals_dev, void* hip_stream);
/* The matching of panoptic quality on the same table: a pair is a true positive when the classes agree and
 * 2 * inter > area_p + area_g - inter (IoU > 1/2, tested exactly in int64, strict).  That holds for at most one partner per object,
 * so there is no order and no threshold.  pq_dev: uint64 (num_classes, 4) ACCUMULATED, row c = [TP, FP, FN, sum over the TP of
 * round_half_even(IoU * 2^32)] with IoU the fp64 quotient above: an integer sum, exact and order-free (the trick of
 * mgu_object_scores).  FP = predicted objects of class c - TP, FN = GT objects of class c - TP; objects whose class lies outside
 * [0, num_classes) are ignored on both sides, images skipped for a capacity too.  One launch.  B <= 65535. */
int mgu_panoptic_totals(mgu_ctx* ctx, int B, const int64_t* pair_ptr_dev, const int64_t* pair_gt_dev, const int64_t* pair_inter_dev,
                        int64_t pair_capacity, const int64_t* gt_offsets_dev, const int64_t* gt_class_dev, const int64_t* gt_area_dev,
                        int64_t gt_capacity, const int64_t* pred_offsets_dev, const int64_t* pred_class_dev, const int64_t* pred_area_dev,
                        int64_t pred_capacity, int num_classes, uint64_t* pq_dev, void* hip_stream);

/* ---- object shape: per-object moments, fitted ellipse and the per-instance form of EllipticalShapeLoss (model/unet/shape_loss.py
 *      :155-180 over the instances :42-48 and :85-92 ask for) straight from the label map: no dense masks, no per-object launches,
 *      no host synchronisation; the launch count does not depend on the number of objects ------------------------------------------
 * Raw power sums of mgu_connected_components' labels_dev / offsets_dev at batch-wide object index i < capacity (objects past it
 * are skipped).  moments_dev: uint64 (capacity, 12), row i = sum over the object's pixels of
 *   [u^2, uv, v^2, u^3, u^2 v, u v^2, v^3, u^4, u^3 v, u^2 v^2, u v^3, v^4],  u = x - xmin, v = y - ymin in pixels,
 * with (xmin, ymin) = bbox_dev[4i], bbox_dev[4i+1] as mgu_object_stats wrote them for the same labels (orders 0 and 1 are its
 * area_dev and sums_dev).  The rows of the objects present are zeroed first.  Unsigned 64-bit integer atomics: exact and order-free,
 * so bitwise repeatable.  A sum is exact while area * (max(w, h) - 1)^4 < 2^64 (w, h the box sides; a full-image object up to
 * 1024 x 1024 qualifies); past that it wraps, and mgu_object_shapes marks the object status 2 instead of using it.  B*H*W < 2^31. */
int mgu_object_moments(mgu_ctx* ctx, const int32_t* labels_dev, int B, int H, int W, const int64_t* offsets_dev, int64_t capacity,
                       const int32_t* bbox_dev, uint64_t* moments_dev, void* hip_stream);
/* Per-object shape from mgu_object_stats' area_dev / bbox_dev / sums_dev and mgu_object_moments' moments_dev (labels_dev, B, H, W as
 * given to it), one thread per object, all arithmetic in fp64 from the exact integers, every output rounded to fp32 once.  Row
 * i < min(offsets[B], capacity) of
 *   centroid_dev (2)  [sum x / n, sum y / n] in image coordinates (pixels)
 *   cov_dev (3)       [c_xx, c_xy, c_yy]: the sample covariance, divisor n - 1 (torch.cov), no epsilon (pixels^2)
 *   axes_dev (2)      [a, b] = [2 sqrt(l1), 2 sqrt(l2)], l1 >= l2 the eigenvalues of cov, l2 = det(cov) / l1 clamped at 0: the
 *                     semi-axes, in pixels, of the uniformly filled ellipse with that covariance
 *   angle_dev         0.5 atan2(2 c_xy, c_xx - c_yy), radians, the major axis from +x towards +y; atan2(0, 0) = 0
 *   fill_dev          n / (pi a b), 0 when b = 0: 1 for a filled ellipse, lower for a hollow or merged shape
 *   term_dev          mean_j (d_j^T (cov + epsilon I)^-1 d_j - 1)^2 over the object's centred pixels d_j (shape_loss.py:161-176);
 *                     ~7/3 for a filled ellipse, not 0
 *   status_dev        uint8: 0 analysed; 1 fewer than max(min_pixels, 2) pixels (the reference skips under 10, :158); 2 too large
 *                     for exact moments (the bound above).  With a status != 0 only the centroid is computed, the rest is 0.
 * Conditioning.  While n * max(w, h) < 2^30 the second moments are taken as exact integers, so det(cov), and with it b and fill, is
 * 0 exactly for collinear pixels (past that, fp64).  The term comes from the central moments of orders 2 and 4 (no second sweep)
 * while (l1 + epsilon) <= 256 (l2 + epsilon): its fp64 error grows as the square of that ratio and stays below 1e-11 there.  A
 * thinner object -- at the limit a one-pixel diagonal line, whose cov is singular and whose inverse has entries 1 / epsilon --
 * takes a per-pixel pass over labels_dev instead: each pixel's Mahalanobis value from exact integers, (m - 1)^2 added in uint64
 * fixed point (rounding below 2^-26 per pixel).  Both passes are always launched, whatever the objects.  A thin object
 * with n * max(w, h) >= 2^30 keeps the closed form.  Deterministic: pure functions of exact integers and order-free integer sums.
 * Uses the context's object scratch (8 bytes per capacity row).  B*H*W < 2^31. */
int mgu_object_shapes(mgu_ctx* ctx, const int32_t* labels_dev, int B, int H, int W, const int64_t* offsets_dev, int64_t capacity,
                      const int64_t* area_dev, const int32_t* bbox_dev, const int64_t* sums_dev, const uint64_t* moments_dev, float epsilon,
                      int min_pixels, float* centroid_dev, float* cov_dev, float* axes_dev, float* angle_dev, float* fill_dev, float* term_dev,
                      uint8_t* status_dev, void* hip_stream);
/* EllipticalShapeLoss over instances: loss_dev (one fp32) = the mean of term_dev[i] over the objects i < min(offsets[B], capacity)
 * with status_dev[i] == 0 and, when class_dev != NULL, class_dev[i] == keep_class; 0 when there are none (shape_loss.py:180).  One
 * workgroup adds the terms in a fixed order in fp64: bitwise repeatable. */
int mgu_elliptical_shape_loss_objects(mgu_ctx* ctx, int B, const int64_t* offsets_dev, int64_t capacity, const float* term_dev,
                                      const uint8_t* status_dev, const int64_t* class_dev, int64_t keep_class, float* loss_dev,
                                      void* hip_stream);

/* ---- test-time augmentation: flipped / rotated views of a batch and the mean of their softmaxes ----------------------------------
 * A view is the image flipped (flip bit 0: along W, torch.flip(x, (3,)); bit 1: along H, torch.flip(x, (2,))) and then turned r
 * quarter turns (torch.rot90(x, r, (2, 3))); r odd swaps H and W.  mgunet.tta.view_table lists the views of each transform set.
 * Views: writes G views of the (B,C,H,W) fp32 batch img_dev (element (b,c,y,x) at [b*s[0] + c*s[1] + y*s[2] + x*s[3]], in_strides a
 * HOST array of 4) as one contiguous NCHW batch (G*B, C, Hv, Wv), view-major (view k of the call, then image b).  views: HOST int32
 * (G, 2) rows {flip, r}; all G views must have the same shape (r of one parity unless H == W).  G <= 8, G*B <= 65535. */
int mgu_tta_views(mgu_ctx* ctx, const float* img_dev, int B, int C, int H, int W, const int64_t* in_strides, int G, const int32_t* views,
                  float* out_dev, void* hip_stream);
/* Merge: for every output pixel (b, y, x) and view k (in order), the softmax (fp32, maximum subtracted, expf) of the C logits of the
 * view pixel that the view's transform moved (y, x) to, summed in fp64 and multiplied by 1/K (exact), rounded to fp32 once:
 * the mean of the views' fp32 softmaxes with one fp32 rounding; equal softmaxes average to themselves.  The logits are the NHWC output of the
 * forward of each shape group: group 0 = the views with r even (every view when H == W), (G0*B, H, W, C); group 1 = the views with r
 * odd when H != W, (G1*B, W, H, C) (logits1_dev may be NULL when no view is in it).  views: HOST int32 (K, 4) rows {group, slot, flip,
 * r}: view k is image slot*B + b of its group.  K in {1, 2, 4, 8}, C <= 16.  Writes probs_dev NHWC fp32 (B,H,W,C), labels_dev
 * int64 (B,H,W) = the first maximal class, conf_dev fp32 (B,H,W) = its probability. */
int mgu_tta_merge(mgu_ctx* ctx, const float* logits0_dev, const float* logits1_dev, int B, int C, int H, int W, int K, const int32_t* views,
                  float* probs_dev, int64_t* labels_dev, float* conf_dev, void* hip_stream);

/* ---- tiled inference: an image larger than the network's input runs as overlapping tiles blended into one canvas -----------------
 * Grid, per axis (mgunet.tiled.tile_grid): image length L, tile T, overlap o with 0 <= o < T, stride S = T - o.  L <= T: one tile at
 * origin 0.  Otherwise ceil((L - T) / S) + 1 tiles, origins k S and, for the last, L - T.  The grid of an (H, W) image is the product
 * of the axes (nrows x ncols); tile t of a batch is image t / (nrows ncols), row-major within it.  Every entry point takes the tile
 * (Th, Tw) and the overlaps; the tile counts and origins follow from them, H and W by the rule above, on the host and in the
 * kernels alike (no origin table is passed); [t0, t0 + n) must lie inside B * nrows * ncols.  Refused (MGU_ERR_INVALID): an overlap
 * outside [0, T), a tile range outside the grid, NULL buffers, sizes < 1, more than 2^30 tiles.
 * Gather: writes tiles [t0, t0 + n) of the (B,C,H,W) fp32 batch img_dev (element (b,c,y,x) at [b*s[0] + c*s[1] + y*s[2] + x*s[3]],
 * in_strides a HOST array of 4) as one contiguous NCHW batch out_dev (n, C, Th, Tw), 16-byte aligned.  A tile pixel past the image
 * (only when L < T) reads it by reflect-101 folding, repeated as often as needed (numpy.pad(mode="reflect")); L = 1 reads index 0. */
int mgu_tile_gather(mgu_ctx* ctx, const float* img_dev, int B, int C, int H, int W, const int64_t* in_strides, int Th, int Tw, int overlap_y,
                    int overlap_x, int t0, int n, float* out_dev, void* hip_stream);
/* The same from HWC uint8 images (B, H, W, 3) contiguous, through ToTensor (/255) and Normalize exactly as mgu_preprocess_image_u8
 * applies them: channel c of the output reads byte 2 - c when bgr, mean3 / std3 HOST arrays of 3 floats.  out_dev (n, 3, Th, Tw). */
int mgu_tile_gather_u8(mgu_ctx* ctx, const uint8_t* img_dev, int B, int H, int W, int bgr, const float* mean3, const float* std3, int Th, int Tw,
                       int overlap_y, int overlap_x, int t0, int n, float* out_dev, void* hip_stream);
/* Accumulate: adds tiles [t0, t0 + n) to the canvas acc_dev, NHWC fp32 (B,H,W,C), 16-byte aligned.  tiles_dev: NHWC fp32
 * (n, Th, Tw, C), the forward's logits of the gathered chunk (is_prob 0: each pixel's softmax is taken in fp32, maximum subtracted,
 * expf, as mgu_tta_merge takes it) or probabilities used as they are (is_prob 1).  wy_dev / wx_dev: DEVICE fp32 (nrows, Th) /
 * (ncols, Tw), the per-axis window weights already divided by their sum over the tiles covering each image coordinate
 * (mgunet.tiled.tile_weights); a pixel's weight is the fp32 product of its two entries.  For every pixel of the image that a tile
 * of the chunk covers: acc = (its first covering tile of the whole grid lies in the chunk ? 0 : acc_dev) + sum of weight * p over
 * the chunk's covering tiles in ascending tile number; other pixels (and tile pixels past the image) are not touched.  So chunks
 * must be given in ascending order, each tile once; the canvas needs no clearing, and the result is bitwise the same however the
 * tiles are split into chunks.  No atomics.  labels_dev int64 (B,H,W) / conf_dev fp32 (B,H,W), both or neither: a pixel whose last
 * covering tile lies in the chunk also gets its first maximal class and that class's value (mgu_tile_finish's result).  C <= 16. */
int mgu_tile_accumulate(mgu_ctx* ctx, const float* tiles_dev, int is_prob, int B, int C, int H, int W, int Th, int Tw, int overlap_y, int overlap_x,
                        const float* wy_dev, const float* wx_dev, int t0, int n, float* acc_dev,
                        int64_t* labels_dev, float* conf_dev, void* hip_stream);
/* Finish, for a canvas accumulated without labels_dev / conf_dev: the first maximal class and its value at every pixel.  C <= 16. */
int mgu_tile_finish(mgu_ctx* ctx, const float* acc_dev, int B, int C, int H, int W, int64_t* labels_dev, float* conf_dev, void* hip_stream);

/* ---- resize / gather building blocks of FeatureFusion (model/fusion_detection/feature_fusion.py:43-162) ----------------------------
 * F.interpolate(mode='bilinear', align_corners=False) (:69-76, :140-144) of an NHWC fp32 map (B,Hi,Wi,C) with pixel pitch ld_in into
 * channels [c_off, c_off + C) of a (B,Ho,Wo,ld_out) buffer -- i.e. straight into its slice of the fused tensor. */
int mgu_resize_bilinear_nhwc(mgu_ctx* ctx, const void* in_dev, int ld_in, int B, int Hi, int Wi, int C, void* out_dev, int ld_out, int c_off,
                             int Ho, int Wo, void* hip_stream);
/* The per-region branch (:84-138): out[pixel][c_off + d] = table[ids[pixel]][d]; an id outside [0, R) gives zeros (the reference
 * leaves such pixels of its zero-initialised map untouched).  table (R, D) fp32, ids int64 (npix). */
int mgu_region_map_gather_nhwc(mgu_ctx* ctx, const float* table_dev, int R, int D, const int64_t* ids_dev, int64_t npix, float* out_dev,
                               int ld_out, int c_off, void* hip_stream);

/* ---- input / output pipeline around the network: byte and integer work reproduced exactly ---------------------------
 * The reference does these steps on the host with cv2 / PIL / torchvision.  Images are HWC uint8 in device memory.
 * ImagePreprocessor.preprocess (preprocessing/image_preprocessing/image_preprocess.py:26-31, 57-85): [BGR -> RGB | grey -> RGB] ->
 * torchvision Resize on a PIL image = PIL's antialiased BILINEAR resample in 8-bit fixed point (horizontal pass, then vertical, 22-bit
 * coefficients; vertical first where Image.resize does so: an image over 100 times taller than wide whose height shrinks)
 * -> ToTensor (/255) -> Normalize.  mean3 / std3: HOST arrays of 3 floats.  out element (c, y, x) at
 * out_dev[c*os_c + y*os_h + x*os_w] (fp32): CHW as the reference returns it, or an NHWC slot of a batch. */
int mgu_preprocess_image_u8(mgu_ctx* ctx, const uint8_t* img_dev, int Hs, int Ws, int channels /* 1 | 3 */, int bgr, int H, int W,
                            const float* mean3, const float* std3, void* out_dev, int64_t os_c, int64_t os_h, int64_t os_w, void* hip_stream);
/* preprocess_mask (:87-126): cv2.resize(INTER_NEAREST) (source index floor(dst * src/dst), clamped), np.clip to [0, num_classes-1], int64. */
int mgu_preprocess_mask_u8(mgu_ctx* ctx, const uint8_t* mask_dev, int Hs, int Ws, int H, int W, int num_classes, int64_t* out_dev,
                           void* hip_stream);
/* ---- training augmentation (image_preprocess.py:34-51): RandomHorizontalFlip then RandomRotation of the resized PIL image ------------
 * The flip and the rotation (PIL's img.rotate(angle, NEAREST, expand=False, fillcolor=0) through its 16.16 fixed-point affine path) of
 * one image are described by the flag `flip` and six int32 coefficients fix = {a0..a5} (mgunet.preprocess.pil_rotation_fixed): output
 * pixel (x, y) reads source pixel (xin, yin) = ((a2 + y a1 + x a0) >> 16, (a5 + y a4 + x a3) >> 16) -- column W-1-xin under flip -- when it
 * lies inside the image, else the fill.  H, W <= 8192 (above that PIL uses a float64 path that is not reproduced: MGU_ERR_INVALID).
 * Batch form: images (B, C, H, W) fp32, element (b, c, y, x) at [b*s[0] + c*s[1] + y*s[2] + x*s[3]] for in_strides / out_strides (HOST
 * arrays of 4; NCHW, channels-last or a slot of a bigger batch), out of place; fill_c: HOST array of C <= 16 floats (the fill per
 * channel, e.g. (0 - mean) / std); masks: optional int64 (B, H, W) contiguous (both null or both set), fill mask_fill; params_dev:
 * DEVICE int32 (B, 7) rows {flip, a0, a1, a2, a3, a4, a5}.  One launch for images and masks. */
int mgu_augment_flip_rotate(mgu_ctx* ctx, const float* img_in, float* img_out, int B, int C, int H, int W, const int64_t* in_strides,
                            const int64_t* out_strides, const float* fill_c, const int64_t* mask_in, int64_t* mask_out, int64_t mask_fill,
                            const int32_t* params_dev, void* hip_stream);
/* mgu_preprocess_image_u8 with the flip / rotation applied to the resized image (fix6: HOST array of 6); out-of-image pixels are the
 * normalised black (0/255 - mean) / std.  Same launches as mgu_preprocess_image_u8. */
int mgu_preprocess_image_u8_aug(mgu_ctx* ctx, const uint8_t* img_dev, int Hs, int Ws, int channels, int bgr, int H, int W, const float* mean3,
                                const float* std3, void* out_dev, int64_t os_c, int64_t os_h, int64_t os_w, int flip, const int32_t* fix6,
                                void* hip_stream);
/* mgu_preprocess_mask_u8 followed by the flip / rotation of the (H, W) label map; out-of-image pixels get mask_fill (not clipped). */
int mgu_preprocess_mask_u8_aug(mgu_ctx* ctx, const uint8_t* mask_dev, int Hs, int Ws, int H, int W, int num_classes, int flip, const int32_t* fix6,
                               int64_t mask_fill, int64_t* out_dev, void* hip_stream);
/* ---- scale, crop and colour augmentation from uint8 batches (csrc/augment_affine.hip) -----------------------------------------------
 * The reference has no such stage.  THIS BUILD'S DEFINITION, integers only up to the last step; `>>` is the arithmetic shift (floor).
 * img_u8 (B, Hs, Ws, 3) uint8 contiguous (bgr != 0: channel order B, G, R), mask_u8 optional (B, Hs, Ws) uint8 -> out: fp32 (B, 3, H, W),
 * element (b, c, y, x) at out[b*s[0] + c*s[1] + y*s[2] + x*s[3]] for out_strides (HOST array of 4), and mask_out int64 (B, H, W) contiguous.
 * params_dev: DEVICE int32 (B, 16), per image {a0..a5, A[3][3] row-major, k}.
 * Geometry.  Output pixel (x, y) has the source coordinates, 16.16 fixed point in pixel-index units, sums in int64:
 *     sx = a2 + y a1 + x a0          sy = a5 + y a4 + x a3
 *   The host folds flip, rotation, zoom, aspect, crop position, the Ws/W, Hs/H stretch and both half-pixel centres into a0..a5 with
 *   FIX(v) = floor(v 65536 + 0.5) on the float64 matrix (mgunet.preprocess.affine_fixed).
 *   Image, bilinear with 8-bit fractions: ix = sx >> 16, fx = (sx >> 8) & 255 (iy, fy likewise); taps (ix, iy), (ix+1, iy), (ix, iy+1),
 *   (ix+1, iy+1) with the weights (256-fx)(256-fy), fx(256-fy), (256-fx)fy, fx fy (sum 65536); a tap outside the source reads
 *   fill_rgb[c] (HOST array of 3 bytes, R G B; no clamp to the edge); v_c = (sum w p + 32768) >> 16, exact in uint32, at most 255.
 *   Mask, nearest: source pixel ((sx + 32768) >> 16, (sy + 32768) >> 16); outside the source mask_fill (e.g. -100, not clipped), inside
 *   the byte, clipped to [0, num_classes - 1] when num_classes > 0.
 * Colour, on the sampled bytes v = (v_R, v_G, v_B) (so the fill is a source colour and is jittered with the rest); A and k are Q12:
 *     t     = (k m + 128) >> 8                                                        (int64)
 *     out_c = clamp((A[c][0] v_R + A[c][1] v_G + A[c][2] v_B + t + 2048) >> 12, 0, 255)
 *   m: the image's mean luma in Q8 byte units over the WHOLE SOURCE image: S = sum over pixels (77 R + 150 G + 29 B) (uint64, integer
 *   atomics: associative, bitwise reproducible), m = (S + n/2) / n, n = Hs Ws, integer division.  |A|, |k| <= 2^15 (the host refuses
 *   more: mgunet.preprocess.color_matrix_q12); A = 4096 I, k = 0 passes the bytes unchanged.
 * Output: ToTensor (/255) and Normalize of out_c with mean3 / std3 (HOST arrays of 3), the float operations of mgu_preprocess_image_u8.
 * need_mean = 0 is the caller's statement that every k is 0: no luma kernel runs and t = 0.  Launches: the luma kernel (need_mean only,
 * after the one fill that clears its B sums in the context's scratch; 16-byte reads, one 64-bit integer atomic per workgroup and image)
 * and one kernel for the images and masks of the whole batch; no host synchronisation.  The result is stored 16 bytes at a time when
 * the output x-stride is 1, W % 4 == 0 and every row, channel and image of out (and mask_out) starts 16-byte aligned, else by element.
 * MGU_ERR_INVALID, before any device work: a null pointer; B, Hs, Ws, H, W < 1; a side above 8192; mask_u8 and mask_out not both set or
 * both null; B * tiles >= 2^31 (tiles: 32 x 32 of the result, mgu_augment_luma_tile() pixels of the source). */
int mgu_augment_affine_color(mgu_ctx* ctx, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, const uint8_t* mask_u8, int num_classes,
                             float* out, int H, int W, const int64_t* out_strides, const float* mean3, const float* std3,
                             const uint8_t* fill_rgb, int64_t* mask_out, int64_t mask_fill, const int32_t* params_dev, int need_mean,
                             void* hip_stream);
/* source pixels per workgroup of the luma kernel (tests place image sizes on its edges) */
int mgu_augment_luma_tile(void);
/* The luma pass alone: sums_dev[b] = S of image b (DEVICE int64 (B), cleared by this call's fill), as mgu_augment_affine_color forms it;
 * the mean luma of the definition is m = (S + n/2) / n. */
int mgu_augment_luma_sums(mgu_ctx* ctx, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, int64_t* sums_dev, void* hip_stream);
/* ---- elastic deformation in the scale / crop / colour pass (csrc/augment_elastic.hip) ---------------------------------------------------
 * Random elastic deformation (Ronneberger et al., MICCAI 2015, 3.1: displacement vectors on a coarse grid, interpolated to every pixel)
 * as one more term of the source coordinate of mgu_augment_affine_color: the image is still resampled once.  The reference has no such
 * stage.  THIS BUILD'S DEFINITION, integers only; `>>` is the arithmetic shift (floor), `/` the integer division of non-negative values.
 * Control grid.  Per image gh x gw nodes, 4 <= gh, gw <= 32; a node holds a displacement (cx, cy), int32 in 16.16 SOURCE-pixel units,
 *   |c| <= 2^26 (mgunet.preprocess.elastic_control refuses more).  ctrl_dev: DEVICE int32 (B, 2, gh, gw), plane 0 x, plane 1 y, nodes
 *   row-major.
 * Lattice coordinate of output pixel (x, y) of the W x H result:
 *     su = ((gw - 3) << 16) / W      u = x su + (su >> 1)  (int64)      i = u >> 16 in [0, gw - 4]      t = (u >> 8) & 255
 *   (floored, not rounded: (W-1) su + (su >> 1) < W su <= (gw - 3) 65536, so the last pixel stays below cell gw - 3); sv, v, j, s likewise
 *   from gh, H and y.
 * Weights.  The uniform cubic B-spline as a Q14 table Wq[t][0..3], t = 0..255, from integers: T = 256, D = 6 T^3,
 *     n0 = (T - t)^3     n1 = 3 t^3 - 6 T t^2 + 4 T^3     n2 = -3 t^3 + 3 T t^2 + 3 T^2 t + T^3     n3 = t^3        (sum D)
 *     w_k = (2 * 16384 n_k + D) / (2 D)
 *   and the larger of w1, w2 (w1 on a tie) takes the remainder, so that every row sums to 16384 exactly.  Wq[0] = (2731, 10922, 2731, 0),
 *   Wq[128] = (341, 7851, 7851, 341).  The library forms the table itself (mgunet.preprocess.bspline_weights_q14 is the same table).
 * Field.  Per plane  acc = sum_{b=0..3} sum_{a=0..3} Wq[s][b] Wq[t][a] c[j+b][i+a]  in int64 (|acc| < 2^54; exact, so the order of
 *   summation is free and nothing is rounded between the two passes), D = (acc + 2^27) >> 28.  A constant control field gives D = c
 *   exactly, zero gives zero; |D| <= 2^26.
 * Coordinates.  sx = a2 + y a1 + x a0 + Dx     sy = a5 + y a4 + x a3 + Dy   (int64).  From here on everything is the definition of
 *   mgu_augment_affine_color word for word: bilinear image taps with 8-bit fractions and fill_rgb, nearest mask with mask_fill and the
 *   class clip, the Q12 colour matrix and the mean luma over the whole source image, ToTensor + Normalize, arbitrary output strides.
 * Instance labels (optional).  labels_i32 int32 (B, Hs, Ws) -> labels_out int32 (B, H, W), both contiguous: nearest, source pixel
 *   ((sx + 32768) >> 16, (sy + 32768) >> 16), label_fill outside the source; values are never clipped.
 * mgu_augment_elastic_color takes the arguments of mgu_augment_affine_color, then the labels and the control grid.  ctrl_dev == NULL
 * requires gh == gw == 0 and gives the affine result.  Launches as the affine entry: the luma fill and kernel when need_mean, then ONE
 * kernel for the images, masks and labels of the whole batch; no host synchronisation.  The 16-byte stores need labels_out 16-byte
 * aligned too.  MGU_ERR_INVALID, before any device work: the affine entry's conditions; gh or gw outside [4, 32] when ctrl_dev is set (not
 * both 0 when it is not); labels_i32 and labels_out not both set or both null. */
int mgu_augment_elastic_color(mgu_ctx* ctx, const uint8_t* img_u8, int B, int Hs, int Ws, int bgr, const uint8_t* mask_u8, int num_classes,
                              float* out, int H, int W, const int64_t* out_strides, const float* mean3, const float* std3,
                              const uint8_t* fill_rgb, int64_t* mask_out, int64_t mask_fill, const int32_t* params_dev, int need_mean,
                              const int32_t* labels_i32, int32_t* labels_out, int32_t label_fill, const int32_t* ctrl_dev, int gh, int gw,
                              void* hip_stream);
/* The field alone: field_out DEVICE int32 (B, 2, H, W), plane 0 Dx, plane 1 Dy of every pixel of the W x H result, one launch.
 * MGU_ERR_INVALID: a null pointer; B, H, W < 1; a side above 8192; gh or gw outside [4, 32]; B * tiles >= 2^31. */
int mgu_elastic_field(mgu_ctx* ctx, const int32_t* ctrl_dev, int B, int gh, int gw, int H, int W, int32_t* field_out, void* hip_stream);
/* EdgeDetector.sobel_edges (preprocessing/graph_feature_processing/edge_detection.py:14-44), kernel size 3: RGB -> grey (15-bit fixed
 * point), Sobel x / y with reflect-101 borders, magnitude / max * 255 in double, truncated to uint8.  rgb (H,W,3) -> out (H,W). */
int mgu_sobel_edges_u8(mgu_ctx* ctx, const uint8_t* rgb_dev, int H, int W, uint8_t* out_dev, void* hip_stream);
/* HistogramEqualizer.equalize_histogram_rgb (histogram_equalization.py:13-35): RGB -> YUV, equalizeHist on Y, YUV -> RGB. */
int mgu_equalize_hist_rgb_u8(mgu_ctx* ctx, const uint8_t* rgb_dev, int H, int W, uint8_t* out_dev, void* hip_stream);
/* image_to_patches(map).mean(...) (scripts/graph_refinement.py:97-104): mean over each patch x patch window of a uint8 HWC map, zero
 * padded bottom / right; per_channel = 0: one value per patch over all channels, 1: one per channel.  out (nph*npw, 1 | channels). */
int mgu_patch_mean_u8(mgu_ctx* ctx, const uint8_t* img_dev, int H, int W, int channels, int patch, int per_channel, float* out_dev,
                      void* hip_stream);
/* GaussianSmoother.smooth (preprocessing/graph_feature_processing/gaussian_smoothing.py:23-34: cv2.GaussianBlur on uint8), csrc/gaussian.hip.
 * img (B,H,W,channels) interleaved uint8, channels 1..4 -> out of the same shape.  THIS BUILD'S DEFINITION, integers only, per channel:
 *   h[y][x] = sum_d kx[d] * src[y][r(x + d - kw/2, W)]          (at most 65280: 16 bits)
 *   v       = sum_d ky[d] * h[r(y + d - kh/2, H)][x]
 *   out     = (v + 32768) >> 16                                  (at most 255: no clamp)
 * r = reflect-101 applied repeatedly until the index is inside (a radius may exceed the image side); n == 1 gives 0.  kx_host / ky_host:
 * HOST arrays of kw / kh Q8.8 weights (passed to the kernel by value), kw and kh odd and in 1..31, every weight >= 0, each axis summing
 * to exactly 256 -- what mgunet.preprocess.gaussian_kernel_q8 makes from a float64 Gaussian (OpenCV's small tables for sigma <= 0 and
 * k <= 7) by rounding half to even with the error carried to the next tap and the centre taking the rest.  This follows the bit-exact
 * fixed-point scheme OpenCV 4.x publishes for 8-bit GaussianBlur; cv2 is absent from this build, so equality with a cv2 build is NOT
 * verified.  MGU_ERR_INVALID: even or out-of-range sizes, weights that are negative or do not sum to 256, out_dev overlapping img_dev,
 * H*W >= 2^31.  One launch whatever B is, no workspace, no floating point on the device: bitwise reproducible. */
int mgu_gaussian_blur_u8(mgu_ctx* ctx, const uint8_t* img_dev, int B, int H, int W, int channels, const int32_t* kx_host, int kw,
                         const int32_t* ky_host, int kh, uint8_t* out_dev, void* hip_stream);
/* The "Smooth" column block of the node features (scripts/graph_refinement.py:81): columns [col0, col0 + (per_channel ? 3 : 1)) of rows
 * (B*nph*npw, ld_out) fp32 get, bit for bit, what mgu_patch_mean_u8 gives on mgu_gaussian_blur_u8 of image b of rgb (B,H,W,3) -- same
 * zero padding bottom / right, row order and mean expression -- without writing a blurred image.  Other columns are not touched.  One
 * launch; patch 1..64, weights as above. */
int mgu_patch_smooth_mean_u8(mgu_ctx* ctx, const uint8_t* rgb_dev, int B, int H, int W, int patch, const int32_t* kx_host, int kw,
                             const int32_t* ky_host, int kh, int per_channel, float* out_dev, int ld_out, int col0, void* hip_stream);
/* Contrast-limited adaptive histogram equalisation (cv2.createCLAHE(clipLimit, tileGridSize).apply on 8-bit images), csrc/clahe.hip;
 * INTEGRATION.md section W.  The reference has no such stage.  img (B,H,W,channels) interleaved uint8, channels 1 or 3 -> out of the same
 * shape; grid_y x grid_x tiles, each in 1..64; clip_limit <= 0: no clipping.  channels 1: the plane v is the image; channels 3: v is Y of
 * cv2's RGB2YUV and the output pixel is YUV2RGB(out_v, U, V) with the pixel's own U and V, as mgu_equalize_hist_rgb_u8 around its table.
 * THIS BUILD'S DEFINITION, after OpenCV 4.x clahe.cpp for 8-bit images; cv2 is absent from this build, so equality with a cv2 build is
 * NOT verified.  Bitwise equal to tests/clahe_oracle.py and from run to run.
 *   geometry  H % grid_y == 0 and W % grid_x == 0: He, We = H, W.  Otherwise BOTH He = H + grid_y - H % grid_y and
 *             We = W + grid_x - W % grid_x (OpenCV's rule: an axis that divides is still extended by a whole grid when the other does
 *             not; 64 x 60 with 8 x 8 tiles gives 72 x 64).  th = He / grid_y, tw = We / grid_x, area = th * tw.  Extended pixel (y, x)
 *             reads v[r(y, H)][r(x, W)], r = reflect-101 applied until the index is inside (n == 1 gives 0); no extended image is written.
 *   table     of tile (ty, tx): h[256] over the tile's area extended pixels.  clip_limit > 0: cl = max(1, (int)(clip_limit * area / 256))
 *             (double, on the host); clipped = sum max(h[i] - cl, 0); h[i] = min(h[i], cl) + clipped / 256; residual = clipped % 256; if
 *             residual > 0, step = max(256 / residual, 1) and the bins k * step, k = 0 .. residual - 1, get one more each (OpenCV's loop in
 *             closed form; the sum of h is area again; no second clipping round).  lut[i] = sat8(rint((float)S_i * lutScale)), S_i the
 *             int32 inclusive sum converted to fp32, lutScale = 255.0f / (float)area (host), one rounded fp32 product, rint half to even.
 *   pixel     all fp32, EVERY operation rounded on its own (no fused multiply-add), inv_tw = 1.0f / (float)tw and inv_th on the host:
 *               txf = (float)x * inv_tw - 0.5f;  tx1 = floor(txf);  xa = txf - (float)tx1;  xa1 = 1.0f - xa
 *               tx2 = min(tx1 + 1, grid_x - 1);  tx1 = max(tx1, 0)        (clamped after xa is formed; likewise ty1, ty2, ya, ya1)
 *               res = (lut[ty1][tx1][v] * xa1 + lut[ty1][tx2][v] * xa) * ya1 + (lut[ty2][tx1][v] * xa1 + lut[ty2][tx2][v] * xa) * ya
 *               out = sat8(rint(res))
 * luts_dev: optional DEVICE (B, grid_y, grid_x, 256) uint8 that receives the tables; NULL keeps them in context scratch
 * (B * grid_y * grid_x * 256 bytes).  out_dev == img_dev is allowed (the tables are complete before the second launch, and each pixel is
 * read and written by one thread); any other overlap of the two, or of the tables with either, is MGU_ERR_INVALID, as are channels other
 * than 1 or 3, a grid outside 1..64, a non-finite clip_limit, NULL pointers, H*W >= 2^31 and B > 65535.  Exactly two launches whatever B,
 * the grid and the data are; no host synchronisation. */
int mgu_clahe_u8(mgu_ctx* ctx, const uint8_t* img_dev, int B, int H, int W, int channels, int grid_y, int grid_x, double clip_limit,
                 uint8_t* out_dev, uint8_t* luts_dev, void* hip_stream);
/* The equalised column block of the node features from CLAHE: columns [col0, col0 + (per_channel ? 3 : 1)) of rows (B*nph*npw, ld_out)
 * fp32 get, bit for bit, what mgu_patch_mean_u8 gives on mgu_clahe_u8 of image b of rgb (B,H,W,3) -- same zero padding bottom / right,
 * row order and mean expression -- without writing an equalised image.  Other columns are not touched.  Two launches (the table launch
 * is mgu_clahe_u8's, into context scratch); patch 1..64, the other arguments as above. */
int mgu_patch_clahe_mean_u8(mgu_ctx* ctx, const uint8_t* rgb_dev, int B, int H, int W, int patch, int grid_y, int grid_x, double clip_limit,
                            int per_channel, float* out_dev, int ld_out, int col0, void* hip_stream);
/* ---- edge-aware refinement of class probabilities (csrc/refine.hip) ---------------------------------------------
 * Every class plane is filtered `iterations` times with a joint bilateral kernel guided by the photograph, then argmax: cost-volume
 * filtering (Hosni et al., PAMI 2013), the message-passing step of a dense CRF.  The reference has NO such stage: what follows is THIS
 * BUILD'S DEFINITION, integers only after the first step, bitwise equal to tests/refine_oracle.py and from run to run.
 *   src_dev    NHWC fp32 (B,H,W,C), 1 <= C <= 16: probabilities (is_prob 1) or logits (is_prob 0: each pixel's softmax in fp32, maximum
 *              subtracted, expf, divided by its sum, exactly as mgu_tta_merge forms one view's softmax)
 *   guide_dev  uint8 (B,H,W,G) contiguous, G 1 or 3 (the photograph at the probabilities' resolution; the channel order does not matter)
 *   space_lut  HOST int32 (radius+1)*(radius+1), indexed [|dy|][|dx|];  range_lut  HOST int32 [1024];  every entry in [0, 256] and
 *              space_lut[0][0] * range_lut[0] >= 128 (the centre weight is >= 1: no denominator is 0).  shift in [0, 18], radius in
 *              [1, 7], iterations in [1, 16].  mgunet.bilateral_tables makes them from two sigmas.  Both are passed to the kernel by value.
 * Per image (images never interact):
 *   1. q0_k(p) = rint(clamp(x, 0, 1) * 65535): the product in fp32, rounded to nearest even, NaN -> 0; uint16, not renormalised.
 *   2. weight of tap d = (dy, dx), |dy|, |dx| <= radius, p + d inside the image, with d2 = sum_g (I_g(p) - I_g(p + d))^2 <= 195075:
 *        w = (space_lut[|dy|][|dx|] * range_lut[min(d2 >> shift, 1023)] + 128) >> 8          in [0, 256]
 *      Taps outside the image are skipped in numerator and denominator alike.
 *   3. num_k(p) = sum_d w q_k(p + d), den(p) = sum_d w, q'_k(p) = (num_k + (den >> 1)) / den (integer division).  radius <= 7 gives
 *      num <= 225 * 256 * 65535 = 3 774 816 000 < 2^32: uint32 sums are exact, and w <= 256 keeps each product a 24-bit multiply.
 *      That bound is why the radius stops at 7.
 *   4. repeated `iterations` times; iteration t + 1 reads only iteration t's planes.
 *   5. outputs, all SET: labels_dev int64 (B,H,W) the first maximal q_k (mgu_argmax_classes's tie rule); probs_dev fp32 NHWC (B,H,W,C)
 *      (float)q_k / 65535.0f, correctly rounded -- the planes need NOT sum to 1; conf_dev fp32 (B,H,W) the label's value in probs;
 *      changed_dev int64 (B) the pixels whose label differs from the first maximal q0_k (integer atomics).  probs_dev, conf_dev and
 *      changed_dev may be NULL.
 * Exactly `iterations` launches, plus one fill when changed_dev is given, whatever B, C and the contents; no host synchronisation.
 * Scratch (the context's, grown on first use): none for one iteration, one uint16 plane set of 2 B H W C bytes for two, two sets beyond.
 * MGU_ERR_INVALID, before anything is launched or written: a range violation above, G not 1 or 3, a NULL src_dev, guide_dev, labels_dev
 * or table, an output overlapping the source or the guide, B > 65535, B*H*W >= 2^31.  B*H*W == 0: MGU_OK, nothing touched. */
int mgu_refine_probs(mgu_ctx* ctx, const float* src_dev, int is_prob, const uint8_t* guide_dev, int B, int H, int W, int C, int G, int radius,
                     const int32_t* space_lut, const int32_t* range_lut, int shift, int iterations, float* probs_dev, int64_t* labels_dev,
                     float* conf_dev, int64_t* changed_dev, void* hip_stream);
/* ---- superpixel graphs (csrc/superpixels.hip) ------------------------------------------------------------------
 * Per image of a uint8 batch: an over-segmentation, its region adjacency graph as a CSR, a node-feature table and the means of feature
 * maps over the regions.  The reference has none of this (its region graph is a fully connected placeholder): what follows is THIS
 * BUILD'S DEFINITION, integers throughout, bitwise equal to tests/superpixels_oracle.py and from run to run.  No entry point
 * synchronises with the host; scratch comes from the context; MGU_ERR_INVALID is returned before anything is launched or written;
 * B == 0 is MGU_OK with nothing touched (the pointers may then be NULL).  B <= 65535, B*H*W < 2^31 everywhere.
 *
 * Colour.  Three HOST tables (mgunet.lab_tables(); the context keeps a device copy and refreshes it when their contents change):
 * lin_host uint16[256] = rint(4095 srgb_to_linear(v / 255)); m_host int32[9], row-major sRGB -> XYZ (D65) with every row scaled to
 * sum to exactly 4096; f_host uint16[4096] = rint(1024 f(t / 4095)) with the CIELAB f.  Accepted: lin <= 4095, m >= 0 with rows
 * summing to 4096, f <= 1024.  Per pixel, in int32:
 *   xyz_c = (m[c][0] lin[r] + m[c][1] lin[g] + m[c][2] lin[b] + 2048) >> 12                      in 0..4095
 *   L = (116 f[y] - 16384 + 128) >> 8,  a = (500 (f[x] - f[y]) + 128) >> 8,  b = (200 (f[y] - f[z]) + 128) >> 8
 * in quarter Lab units; >> of a negative value is an arithmetic shift (floor).
 *
 * mgu_slic_labels: integer SLIC in the gSLIC formulation.  rgb_dev (B,H,W,3) contiguous uint8; step S in 4..128, mq = round(4 m) in
 * 1..1024 (m: the compactness in Lab units), passes T in 1..32.  gx = ceil(W / S), gy = ceil(H / S); centre k = i gx + j starts at
 * (min(j S + S/2, W-1), min(i S + S/2, H-1)) with that pixel's Lab.  An assignment pass gives pixel (x, y), home cell (y / S, x / S),
 * to the centre of the up to nine cells (i + di, j + dj), di, dj in {-1, 0, 1}, inside the grid that minimises
 *   D = (dL^2 + da^2 + db^2) S^2 + mq^2 (dx^2 + dy^2)        int64; |dx|, |dy| < 3 S, so D < 2^39
 * against the centre's current integer [x, y, L, a, b]; an equal D goes to the smaller k.  A centre update sets each of the five to
 * floor((2 sum + n) / (2 n)) over the n pixels just assigned (floor, not truncation: the sums of a and b are negative on green and
 * blue images); n == 0 keeps the centre.  T passes with T - 1 updates in between; the labels of pass T are the output.
 *   raw_labels_dev  int32 (B,H,W) in [0, gx gy)
 *   centres_dev     optional int32 (B, gx gy, 6): [x, y, L, a, b, n] as the last pass read them, n = the pixels of the update that made
 *                   them (0 for a centre that was kept, and everywhere when T == 1)
 * Launches: 1 (Lab, packed 8 bytes per pixel) + 1 (centres) + T (assignment: a 32 x 32 tile per workgroup, its centres and the sums
 * of the next update in LDS, lanes that share a centre combined before the LDS atomics, six int32 atomics per centre and tile to
 * global memory; the last pass writes the label map instead) + T - 1 (update) = 2 T + 1, whatever B and the contents.  Scratch:
 * 8 bytes per pixel + 48 per centre.
 *
 * mgu_regions_connect: raw_labels_dev int32 (B,H,W), values in [0, 2^31 - 2], e.g. mgu_slic_labels' output.  The 4-connected
 * same-value components become regions (images never join; objects.hip's labelling passes).  Then `rounds` (0..8) merge rounds with
 * min_area (>= 0): at the start of a round a region is small if its area < min_area; each small region merges into the 4-adjacent
 * region of area >= min_area that shares the most pixel edges with it (a pixel edge: a horizontally or vertically adjacent pixel pair
 * with one pixel in each region), ties to the one whose first pixel comes first in raster order; a small region without such a
 * neighbour stays.  All merges of a round are decided from its starting state and applied together (small into large only: no
 * chains); the regions are renumbered after every round.
 *   labels_dev  int32 (B,H,W): every pixel in a region 0..n_b-1 of its image, numbered in raster order of the region's first pixel
 *   counts_dev  int64 (B), offsets_dev int64 (B+1): as mgu_connected_components writes them; batch-wide node = offsets[b] + label
 * Launches: 10 + 9 rounds, fills: 1 + 3 rounds, whatever B, the contents and whether a round merges anything.  Scratch: about 76 bytes
 * per pixel.  An output overlapping raw_labels_dev or another output is MGU_ERR_INVALID.  H*W == 0 with B > 0: counts and offsets 0.
 *
 * mgu_regions_adjacency: any int32 label map with offsets (labels < 0 or >= n_b take no part: a mgu_connected_components output
 * works after subtracting 1).  Nodes u != v of one image are adjacent when a pixel edge joins them; the weight is the number of such
 * pixel edges.  Both directions are written, rows by batch-wide node index, columns ASCENDING inside a row, no self loops; a row may
 * be empty.  int32 indices: what mgu_gat_layer_forward* consumes.
 *   rowptr_dev  int32 (node_capacity + 1): every entry is written; the true prefix sums, also on overflow
 *   col_dev, border_dev  int32 (edge_capacity): entries [0, min(edges, edge_capacity)); nothing is written past a capacity
 *   status_dev  int32, OR-ed (the caller clears it): 1 = more directed edges than edge_capacity (the surplus is dropped); 2 = an
 *               image's nodes pass node_capacity (offsets[b+1] > node_capacity): that image contributes nothing
 * Construction: objects_common.h's pair hash table (keyed row << 32 | column) and its scan / pour / rank kernels, shared with
 * mgu_object_overlaps.  6 launches and 2 fills.  Regions of mgu_regions_connect are connected, so their graph is planar: at most
 * 6 N - 12 directed edges for N >= 3 nodes.  B*H*W < 2^29, capacities < 2^31 - 1.  Scratch: up to 144 bytes per pixel.
 *
 * mgu_regions_features_u8: per node, integer atomics give area, sum x, sum y and the sums of the quarter-unit L, a, b above; then one
 * IEEE double expression per column, cast to fp32 once, into feat_dev (node_capacity, 8):
 *   [sum L / (400 area), sum a / (512 area), sum b / (512 area), (2 sum x + area) / (2 area W), (2 sum y + area) / (2 area H),
 *    area / (H W), 0, 0]
 * (integer numerators and denominators, each converted to double exactly; columns 6, 7 pad to the GAT's Fin % 4 == 0).  Rows of no
 * node, or of a node without a pixel, are zero.  stats_dev: optional int64 (node_capacity, 6) [area, sum x, sum y, sum L, sum a,
 * sum b].  Nodes of an image whose nodes pass node_capacity are skipped.  3 launches.
 *
 * mgu_regions_pool_nhwc: the mean over every region of channels [c_off, c_off + D) of feat_dev fp32 (B,H,W,ld) (1 <= D <= 4096,
 * c_off + D <= ld).  Each value adds q = round_half_even(clamp(v, -65536, 65536) * 2^20) (NaN -> 0; the product is exact in fp32) to
 * an int64 sum with integer atomics (exact while the region's sum of |v| stays below 2^43); out_dev (node_capacity, D) fp32 =
 * (float)((double)sum / (double)area * 2^-20), 0 for a row without pixels.  Order-free and bitwise reproducible; within
 * 2^-21 + 2^-24 |mean| of the float64 mean of the unquantised values.  3 launches.  No backward. */
int mgu_slic_labels(mgu_ctx* ctx, const uint8_t* rgb_dev, int B, int H, int W, int step, int mq, int passes, const uint16_t* lin_host,
                    const int32_t* m_host, const uint16_t* f_host, int32_t* raw_labels_dev, int32_t* centres_dev, void* hip_stream);
int mgu_regions_connect(mgu_ctx* ctx, const int32_t* raw_labels_dev, int B, int H, int W, int min_area, int rounds, int32_t* labels_dev,
                        int64_t* counts_dev, int64_t* offsets_dev, void* hip_stream);
int mgu_regions_adjacency(mgu_ctx* ctx, const int32_t* labels_dev, const int64_t* offsets_dev, int B, int H, int W, int64_t node_capacity,
                          int64_t edge_capacity, int32_t* rowptr_dev, int32_t* col_dev, int32_t* border_dev, int32_t* status_dev,
                          void* hip_stream);
int mgu_regions_features_u8(mgu_ctx* ctx, const uint8_t* rgb_dev, const int32_t* labels_dev, const int64_t* offsets_dev, int B, int H, int W,
                            const uint16_t* lin_host, const int32_t* m_host, const uint16_t* f_host, int64_t node_capacity, float* feat_dev,
                            int64_t* stats_dev, void* hip_stream);
int mgu_regions_pool_nhwc(mgu_ctx* ctx, const float* feat_dev, int ld, int c_off, int D, const int32_t* labels_dev, const int64_t* offsets_dev,
                          int B, int H, int W, int64_t node_capacity, float* out_dev, void* hip_stream);
/* ---- graph-branch inputs for a whole batch: the node features scripts/graph_refinement.py:72-113 defines and the patch labels
 *      scripts/train_end_to_end.py:340 describes (the training script draws both from torch's RNG, :326 / :342) -----------------------
 * Node features.  rgb (B,H,W,3) uint8 -> rows (B*nph*npw, ld_out) fp32, nph = ceil(H / patch), npw = ceil(W / patch), patches zero
 * padded bottom / right as image_to_patches pads them, image b's patches at rows [b*nph*npw, (b+1)*nph*npw) in raster order.  Columns:
 *   [0, repeat)         patches.mean(dim=[1,2,3]) repeated (:78; the script's repeat is 16) of the normalised fp32 image (B,3,H,W) whose
 *                       element (b,c,y,x) is img_dev[b*is_n + c*is_c + y*is_h + x*is_w] (NCHW or NHWC storage): double accumulation in a
 *                       fixed order over the patch's real pixels (pad pixels are zeros), / (3 patch^2), rounded once.  Skipped (no
 *                       columns) when img_dev is NULL or repeat is 0.
 *   next unet_cols      a copy of row i of unet_rows_dev (B*nph*npw, unet_cols) fp32 -- e.g. what mgu_unet_request_patch_mean or
 *                       mgu_patch_mean wrote.  Skipped when unet_rows_dev is NULL.
 *   next 1              mean byte of mgu_sobel_edges_u8(image b) over the patch (:89, :97-98)
 *   next 3 | 1          mean bytes of mgu_equalize_hist_rgb_u8(image b): per channel (per_channel 1; :101-103) or over all three (0)
 *   up to ld_out        zeros (ld_out >= the used columns; it lets a caller meet the GAT's Fin % 4 == 0 without another copy)
 * The two byte blocks equal mgu_patch_mean_u8 of the per-image maps bit for bit, but no map is written: one memset and three launches
 * whatever B is (per-image histogram + largest gradient; B equalisation tables; one workgroup, or one wave, per patch).  patch 1..64,
 * H*W < 2^31, B*nph*npw < 2^31.  Deterministic. */
int mgu_patch_node_features_u8(mgu_ctx* ctx, const uint8_t* rgb_dev, int B, int H, int W, int patch, const float* img_dev, int64_t is_n,
                               int64_t is_c, int64_t is_h, int64_t is_w, int repeat, const float* unet_rows_dev, int unet_cols, int per_channel,
                               float* out_dev, int ld_out, void* hip_stream);
/* Patch labels: one class per patch x patch window (the same grid, padding and row order as above) of B images.  src_kind as in
 * mgu_connected_components: 0 = int64 class map (B,H,W); 1 = NHWC fp32 logits (B,H,W,C) -- what mgu_unet_forward writes -- whose
 * per-pixel class is the first maximal channel (bit-identical to mgu_argmax_classes).  counts_dev (NULL: skipped): int32 (B*Np, C)
 * class histogram over the patch's REAL pixels -- pad pixels are not counted, and map values outside [0, C) (-100 ignore labels) are
 * counted nowhere; labels_dev: int64 (B*Np) the class with the largest count, the lowest such class on ties; purity_dev (NULL:
 * skipped): fp32 (B*Np) (float)((double)that count / (double)real pixels of the patch).  A patch with no counted pixel gets label 0
 * and purity 0.  1 <= C <= 32 (beyond: MGU_ERR_INVALID), patch 1..4096.  One launch; integer counts: exact and deterministic. */
int mgu_patch_labels(mgu_ctx* ctx, const void* src_dev, int src_kind, int B, int H, int W, int C, int patch, int32_t* counts_dev,
                     int64_t* labels_dev, float* purity_dev, void* hip_stream);
/* ---- exact binary s-t min cut of the patch graph (csrc/graphcut.hip) ------------------------------------------
 * The solver of the energy MinCutRefinement's constructor arguments parameterise (mincut_refinement.py:9-25; the reference has none):
 *   E(S) = sum_i D_i(S_i) + smoothness * sum over undirected (i,j) of w_ij [S_i != S_j],  D_i(fg) = -log p_i,  D_i(bg) = -log(1 - p_i),
 *   p clamped to [1e-6, 1 - 1e-6],  w_ij = exp(-(I_i - I_j)^2 / (2 sigma_intensity^2)) + gamma exp(-|f_i - f_j|^2 / (2 sigma_features^2)),
 * quantised to integer capacities q(x) = min(lrintf(x * unit), 2^20).  B graphs share ONE topology: the COO list (2, E) int64 of one
 * graph, holding both directions of every edge; node i of graph b is row b*N + i, edge k of graph b is entry b*E + k (COO order).
 *
 * Reverse-edge index over the CSR BY SOURCE of that list (mgu_coo_to_csr_device of the flipped list: rows = sources, col = targets,
 * rows not sorted by column).  For COO edge k = (u -> v) at CSR position p: perm_dev[p] = k, rev_dev[p] = position of (v -> u).
 * *status_dev (device int) gets bit 1: a reverse edge is missing; 2: a duplicate (u, v); 4: a self loop; 8: an id outside [0, N) or an
 * edge the CSR does not hold; 16 (no error of the list): a node of degree >= 4095, which only mgu_graphcut_expand cannot take.  The caller
 * decides when to read it (once per new graph). */
int mgu_graphcut_rev_index(mgu_ctx* ctx, const int64_t* coo_dev, int64_t E, int num_nodes, const int32_t* rowptr_dev, const int32_t* col_dev,
                           int32_t* rev_dev, int32_t* perm_dev, int* status_dev, void* hip_stream);
/* One launch: cap_source[b*N+i] = q(D_i(bg)), cap_sink[b*N+i] = q(D_i(fg)), cap_edge[b*E+k] = q(smoothness * w) (all int32).  The prior is
 * EITHER prior_dev fp32 (B*N) probabilities OR counts_dev int32 (B*N, num_classes) class counts as mgu_patch_labels writes them with
 * p = (n_fg + 1) / (n_all + 2) for class fg_class; the other pointer NULL.  intensity_dev fp32 (B*N) on the 0..255 scale and feat_dev
 * fp32 (B*N, D) are optional: a term of w whose input is NULL is dropped (neither: every cap_edge is 0).  fp32 logf / expf, the
 * squared feature distance in double; both directions of an edge form it from the lower to the higher node id, so cap_edge is
 * bitwise symmetric.  An edge with an id outside [0, N) gets capacity 0. */
int mgu_graphcut_capacities(mgu_ctx* ctx, int B, int N, const int64_t* coo_dev, int64_t E, const float* prior_dev, const int32_t* counts_dev,
                            int num_classes, int fg_class, const float* intensity_dev, const float* feat_dev, int D, float gamma,
                            float sigma_intensity, float sigma_features, float smoothness, float unit, int32_t* cap_source_dev,
                            int32_t* cap_sink_dev, int32_t* cap_edge_dev, void* hip_stream);
/* The cut: phase 1 of push-relabel in lock step, one workgroup per graph, the residual graph in LDS (20 N + 4 E + 40 bytes, checked
 * against the device's shared memory per block: a larger graph is MGU_ERR_INVALID before anything is launched).  Capacities are int32
 * in the layout above (negative values count as 0) and are not written.  labels_dev uint8 (B*N): 1 = foreground (source side) iff
 * the sink cannot be reached from the node in the residual graph -- the same set for every maximum preflow, i.e. among cuts of equal
 * cost the one with the LARGEST foreground; flow_dev int64 (B): the flow into the sink = E(labels) in capacity units; rounds_dev int32
 * (B): push / relabel rounds taken (deterministic); converged_dev int32 (B): 0 when max_rounds ended the solve first (labels and flow
 * are then no cut).  relabel_period: rounds between global relabels, threads: workgroup size (a multiple of 64 up to 1024); 0 = the
 * measured defaults.  No host synchronisation. */
int mgu_graphcut_solve(mgu_ctx* ctx, int B, int N, int64_t E, const int32_t* rowptr_dev, const int32_t* col_dev, const int32_t* rev_dev,
                       const int32_t* perm_dev, const int32_t* cap_source_dev, const int32_t* cap_sink_dev, const int32_t* cap_edge_dev,
                       int max_rounds, int relabel_period, int threads, uint8_t* labels_dev, int64_t* flow_dev, int32_t* rounds_dev,
                       int32_t* converged_dev, void* hip_stream);
/* energy_dev int64 (B): cap_sink over the nodes labelled non-zero (foreground) + cap_source over the others + cap_edge[k] over the COO
 * edges from a foreground to a background node.  Integer sums: exact, order-free.  B <= 65535. */
int mgu_graphcut_energy(mgu_ctx* ctx, int B, int N, const int64_t* coo_dev, int64_t E, const uint8_t* labels_dev, const int32_t* cap_source_dev,
                        const int32_t* cap_sink_dev, const int32_t* cap_edge_dev, int64_t* energy_dev, void* hip_stream);
/* ---- K labels over the same graph: alpha-expansion (csrc/graphcut.hip) -------------------------------------------
 *   E(L) = sum_i U_i(L_i) + sum over pairs {i,j} of w_ij [L_i != L_j],  L_i in {0 .. K-1},  U_i(k) = q(-log p_i(k)), p clamped to [1e-6, 1],
 * w_ij = cap_edge of the arc from the LOWER to the HIGHER node id as mgu_graphcut_capacities writes it (the other direction is not read;
 * that kernel writes both bitwise equal).  Costs and weights count as clamped to [0, 2^20].  For K = 2, cap_source = U(., 0) and
 * cap_sink = U(., 1) this is E(S) above.
 *
 * One launch: costs_dev int32 (rows, K) from EITHER prob_dev fp32 (rows, K) probabilities OR counts_dev int32 (rows, K) class counts as
 * mgu_patch_labels writes them, p = (n_k + 1) / (n_all + K); the other pointer NULL.  Evaluated in double: the count path is exact. */
int mgu_graphcut_label_costs(mgu_ctx* ctx, int64_t rows, int K, const float* prob_dev, const int32_t* counts_dev, float unit, int32_t* costs_dev,
                             void* hip_stream);
/* The whole expansion in one launch, one workgroup per graph, topology arrays as for mgu_graphcut_solve.  Start: init_dev uint8 (B*N), a
 * value >= K replaced by the node's cheapest label; NULL: every node's cheapest label (the lowest on ties).  A move on alpha builds the
 * binary cut "x_i = 1: node i takes alpha" of the current labelling in LDS (pair i < j, a = L_i, b = L_j, A = w[a != b], B = w[a != alpha],
 * C = w[alpha != b]: sink(i) += max(C - A, 0), source(i) += max(A - C, 0), source(j) += C, arc j -> i = B + C - A; U_i(alpha) on the sink
 * arc, U_i(L_i) on the source arc), solves it by the rounds of mgu_graphcut_solve from zero heights and takes the largest set of nodes
 * that may switch at minimal cost.  The move is accepted iff it lowers E strictly (integer sums: exact).  alpha runs 0 .. K-1
 * cyclically; K rejected moves in a row end the loop with converged 1.  max_cycles * K moves, or a move whose solve reaches max_rounds,
 * end it with converged 0 and the last accepted labelling.  Outputs per graph: labels_dev uint8 (B*N), energy_dev int64 = E(labels),
 * moves_dev / accepted_dev / rounds_dev (summed over the moves) / converged_dev int32.  costs_dev and cap_edge_dev are not written.
 * LDS: 20 N + 4 E + 48 + (N rounded up to 8) bytes against the device's shared memory per block, MGU_ERR_INVALID beyond it before
 * anything is launched.  A move's residual sink word is 32 bits and can reach (1 + degree) 2^20: the topology must not carry status
 * bit 16 of mgu_graphcut_rev_index (the caller checks; such a word saturates at 2^32 - 1).  1 <= K <= 255, 0 <= max_cycles <= 2^20. */
int mgu_graphcut_expand(mgu_ctx* ctx, int B, int N, int64_t E, int K, const int32_t* rowptr_dev, const int32_t* col_dev, const int32_t* rev_dev,
                        const int32_t* perm_dev, const int32_t* costs_dev, const int32_t* cap_edge_dev, const uint8_t* init_dev, int max_cycles,
                        int max_rounds, int relabel_period, int threads, uint8_t* labels_dev, int64_t* energy_dev, int32_t* moves_dev,
                        int32_t* accepted_dev, int32_t* rounds_dev, int32_t* converged_dev, void* hip_stream);
/* energy_dev int64 (B): E(L) above of any labelling labels_dev uint8 (B*N); a label >= K counts as K - 1.  Integer sums: exact.  B <= 65535. */
int mgu_graphcut_energy_multi(mgu_ctx* ctx, int B, int N, const int64_t* coo_dev, int64_t E, int K, const uint8_t* labels_dev, const int32_t* costs_dev,
                              const int32_t* cap_edge_dev, int64_t* energy_dev, void* hip_stream);
/* postprocess_segmentation (scripts/infer_segmentation.py:20-51, :123): class labels int64 -> colour map uint8 (npix, 3) through a
 * palette (num_classes, 3) the caller provides (the reference's BGR list), labels outside [0, num_classes) stay black; and, if
 * labels_u8_dev != NULL, the uint8 label map written next to it. */
int mgu_colorize_labels(mgu_ctx* ctx, const int64_t* labels_dev, int64_t npix, const uint8_t* palette_dev, int num_classes, uint8_t* vis_dev,
                        uint8_t* labels_u8_dev, void* hip_stream);

/* ---- per-channel building blocks of the DetectionHead: model/fusion_detection/detection_head.py ---- */
/* y[m][c] = act(scale[c] * x[m][c] + shift[c]) over an (M, C) NHWC view with row pitches ldx / ldy (floats); scale / shift
 * may be NULL (1 / 0); act 0 = none (the BatchNorm2d that follows a ReLU, :33-38), 1 = ReLU, 2 = sigmoid (:101,104).
 * C, ldx, ldy multiples of 4. */
int mgu_channel_affine_nhwc(mgu_ctx* ctx, const float* x_dev, int ldx, int64_t M, int C, const float* scale_dev,
                            const float* shift_dev, int act, float* y_dev, int ldy, void* hip_stream);
/* out[c] = sum over the M rows of x[m][c]: AdaptiveAvgPool2d((1,1)) (:39) per image is this sum / (H W). 4 <= C <= 1024. */
int mgu_channel_sum_nhwc(mgu_ctx* ctx, const float* x_dev, int ldx, int64_t M, int C, float* out_dev, void* hip_stream);

/* out (B, C)[b] = column sums of image b of x (B, M, C) (row pitch ldx): AdaptiveAvgPool2d over a batch in one call. */
int mgu_channel_sum_images_nhwc(mgu_ctx* ctx, const float* x_dev, int ldx, int B, int64_t M, int C, float* out_dev, void* hip_stream);

/* ---- video: frame registration and object tracks (csrc/video.hip) ----------------------------------------------
 * THIS BUILD'S DEFINITION (the reference cuts its videos into frames and has no such stage).  Integers only; every output word is a
 * pure function of the inputs (integer atomics, ranks and scans): bitwise repeatable.  No call synchronises with the host.
 *
 * Registration.  frames_u8: uint8 (T, H, W, channels), channels 3 (RGB, or BGR with bgr != 0) or 1 (grey), T >= 2.
 *   luma byte      Y = (77 R + 150 G + 29 B + 128) >> 8 (mgu_augment_affine_color's coefficients); a grey frame is its own luma
 *   coarse plane   Hc = H / factor, Wc = W / factor (floor; trailing rows and columns are dropped), factor f in {1, 2, 4, 8};
 *                  pixel = (sum of the f x f block of Y + f*f/2) / (f*f)
 *   coarse search  pair (t, t+1), A / B = the coarse planes of frames t / t+1, R = radius (1..32): for every s = (sy, sx) in [-R, R]^2
 *                  cost(s) = sum over p in [R, Hc-R) x [R, Wc-R) of |A(p) - B(p + s)| -- the same window for every s, nothing read
 *                  outside a plane; a scene point at p in frame t lies at p + s in frame t+1.  Hc - 2R >= 8 and Wc - 2R >= 8.
 *   choice         the smallest cost; ties: the smallest sy^2 + sx^2, then the smaller sy, then the smaller sx
 *   fine search    (f > 1) on the full-resolution luma: shifts f*s_c + d, d in [-f, f]^2, window [M, H-M) x [M, W-M) with
 *                  M = f*R + f for every pair, the same choice applied to d; the centre f*s_c is read from device memory
 *   shifts_dev     int32 (T-1, 2): [dy, dx] in full-resolution pixels
 *   cost_dev       int64 (T-1, 2): of the last level searched, [the cost at the chosen shift, the cost at that level's d = 0 (the
 *                  zero shift when f = 1, the coarse choice f*s_c when f > 1)]
 *   surface_dev    NULL, or int64 (T-1, 2R+1, 2R+1): the coarse cost surface, [sy + R][sx + R]
 * A workgroup holds one 48 x 48 tile (mgu_frame_sad_tile) of the window and its search halo as bytes in LDS; a lane owns four
 * x-shifts of one y-shift and walks the tile with v_sad_u8 on 32-bit words (an unaligned word from two neighbours: v_alignbyte_b32);
 * tile partials are uint32, the surface is summed with 64-bit integer atomics.  No masked SAD form is used: zero bytes count.
 * Launches whatever T and the contents: f = 1: 3 kernels (planes, SAD, pick) and 1 fill; f > 1: 6 kernels (two of each) and 2 fills.
 * Scratch from the context: T * (Hc*Wc + H*W) bytes and the surfaces. */
int mgu_frame_sad_tile(void);
int mgu_frame_shifts(mgu_ctx* ctx, const uint8_t* frames_u8, int T, int H, int W, int channels, int bgr, int radius, int factor,
                     int32_t* shifts_dev, int64_t* cost_dev, int64_t* surface_dev, void* hip_stream);
/* One coordinate frame per pair.  labels_dev int32 (T, H, W) and offsets_dev int64 (T+1) as mgu_connected_components /
 * mgu_split_objects write them for the T frames as one batch; shifts_dev int32 (T-1, 2) as mgu_frame_shifts writes them (read on the
 * device; any values are safe).  For pair b = frames (b, b+1) with s = shifts[b], both int32 (T-1, H, W):
 *   prev_aligned[b][q] = labels[b][q - s] where q - s lies inside the frame, else 0
 *   next_cropped[b][q] = labels[b+1][q] where q - s lies inside the frame (the common rectangle of frame and frame + s), else 0
 * vis_prev_dev / vis_next_dev: int64 (capacity), cleared by the call: at an object's batch-wide index the pixels it keeps in
 * prev_aligned of the pair it opens (objects of frames 0..T-2) / in next_cropped of the pair it closes (frames 1..T-1); objects at
 * an index >= capacity are not counted.  The two maps with offsets_dev (prev side) and offsets_dev + 1 (next side) are what
 * mgu_object_overlaps and mgu_match_masks take as "gt" and "pred" of T-1 images: their indices are batch-wide, so offsets that do not
 * start at 0 need no rebasing.  1 kernel and 2 fills.  T*H*W < 2^31. */
int mgu_track_align(mgu_ctx* ctx, const int32_t* labels_dev, const int64_t* offsets_dev, int64_t capacity, const int32_t* shifts_dev, int T,
                    int H, int W, int32_t* prev_aligned_dev, int32_t* next_cropped_dev, int64_t* vis_prev_dev, int64_t* vis_next_dev,
                    void* hip_stream);
/* Track ids.  offsets_dev int64 (T+1); link_dev int64 (capacity): the batch-wide index of an object's predecessor (an object of an
 * earlier frame) or -1 (row 0 of mgu_match_masks' match_gt); class_dev int64 (capacity).  One workgroup walks the frames in order: an
 * object takes its predecessor's id, an unlinked object the next fresh id in object order (*next_id_dev + its rank among the frame's
 * unlinked objects: a scan, no atomic decides an id).  first_ids_dev: NULL (frame 0's objects are all new), or the ids of frame 0's
 * objects from the call before, when frame 0 repeats that call's last frame: they are taken as they are and frame 0 is not counted
 * again.  next_id_dev: int64 device scalar, read and written.
 *   track_id_dev     int64 (capacity)
 *   track_len_dev    int32 (track_capacity), ACCUMULATED (the caller clears it): frames in which the track has an object
 *   track_class_dev  int64 (track_capacity): the class of the track's first object
 *   status_dev       int32 scalar, OR-ed: 1 = an id reached track_capacity (its track is not recorded; nothing is written past the
 *                    arrays; track_id still carries it), 2 = objects past capacity were left out
 * 1 kernel. */
int mgu_track_ids(mgu_ctx* ctx, const int64_t* offsets_dev, int T, int64_t capacity, const int64_t* link_dev, const int64_t* class_dev,
                  const int64_t* first_ids_dev, int64_t* next_id_dev, int64_t* track_id_dev, int32_t* track_len_dev, int64_t* track_class_dev,
                  int64_t track_capacity, int32_t* status_dev, void* hip_stream);

/* ---- masks in and out (csrc/maskio.hip): COCO run lengths, polygon outlines, polygon fill ------------------
 * The label map is what mgu_connected_components / mgu_split_objects write: labels_dev int32 (B, H, W), 0 = background, and
 * offsets_dev int64 (B + 1); object k of image b is batch-wide row offsets[b] + k - 1.  A pixel whose value lies outside
 * [1, offsets[b+1] - offsets[b]], or whose row is >= capacity (the length of the per-object arrays), belongs to no object.  All four
 * are integer definitions of this build (the reference reads class PNGs and has no such stage).  Every output word is a pure function
 * of the inputs: places come from scans and a stable radix sort, the only atomics are integer add and max; bitwise repeatable.  No
 * host synchronisation, no wait between workgroups; the number of launches depends on H, W and the arguments, never on the data or
 * on B.  Arrays are sized by the caller; status_dev is an int32 scalar, OR-ed (the caller clears it), one bit per kind of overflow,
 * and the surplus is dropped: nothing is written past an array.  B*H*W < 2^31, B <= 65535, H, W <= 32768, capacities < 2^31.
 * With P(n) = ceil(n / 8) sort passes and bits(v) the bits that hold v, N = capacity:
 *
 * mgu_mask_runs: the runs of every object in COCO's column-major order.  The position of pixel (x, y) is p = x*H + y; a run of object
 * i is a maximal interval of consecutive positions whose pixels are i's (so a run continues from the last row of a column into the
 * first row of the next).  CSR by object:
 *   run_ptr_dev     int64 (capacity + 1), every entry written: the true prefix sums, also on overflow
 *   run_start_dev   int32 (run_capacity): ascending inside a row, start[j+1] > start[j] + length[j]
 *   run_length_dev  int32 (run_capacity)
 *   status          1 = more runs than run_capacity (entries whose place is >= run_capacity are dropped: every row that ends at or
 *                   before run_capacity is complete); 2 = offsets[B] > capacity (the objects past it have no row)
 * Runs <= B*H*W, so that run_capacity never overflows.  9 + 3 P(bits(N-1)) launches and 1 fill; scratch 29 bytes per pixel + 4 per row. */
int mgu_mask_runs(mgu_ctx* ctx, const int32_t* labels_dev, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W,
                  int64_t run_capacity, int64_t* run_ptr_dev, int32_t* run_start_dev, int32_t* run_length_dev, int32_t* status_dev,
                  void* hip_stream);
/* The inverse: labels_dev is filled with zeros, then every run of row i paints k = i - offsets[b] + 1 over its positions of image b
 * (the image whose rows hold i).  Where objects overlap the largest label wins.  status: 1 = a run with start < 0, length < 1 or
 * start + length > H*W (it paints nothing); 2 = a run of a row outside [offsets[0], offsets[B]) (nothing); 4 = run_ptr[capacity] >
 * run_capacity (the runs past it are not there).  1 launch and 1 fill; no scratch. */
int mgu_runs_to_labels(mgu_ctx* ctx, const int64_t* run_ptr_dev, const int32_t* run_start_dev, const int32_t* run_length_dev,
                       int64_t run_capacity, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W, int32_t* labels_dev,
                       int32_t* status_dev, void* hip_stream);
/* mgu_object_outlines: the closed polygons of every object on the pixel grid.  Pixel (x, y) has corners (x, y), (x+1, y), (x+1, y+1),
 * (x, y+1); a side is an outline edge of object i when the pixel is i's and the pixel across is not -- the outside of the image
 * counts as "not", so outlines are closed along the frame.  Sides run clockwise on the screen: top 0 (x,y)->(x+1,y), right 1
 * (x+1,y)->(x+1,y+1), bottom 2 (x+1,y+1)->(x,y+1), left 3 (x,y+1)->(x,y); edge id = (y*W + x)*4 + side.  The successor of an edge is
 * the edge of the same object that leaves its end point; where two leave (two pixels of i meet diagonally), connectivity 1 takes the
 * right turn (the same pixel) and connectivity 2 the left turn (the diagonal pixel).  The cycles of that permutation are the loops.  A
 * loop's leader is its smallest edge id; the loops of an object are listed by ascending leader; the stored vertices are the start
 * points of the edges whose predecessor has another direction, in travel order from the first such point at or after the leader's
 * start point.
 *   loop_ptr_dev    int64 (capacity + 1): the loops of object i are [loop_ptr[i], loop_ptr[i+1]); true prefix sums, also on overflow
 *   vertex_ptr_dev  int64 (loop_capacity + 1): the vertices of loop l; true prefix sums of the loops below loop_capacity
 *   vertices_dev    int32 (vertex_capacity, 2): (x, y)
 *   loop_area2_dev  int64 (loop_capacity): the shoelace sum of x_j y_j+1 - x_j+1 y_j: > 0 for an outer loop, < 0 for a hole; over
 *                   the loops of an object it is twice the object's pixel count
 *   status          1 = more loops than loop_capacity; 2 = more vertices than vertex_capacity (in both cases what lies past the
 *                   capacity is dropped and every row that ends before it is complete); 4 = offsets[B] > capacity
 * Loops <= B*H*W and vertices <= 4*B*H*W (every pixel its own object reaches both).  4*B*H*W < 2^31.  17 + bits(4HW-1) +
 * 3 P(bits(N-1) + bits(4HW-1)) launches and 4 fills; scratch 165 bytes per pixel + 4 per row and per loop_ptr / vertex_ptr entry. */
int mgu_object_outlines(mgu_ctx* ctx, const int32_t* labels_dev, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W,
                        int connectivity, int64_t loop_capacity, int64_t vertex_capacity, int64_t* loop_ptr_dev, int64_t* vertex_ptr_dev,
                        int32_t* vertices_dev, int64_t* loop_area2_dev, int32_t* status_dev, void* hip_stream);
/* mgu_polygons_to_labels: polygons in the layout above (loop_ptr (capacity + 1), vertex_ptr (loop_capacity + 1), vertices) into a
 * label map.  Coordinates are fixed point with frac_bits in 0..4 fraction bits, |v| < 2^24, and may lie outside the image.  Object i
 * covers a pixel iff an odd number of the edges of all its loops count for the pixel's centre (even-odd, not winding), exactly: in
 * doubled units X = 2v, Cx = (2x+1) 2^frac_bits, Cy = (2y+1) 2^frac_bits, the edge (x0,y0)->(x1,y1) counts iff (y0 <= Cy) != (y1 <= Cy)
 * and, ordered so that y0 < y1, x0 (y1-y0) + (x1-x0)(Cy-y0) < Cx (y1-y0).  Horizontal and zero-length edges never count; a centre on
 * an edge is decided by these inequalities alone.  Every loop is closed from its last vertex to its first.  labels_dev is filled with
 * zeros first; where objects overlap the largest label wins.  This is not COCO's rleFrPoly (which upsamples by 5 and draws lines).
 * One crossing is kept per (edge, scanline it counts for):
 *   status          1 = more crossings than crossing_capacity (the objects whose edges come first are complete); 2 = a loop of a row
 *                   outside [offsets[0], offsets[B]), or loop_ptr / vertex_ptr pass loop_capacity / vertex_capacity; 4 = a coordinate
 *                   outside (-2^24, 2^24) (the edge is left out)
 * The outlines of a label map cross 2*B*H*W times at most.  4 + 3 P(bits(N-1) + bits(H-1) + bits(W)) launches and 1 fill; scratch
 * 24 bytes per crossing_capacity entry + 12 per vertex. */
int mgu_polygons_to_labels(mgu_ctx* ctx, const int64_t* loop_ptr_dev, const int64_t* vertex_ptr_dev, const int32_t* vertices_dev,
                           int64_t loop_capacity, int64_t vertex_capacity, const int64_t* offsets_dev, int64_t capacity, int B, int H, int W,
                           int frac_bits, int64_t crossing_capacity, int32_t* labels_dev, int32_t* status_dev, void* hip_stream);

/* ---- introspection for bench.py / profiles ------------------------------------------------------ */
/* FLOPs (2*MAC, convolutions only) of one U-Net forward over B images: SURVEY 8d table. */
double mgu_unet_flops(mgu_ctx* ctx, int B, int H, int W);
/* FLOPs the matrix cores actually EXECUTE for the same forward: the fp32 3x3 layers with Cin % 16 == 0 run as
 * Winograd F(2x2,3x3) -- 16 multiplies per 2x2 output tile and (cin, cout) pair instead of 36 (csrc/wino_f32.hip);
 * equal to mgu_unet_flops when that path is off (bf16 storage, MGU_NO_WINOGRAD=1). */
double mgu_unet_mfma_flops(mgu_ctx* ctx, int B, int H, int W);
/* Time the conv/GEMM kernels of the LAST mgu_unet_forward with HIP events on the launch stream:
 * enable before the forward, read after.  Adds event records only (no syncs) while enabled. */
int mgu_profile_enable(mgu_ctx* ctx, int on);
/* Per kernel family, summed over the launches recorded since mgu_profile_enable(ctx, 1) (U-Net forward / backward convolutions,
 * the mgu_conv2d_nhwc / mgu_conv2d_prepared_nhwc / mgu_conv_transpose2x2_nhwc building blocks -- name only, no FLOP counts --,
 * GAT kernels): time between HIP events recorded on the launch stream right around each launch, algorithmic FLOPs (2*MAC of the
 * operator) and the FLOPs actually issued on the matrix pipe (`pipe`: 0 fp32 MFMA, 1 bf16 MFMA, -1 none).  `name` is the kernel's
 * name as rocprofv3 --kernel-trace prints it (template arguments included where two instantiations are used).  A read CONSUMES the
 * records: with profiling left on, the next read covers the launches since this one. */
typedef struct {
  const char* name;
  double ms, flops_alg, flops_mfma;
  int launches, pipe;
} mgu_kernel_stat;
int mgu_profile_read_kernels(mgu_ctx* ctx, mgu_kernel_stat* out, int cap, int* n_out);
int mgu_profile_read(mgu_ctx* ctx, double* conv_ms, int* conv_launches, double* total_ms);
/* ConvTranspose launches of this context since mgu_create that ran on the hand-scheduled assembly kernel mgu_convt_x3_gfx950
 * (csrc/asm/gen_convt_x3.py).  The profiling records name it like the C++ kernel it replaces, convt2x2_x3_kernel (bitwise equal
 * results): this count is how a test or a tool tells the two apart.  MGU_CONVT_ASM=0 at mgu_create keeps it at 0. */
int64_t mgu_convt_asm_launches(mgu_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* MGUNET_H */
