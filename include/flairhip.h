/* libflairhip -- C ABI of the MI355X (gfx950) tiled-segmentation hot path.
 *
 * The reference (kezakool/flair-for-aigle) is pure Python and has no FFI of its own: the seam this
 * library replaces is the set of torch / segmentation_models_pytorch calls listed per entry point
 * below (file:line under the reference tree).  INTEGRATION.md shows the ctypes binding a maintainer
 * would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, a negative FFA_ERR_* for argument / support errors, or a
 *     positive hipError_t when a launch fails; nothing throws; ffa_last_error() gives the text of
 *     the last failure on the calling thread
 *   - every launch goes to the caller's hipStream_t; the library never allocates device memory,
 *     never synchronises and keeps no mutable global state (workspace is passed in; query sizes
 *     with the *_workspace_bytes functions)
 *   - tensors are raw device pointers, NHWC, contiguous, dtype FFA_BF16 (storage) or FFA_F32,
 *     channel pitch a multiple of 16 elements (8 where noted); pad channels must hold zeros
 *   - all reductions are fixed-order (bitwise reproducible); no float atomics anywhere
 */
#ifndef FLAIRHIP_H
#define FLAIRHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* ffa_stream_t; /* == hipStream_t */

#define FFA_BF16 0
#define FFA_F32 1

#define FFA_OK 0
#define FFA_ERR_ARG (-1)
#define FFA_ERR_UNSUPPORTED (-2)
#define FFA_ERR_WORKSPACE (-3)

const char* ffa_last_error(void);
int ffa_version(void);
const char* ffa_target_arch(void);

/* ---- convolution (replaces the conv2d forward/backward reached via
 *      flair_hub/models/monotemp_model.py:68-92 -> smp encoder/decoder, called at
 *      flair_hub/models/flair_model.py:376 and :417-419) ------------------------------------------ */

/* preferred block height (output channels per workgroup) for a layer; weights are packed for it */
int ffa_conv_block_co(int kh, int kw, int stride, int cout);
/* Operand layout + block height of a layer: the `bco` value for ffa_pack_conv_weight_bytes / ffa_pack_conv_weight /
 * ffa_pack_desc_fill / ffa_pack_conv_weights_batched and for the `bco` field of ffa_conv_call_t.
 * Bits 0..11 = rows per block (pad the row count to a multiple of it).  FFA_BCO_RING = the operand is packed for the
 * LDS-DMA ring kernels (csrc/conv3x3_ring.hip; bf16: conv3x3_ring16_kernel, the default for 3x3 stride 1 pad 1 layers
 * with >= 64 output channels and whole 64-byte groups of input channels -- FFA_RING=0 in the environment restores the
 * conv_igemm kernels; f32: conv3x3_ring_kernel, FFA_RING=1).  FFA_BCO_THIN = the register-resident operand of the thin
 * layers (csrc/conv3x3_thin.hip: bf16, <= 32 real output rows, input pitch 16 or 32 -- the decoder's last two blocks
 * and the segmentation head; FFA_THIN=0 disables).  FFA_BCO_STEM = the operand of the ResNet stem kernel
 * (csrc/conv7x7_stem.hip: bf16 7x7 stride-2 pad-3 convolution of a <= 8-channel tile stored at pitch 16 into 64
 * channels, torchvision's conv1 as smp's ResNetEncoder keeps it; FFA_STEM=0 disables).  `allow`: bit 0 admits the ring
 * layout, bit 1 the thin one, bit 2 the stem one; which forms of call each layout serves is the table at
 * ffa_conv_call_t. */
#define FFA_BCO_RING 0x1000
#define FFA_BCO_THIN 0x2000
#define FFA_BCO_STEM 0x8000
int ffa_conv_plan(int dtype, int kh, int kw, int stride, int cout, int ci_pitch, int allow);
int ffa_conv_row_group(int kh);
/* Weight packing (csrc/conv_pack.hip): OIHW f32 master weight -> the operand of the layout in `bco` (ffa_conv_plan),
 * whose size in bytes the first call returns.  transpose=1 builds the dgrad operand (rows = input channels, taps
 * mirrored).  scale (optional, per row) folds an eval-mode BatchNorm. */
long long ffa_pack_conv_weight_bytes(int dtype, int co_rows, int ci_pitch, int kh, int kw, int bco);
int ffa_pack_conv_weight(int dtype, const float* w_oihw, const float* scale, void* dst, int O, int I, int kh, int kw,
                         int transpose, int co_rows, int ci_pitch, int bco, int rg, ffa_stream_t stream);
/* Every conv operand of a network in one launch per layout: descriptors (ffa_pack_desc_bytes each, the same type for every
 * layout) are filled on the host, copied to the device once, one table per layout, and replayed every step.  A
 * descriptor covers the column block W[:, col0 : col0 + ncols] of a weight with I_total input channels (one modality's
 * share of a FusionHandler 1x1 convolution, flair_hub/models/flair_model.py:470-475,533-541; conv_igemm layout only)
 * or, with col0 = 0 and ncols = I_total, the whole tensor. */
int ffa_pack_desc_bytes(void);
int ffa_pack_desc_fill(void* host_desc, const float* w_oihw, const float* scale, void* dst, int O, int I_total, int col0,
                       int ncols, int kh, int kw, int transpose, int co_rows, int ci_pitch, int bco, int rg, int dtype);
int ffa_pack_conv_weights_batched(int dtype, int bco, const void* descs_device, int n, ffa_stream_t stream);

/* One forward / input-gradient convolution call.  Replaces F.conv2d and what surrounds it at the call sites below.
 *
 * form
 *   FFA_CONV_PLAIN   out = relu?(conv(in', w) + bias + residual).  dil = 2 reads `in` through a virtual zero insertion
 *                    (the input gradient of a stride-2 layer; stride must then be 1).  smp's Conv2dReLU / torchvision's
 *                    BasicBlock and Bottleneck convolutions and their input gradients.
 *   FFA_CONV_UPCAT   3x3 stride-1 pad-1 convolution over the virtual tensor cat(nearest_x2(in), in2) -- what smp's
 *                    DecoderBlock builds with F.interpolate(scale_factor=2, mode="nearest") + torch.cat before its
 *                    first conv (reached from flair_model.py:417-419) -- without writing it: in [B][Hi/2][Wi/2][c1],
 *                    in2 [B][Hi][Wi][Ci - c1], or null with c1 = Ci (the skip-less form).  Hi, Wi, Ci describe the
 *                    virtual tensor.  No residual.
 *   FFA_CONV_POOLED  the input gradient of the FFA_CONV_UPCAT convolution as the two tensors the decoder block needs
 *                    (replaces the dgrad convolution + ffa_upsample_nearest2x_concat_bwd): output channels below c1 are
 *                    2x2-sum-pooled (the adjoint of nearest x2) into out [B][Ho/2][Wo/2][c1], the rest go to out2
 *                    [B][Ho][Wo][Co - c1], or nowhere with c1 = Co.  Ho, Wo, Co describe the gradient of the virtual
 *                    tensor; w is the transposed operand.  Plain epilogue: no bias, residual, relu or statistics.
 * Epilogues and the prologue are switched on by their pointers:
 *   stats      per pixel tile, the channel sums and sums of squares of the output stored:
 *              stats[route.ntiles][2][Co] f32.  With ffa_bn_finalize this replaces the statistics pass of the
 *              training-mode BatchNorm that follows (F.batch_norm as called by Conv2dReLU / BasicBlock).
 *   pro_scale, pro_shift  (both or neither) in' = relu(in * pro_scale[c] + pro_shift[c]) evaluated while the input is
 *              staged: the BatchNorm + ReLU of the PRODUCING layer (Conv2dReLU -> Conv2dReLU, BasicBlock conv1 -> bn1 ->
 *              relu -> conv2: flair_hub/models/monotemp_model.py:68-92); the normalised tensor is never written and
 *              zero padding applies to it.  Bit-identical to ffa_bn_apply followed by the same call without prologue.
 *   bnx, bn_scale, bn_shift  (with stats) the output is the gradient dy of y = relu(bnx * bn_scale + bn_shift): stats
 *              receives per tile sum(g), sum(g * bnx), g = dy where y > 0 else 0, so that ffa_bn_bwd_partials can skip
 *              the reduction pass of ffa_bn_bwd.  bnx has the shape and pitch of out.
 *
 * Which operand layout (ffa_conv_plan) serves which form:
 *                 conv_igemm                        ring                thin                        stem
 *   PLAIN         any supported kernel; dil 1 / 2;  3x3 s1 p1 dil 1;    bf16 3x3 s1 p1 dil 1;       bf16 7x7 s2 p3;
 *                 stats, bnx                        stats, prologue     stats, prologue             stats; no residual
 *   UPCAT         c1 covers whole halo channel      --                  in2 = null only; stats,     --
 *                 groups (else UNSUPPORTED); stats                      prologue
 *   POOLED        c1 a multiple of the block's      --                  c1 = Co only                --
 *                 rows (else UNSUPPORTED)
 * A form the layout does not serve is FFA_ERR_UNSUPPORTED (the caller falls back to materialising the tensor), a call
 * that breaks the geometry its layout was packed for is FFA_ERR_ARG. */
#define FFA_CONV_PLAIN 0
#define FFA_CONV_UPCAT 1
#define FFA_CONV_POOLED 2
typedef struct {
  int dtype;
  int form;
  const void* in;
  const void* in2;
  const void* w;       /* packed operand (ffa_pack_conv_weight) of co_rows rows in the layout `bco` */
  const float* bias;   /* [>= Co] or null */
  const void* residual; /* shape and pitch of out, or null */
  void* out;
  void* out2;
  float* stats;
  const float* pro_scale;
  const float* pro_shift;
  const void* bnx;
  const float* bn_scale;
  const float* bn_shift;
  int co_rows, bco;
  int B, Hi, Wi, Ci;   /* channel pitches: a multiple of 16 (Ci) / 8 (Co) */
  int Ho, Wo, Co;
  int kh, kw, stride, pad, dil;
  int relu;
  int c1;              /* channel split of the UPCAT / POOLED forms, else 0 */
} ffa_conv_call_t;

/* What a call runs: kernel family, output pixel tile, pixel tiles (ntiles = rows of the statistics partials) and grid.
 * conv3x3_persist_kernel and conv_igemm_kernel serve the same operands and are separate symbols in a profile
 * (FFA_CONV_PERSIST=0 keeps every call on the latter). */
#define FFA_CONV_KERNEL_IGEMM 0
#define FFA_CONV_KERNEL_PERSIST 1
#define FFA_CONV_KERNEL_RING 2
#define FFA_CONV_KERNEL_RING16 3
#define FFA_CONV_KERNEL_THIN 4
#define FFA_CONV_KERNEL_STEM 5
typedef struct {
  int kernel;
  int variant;  /* instantiation within the family (conv_igemm: 32-byte channel groups per halo fill; ring: tile configuration) */
  int th, tw;
  int tiles_x, tiles_y;
  int ntiles;
  int ncb;      /* blocks of output rows */
  int grid;
} ffa_conv_route_t;

/* Validates geometry and form x layout and fills *route.  Launches nothing, reads no tensor (only whether the optional
 * pointers are null) and makes no HIP call: it answers on a machine without a GPU. */
int ffa_conv_route(const ffa_conv_call_t* call, ffa_conv_route_t* route);
/* Checks the pointers, routes the same way and launches. */
int ffa_conv_run(const ffa_conv_call_t* call, ffa_stream_t stream);
/* sizeof(ffa_conv_call_t) (which = 0) / sizeof(ffa_conv_route_t) (1): a binding checks its own layout against it */
int ffa_conv_struct_bytes(int which);
/* 1 when the channel split (c1 from the low-resolution map, c2 from the skip tensor) of a 3x3 decoder convolution is
 * served by both the FFA_CONV_UPCAT form (conv_igemm layout) and ffa_conv_wgrad_upcat, else 0 */
int ffa_conv_upcat_supported(int dtype, int c1, int c2);
long long ffa_conv_wgrad_workspace_bytes(int dtype, int kh, int kw, int stride, int Co, int Ci, int B, int Ho, int Wo);
int ffa_conv_wgrad(int dtype, const void* x, const void* dy, float* dw_oihw, int B, int Hi, int Wi, int Ci, int Ho,
                   int Wo, int Co, int Co_real, int Ci_real, int kh, int kw, int stride, int pad, int accumulate,
                   void* workspace, long long workspace_bytes, ffa_stream_t stream);

/* Weight gradient of the FFA_CONV_UPCAT convolution: the input is the virtual cat(nearest_x2(lo), skip),
 * dw is OIHW [Co_real][C1 + C2][3][3] f32.  Workspace: ffa_conv_wgrad_workspace_bytes(dtype, 3, 3, 1, Co, C1 + C2, B,
 * 2*Hl, 2*Wl).  FFA_ERR_UNSUPPORTED when C1 is not a multiple of the kernel's input-channel block. */
int ffa_conv_wgrad_upcat(int dtype, const void* lo, const void* skip, const void* dy, float* dw_oihw, int B, int Hl,
                         int Wl, int C1, int C2, int Co, int Co_real, int accumulate, void* workspace,
                         long long workspace_bytes, ffa_stream_t stream);

/* "Normalise on load" for the weight gradient: ffa_conv_wgrad / ffa_conv_wgrad_upcat (skip-less) of a layer whose
 * input was relu(x * pro_scale[c] + pro_shift[c]) -- the prologue of ffa_conv_call_t on the weight-gradient side; the
 * normalised tensor is never written (replaces ffa_bn_apply + ffa_conv_wgrad; bit-identical to that sequence, zero
 * padding applied after the normalisation).  bf16, 3x3 stride 1 pad 1.  up != 0: x is the low-resolution map of the
 * skip-less nearest-x2 form.  FFA_ERR_UNSUPPORTED where no prologue kernel exists. */
int ffa_conv_wgrad_pro(int dtype, const void* x, const void* dy, float* dw_oihw, const float* pro_scale,
                       const float* pro_shift, int B, int Hi, int Wi, int Ci, int Ho, int Wo, int Co, int Co_real,
                       int Ci_real, int up, int accumulate, void* workspace, long long workspace_bytes,
                       ffa_stream_t stream);

/* ---- U-TAE Sentinel time-series branch (flair_hub/models/multitemp_model.py) ------------------
 * Small NHWC kernels around ffa_conv_run for the temporally shared encoder, the L-TAE and the attention-weighted skip
 * aggregation; evaluation-mode forward. */
/* out[n][y][x] = in[n][refl(y-1)][refl(x-1)]: the padding of nn.Conv2d(padding=1, padding_mode="reflect")
 * (multitemp_model.py:473-482); the convolution itself is ffa_conv_run with pad 0 on the padded tensor */
int ffa_reflect_pad1(int dtype, const void* in, void* out, int N, int H, int W, int C, ffa_stream_t stream);
/* y = [residual +] relu?(GroupNorm(x)): nn.GroupNorm of ConvLayer (:464-468, 4 groups over an image) and of LTAE2d
 * (:224-231, 16 groups over the dates of one pixel).  Sample s starts at element (s / Q) * stride_hi +
 * (s % Q) * stride_lo and has `inner` positions, inner_stride elements apart, of C contiguous channels. */
int ffa_group_norm(int dtype, const void* x, const void* residual, void* y, const float* gamma, const float* beta,
                   long long samples, int Q, long long stride_hi, long long stride_lo, int inner,
                   long long inner_stride, int C, int groups, float eps, int relu, ffa_stream_t stream);
/* PositionalEncoder (:287-313): out[n][r*d + j] = sin|cos(pos[n] / period^(2*(j/2)/d)), repeated `repeat` times */
int ffa_positional_encoding(const float* pos, float* out, int n, int d, int repeat, float period, ffa_stream_t stream);
/* x[n][p][c] += vec[n][c] (f32 vec): "out + positional_encoder(bp)" (:270) */
int ffa_add_rowvec(int dtype, void* x, const float* vec, int N, int P, int C, ffa_stream_t stream);
/* MultiHeadAttention with one learnt query per head + masked softmax over the dates (:337-403), per pixel:
 * k [B][T][P][n_head*d_k], v [B][T][P][n_head*d_v], Q f32 [n_head][d_k], pad u8 [B][T] ->
 * out [B][P][n_head*d_v], attn f32 [n_head][B][T][P] */
int ffa_ltae_attention(int dtype, const void* k, const void* v, const float* Q, const unsigned char* pad, void* out,
                       float* attn, int B, int T, int P, int n_head, int d_k, int d_v, ffa_stream_t stream);
/* Temporal_Aggregator(mode="att_group") (:609-628,640-654): out[b][p][c] = sum_t attn[c/(C/n_head)][b][t][p] *
 * x[b][t][p][c], padded dates dropped when use_pad; attn already at the resolution of x */
int ffa_temporal_aggregate(int dtype, const void* x, const float* attn, const unsigned char* pad, void* out, int B,
                           int T, int P, int C, int n_head, int use_pad, ffa_stream_t stream);
/* TemporallySharedBlock.smart_forward (:420-447): pad[n] = image n is all `value`; padded images come out as `value` */
int ffa_detect_pad_images(const float* x, unsigned char* pad, int N, long long per_image, float value,
                          ffa_stream_t stream);
int ffa_mask_images(int dtype, void* x, const unsigned char* pad, int N, long long per_image, float value,
                    ffa_stream_t stream);
/* -- training of the branch: backward of the pieces above (autograd of multitemp_model.py's modules) -- */
int ffa_reflect_pad1_bwd(int dtype, const void* dpad, void* dx, int N, int H, int W, int C, ffa_stream_t stream);
/* GroupNorm backward, ffa_group_norm's geometry; y = [res +] relu?(GN(x)): the residual's gradient is dy itself.
 * partial f32 [samples][2][C] receives per-sample (sum dy' xhat, sum dy'): the caller sums the rows (ffa_column_sums) */
int ffa_group_norm_bwd(int dtype, const void* x, const void* dy, void* dx, const float* gamma, const float* beta,
                       float* partial, long long samples, int Q, long long stride_hi, long long stride_lo, int inner,
                       long long inner_stride, int C, int groups, float eps, int relu, ffa_stream_t stream);
/* ffa_ltae_attention with the attention dropout of ScaledDotProductAttention (:399): drop f32 [n_head][B][T][P] = 0 or
 * 1 / (1 - p) (nullable); attn = the dropped-out masks (what the reference returns), prob = the clean softmax (kept) */
int ffa_ltae_attention_train(int dtype, const void* k, const void* v, const float* Q, const unsigned char* pad,
                             const float* drop, void* out, float* attn, float* prob, int B, int T, int P, int n_head,
                             int d_k, int d_v, ffa_stream_t stream);
/* its backward: dout [B][P][n_head*d_v], dattn_ext f32 [n_head][B][T][P] (nullable: gradient the aggregators send to the
 * returned masks) -> dk, dv (layouts of k, v) and dq_partial f32 [ffa_ltae_attention_bwd_blocks()][n_head*d_k rounded up to a
 * multiple of 8, zero-filled] (rows to sum, e.g. with ffa_column_sums) */
int ffa_ltae_attention_bwd_blocks(int B, int P, int n_head);
int ffa_ltae_attention_bwd(int dtype, const void* k, const void* v, const float* Q, const unsigned char* pad,
                           const float* drop, const float* prob, const void* dout, const float* dattn_ext, void* dk,
                           void* dv, float* dq_partial, int B, int T, int P, int n_head, int d_k, int d_v,
                           ffa_stream_t stream);
int ffa_temporal_aggregate_bwd(int dtype, const void* x, const float* attn, const unsigned char* pad, const void* dout,
                               void* dx, float* dattn, int B, int T, int P, int C, int n_head, int use_pad,
                               ffa_stream_t stream);
/* y = x * m elementwise (nn.Dropout with a pre-scaled keep mask; its own backward) */
int ffa_mul(int dtype, const void* x, const void* m, void* y, long long n, ffa_stream_t stream);
/* y = (xs[0] + ... + xs[n-1]) / divisor elementwise, 1 <= n <= 4 (host array of device pointers): FusionHandler's
 * case 3, torch.mean(torch.stack([maps of several time-series branches]), dim=0), flair_hub/models/flair_model.py:496-501;
 * with n = 1, divisor = branches: its backward */
int ffa_mean_stack(int dtype, const void* const* xs, int n, float divisor, void* y, long long numel, ffa_stream_t stream);

/* ---- measurement only: kernel timing session.  Between ffa_ktime_begin(max_launches) and ffa_ktime_end() the 3x3 MFMA
 *      launches of the process (ffa_conv_run on the ring operand, ffa_conv_wgrad on 64-channel blocks) carry their
 *      own start / stop events (hipExtLaunchKernelGGL): ffa_ktime_end waits for them and returns, in launch order, the
 *      kernels' durations in milliseconds and a tag (1: ring16 8x32 tiles, 2: ring16 16x16, 4: ring16 128-co blocks,
 *      16: wgrad64); its return value is the number of timed launches.  Not for use under stream capture. */
int ffa_ktime_begin(int max_launches);
int ffa_ktime_end(float* ms, int* tags, int cap);

/* ---- optimizer step: Adam / AdamW over all parameter tensors (csrc/optim.hip).  Replaces torch.optim.AdamW / Adam as
 *      built at flair_hub/tasks/tasks_module.py:385-389 (same update, same state tensors: exp_avg, exp_avg_sq, a
 *      per-parameter device step counter that already counts this update).  Host arrays of device pointers, one entry per
 *      f32 parameter tensor; lr is a device scalar; ceil(n / 72) launches, descriptors ride in the kernel arguments. */
int ffa_adamw_multi(int n_tensors, void* const* p, const void* const* g, void* const* m, void* const* v,
                    const void* const* step, const long long* numel, const float* lr, double beta1, double beta2,
                    float eps, float weight_decay, int decoupled, int maximize, ffa_stream_t stream);

/* ---- Swin-Transformer encoder + UPerNet decoder (the reference's default `swin_*-upernet` architecture:
 *      configs/train/config_models.yaml:5, configs/config_model_zonal_segmentation.yaml:26, resolved through
 *      flair_hub/models/monotemp_model.py:64-92 by smp.create_model("upernet", "tu-swin_...")).
 *      Token tensors are NHWC [B][H][W][C]; evaluation-mode forward. ------------------------------------------- */
#define FFA_ACT_NONE 0
#define FFA_ACT_GELU 1
/* nn.Linear (+ nn.GELU) (+ residual add) on tokens: out[m][n] = act(sum_k a[m][k] w[n][k] + bias[n]) + residual[m][n];
 * w is nn.Linear.weight's own [N][K] layout in the dtype of a.  bf16: MFMA token GEMM (K % 32 == 0, N % 8 == 0, pitches
 * % 8 == 0); f32: plain-FMA parity kernel with the same epilogues (any K, N), for gradient checks, not a speed path. */
int ffa_linear(int dtype, const void* a, long long lda, const void* w, const float* bias, const void* residual,
               long long ldr, void* out, long long ldc, int M, int K, int N, int act, ffa_stream_t stream);
/* The same GEMM with the training-time epilogues: act = FFA_ACT_GELU with `aux` != NULL also stores the (bf16) pre-activation
 * to aux [M][ldaux] (Mlp.fc1, kept for the backward pass); act = FFA_ACT_DGELU multiplies the result by gelu'(aux) (the input
 * gradient of Mlp.fc2 carried through the activation); row_scale[m / rows_per_scale] multiplies the result before the
 * residual add (timm's DropPath: 0 or 1 / keep_prob per sample). */
#define FFA_ACT_DGELU 2
#define FFA_ACT_RELU 3 /* relu(a w^T + bias): a 1x1 convolution with folded BatchNorm + ReLU on tokens */
int ffa_linear_ex(int dtype, const void* a, long long lda, const void* w, const float* bias, const void* residual,
                  long long ldr, void* out, long long ldc, int M, int K, int N, int act, void* aux, long long ldaux,
                  const float* row_scale, int rows_per_scale, ffa_stream_t stream);
/* The kernel ffa_linear_ex launches for a shape (host arithmetic, nothing is launched): 0 f32 parity kernel, 1 bf16
 * 64-token tile, 2 bf16 128-token tile, 3 bf16 256 x 256 tile */
int ffa_linear_plan(int dtype, int M, int K, int N);
/* nn.Linear's weight gradient dW[n][k] = sum_m dy[m][n] x[m][k] (f32 [N][K]; accumulate != 0 adds to dw): transposed-
 * operand MFMA GEMM over the tokens, split over token ranges with a fixed-order reduction (deterministic); f32 operands take
 * a plain-FMA kernel with the same slabs and reduction (parity mode) */
long long ffa_linear_wgrad_workspace_bytes(int M, int N, int K);
int ffa_linear_wgrad(int dtype, const void* x, long long ldx, const void* dy, long long ldy, float* dw,
                     float* dbias /* nullable: [N] column sums of dy from the same pass */, int M, int K, int N,
                     int accumulate, void* workspace, long long workspace_bytes, ffa_stream_t stream);
/* PatchEmbed's Conv2d(kernel = stride = ps) as a gather: out[b][y][x][(dy*ps + dx)*C + c] = in[b][y*ps+dy][x*ps+dx][c] */
int ffa_space_to_depth(int dtype, const void* in, void* out, int B, int Ho, int Wo, int C, int ps, ffa_stream_t stream);
/* nn.LayerNorm(C) over rows of C contiguous channels; stats (nullable) receives (mean, rstd) per row for the backward pass */
int ffa_layer_norm(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* stats, long long rows,
                   int C, float eps, ffa_stream_t stream);
/* PatchMerging's 2x2 gather + nn.LayerNorm(4C): x [B][H][W][C] -> y [B][H/2][W/2][4C] */
int ffa_patch_merge_norm(int dtype, const void* x, void* y, const float* gamma, const float* beta, float* stats, int B,
                         int H, int W, int C, float eps, ffa_stream_t stream);
/* backward of the two: dx, dgamma, dbeta (f32) from x (the forward's input), dy and the forward's row statistics;
 * deterministic (chunk partials in the workspace, summed in a fixed order) */
long long ffa_layer_norm_bwd_workspace_bytes(long long rows, int C);
int ffa_layer_norm_bwd(int dtype, const void* x, const void* dy, const float* gamma, const float* stats,
                       const void* dres /* nullable: added to dx (the residual around the normalised branch) */, void* dx,
                       float* dgamma, float* dbeta, long long rows, int C, void* workspace, long long workspace_bytes,
                       ffa_stream_t stream);
int ffa_patch_merge_norm_bwd(int dtype, const void* x, const void* dy, const float* gamma, const float* stats, void* dx,
                             float* dgamma, float* dbeta, int B, int H, int W, int C, void* workspace,
                             long long workspace_bytes, ffa_stream_t stream);
/* SwinTransformerBlock._attn without the two projections: cyclic shift, padding to the window grid, window partition,
 * softmax(scale q k^T + relative position bias + shift mask) v, window reverse, crop, un-shift -- by index arithmetic on
 * qkv [B][H][W][3C] (channel = which*C + head*32 + d); qkv_bias [3C] is what a padding token projects to;
 * table [(2 ws - 1)^2][heads] is relative_position_bias_table */
int ffa_window_attention(int dtype, const void* qkv, void* out, const float* qkv_bias, const float* table, int B, int H,
                         int W, int C, int heads, int ws, int shift, float scale, ffa_stream_t stream);
/* backward of ffa_window_attention (bf16 MFMA kernel; f32 plain-FMA parity kernel): dqkv [B][H][W][3C] from qkv and dout [B][H][W][C]; dtable [(2 ws - 1)^2][heads]
 * and dbias_pad [3C] (gradient reaching the qkv bias through the padding tokens) are written (per-window partial rows in
 * the workspace, summed in a fixed order; only LDS atomics inside a block) */
long long ffa_window_attention_bwd_workspace_bytes(int B, int H, int W, int C, int heads, int ws);
int ffa_window_attention_bwd(int dtype, const void* qkv, const void* dout, void* dqkv, const float* qkv_bias,
                             const float* table, float* dtable, float* dbias_pad, int B, int H, int W, int C, int heads,
                             int ws, int shift, float scale, void* workspace, long long workspace_bytes,
                             ffa_stream_t stream);
/* nn.GELU() (erf form), elementwise; n a multiple of 8 */
int ffa_gelu(int dtype, const void* x, void* y, long long n, ffa_stream_t stream);
/* nn.AdaptiveAvgPool2d(S) of smp's PSPModule: x [B][H][W][C] -> y [B][S][S][C] */
int ffa_adaptive_avg_pool(int dtype, const void* x, void* y, int B, int H, int W, int C, int S, ffa_stream_t stream);
/* F.interpolate(mode="bilinear", align_corners=...) written into channels [y_off, y_off + C) of y [B][Ho][Wo][y_pitch],
 * plus an optional dense addend [B][Ho][Wo][C] (FPNBlock: upsample + lateral) */
int ffa_bilinear_slice(int dtype, const void* x, const void* addend, void* y, int B, int Hi, int Wi, int Ho, int Wo,
                       int C, int y_pitch, int y_off, int align_corners, ffa_stream_t stream);

/* y[m] = x[m] * row_scale[m / rows_per_scale] (DropPath factor on a gradient ahead of the weight / bias reductions) */
int ffa_scale_rows(int dtype, const void* x, void* y, const float* row_scale, long long rows, int C, int rows_per_scale,
                   ffa_stream_t stream);
/* bilinear x2 followed by bilinear x1/2 (both align_corners=False) as one separable 3-tap filter with replicated edges:
 * UPerNet's placeholder FPN stage + the resize back to stride 4; symmetric, so it is its own backward.  x / y are channel
 * slices [x_off, x_off + C) / [y_off, y_off + C) of tensors with pitches x_pitch / y_pitch and the same [B][H][W] */
int ffa_updown2x_slice(int dtype, const void* x, void* y, int B, int H, int W, int C, int x_pitch, int x_off, int y_pitch,
                       int y_off, ffa_stream_t stream);
/* out[c] = sum_m x[m][c] (f32): nn.Linear's bias gradient, any width; deterministic */
long long ffa_column_sums_workspace_bytes(long long rows, int C);
int ffa_column_sums(int dtype, const void* x, float* out, long long rows, int C, void* workspace,
                    long long workspace_bytes, ffa_stream_t stream);
/* backward of ffa_bilinear_slice w.r.t. x (the addend's gradient is the slice itself) and of ffa_adaptive_avg_pool */
int ffa_bilinear_slice_bwd(int dtype, const void* dy, void* dx, int B, int Hi, int Wi, int Ho, int Wo, int C, int y_pitch,
                           int y_off, int align_corners, ffa_stream_t stream);
int ffa_adaptive_avg_pool_bwd(int dtype, const void* dy, void* dx, int B, int H, int W, int C, int S, ffa_stream_t stream);

/* ---- BatchNorm2d + ReLU + residual, MaxPool2d(3,2,1) (smp ResNet-34 encoder / UnetDecoder blocks;
 *      SURVEY.md Appendix C) ----------------------------------------------------------------------- */
long long ffa_bn_workspace_bytes(int C);
int ffa_bn_stats(int dtype, const void* x, long long npix, int C, const float* gamma, const float* beta,
                 float* running_mean, float* running_var, float momentum, float eps, float* scale, float* shift,
                 float* mean_out, float* rstd_out, void* workspace, long long workspace_bytes, ffa_stream_t stream);
/* ffa_bn_stats without the pass over the tensor: partials[nparts][2][C] come from ffa_conv_run with stats */
int ffa_bn_finalize(const float* partials, long long nparts, long long npix, int C, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                    float* scale, float* shift, float* mean_out, float* rstd_out, void* workspace,
                    long long workspace_bytes, ffa_stream_t stream);
int ffa_bn_eval_params(int C, const float* gamma, const float* beta, const float* running_mean,
                       const float* running_var, float eps, float* scale, float* shift, ffa_stream_t stream);
int ffa_bn_apply(int dtype, const void* x, const void* residual, void* y, const float* scale, const float* shift,
                 long long npix, int C, int relu, ffa_stream_t stream);
/* relu: 0 none, 1 mask from the stored output y, 2 mask recomputed from x (y may be null; no residual) */
int ffa_bn_bwd(int dtype, const void* x, const void* dy, const void* y, const float* gamma, const float* beta,
               const float* mean, const float* rstd, void* dx, void* dres, float* dgamma, float* dbeta, long long npix,
               int C, int relu, void* workspace, long long workspace_bytes, ffa_stream_t stream);
/* ffa_bn_bwd in separate calls: stages bit 0 = reduction + finalize (dgamma, dbeta and the apply coefficients, left in
 * the workspace), bit 1 = apply (dx, dres) from the coefficients of an earlier call on the SAME workspace, bit 2 = the
 * reduction kernel alone, bit 3 = the finalize kernel alone (1 == 4 | 8); 3 = everything.
 * relu 1 with dres: the reduction (bit 0 or 2) writes dres = dy masked by y > 0 and the apply (bit 1) reads x and
 * dres only, so an apply-only call needs the dres that the reduction call of the same arguments left.  dres may be
 * dy itself (in place); it must not overlap x, y or dx (FFA_ERR_ARG).
 * Lets a harness bracket each kernel with its own events (bench.py's HBM roofline entry). */
int ffa_bn_bwd_stages(int dtype, const void* x, const void* dy, const void* y, const float* gamma, const float* beta,
                      const float* mean, const float* rstd, void* dx, void* dres, float* dgamma, float* dbeta,
                      long long npix, int C, int relu, void* workspace, long long workspace_bytes, int stages,
                      ffa_stream_t stream);
/* ffa_bn_bwd as ONE co-resident kernel (bf16): x and the masked dy stay in registers across two grid-wide barriers
 * -- three passes over memory instead of five, one launch instead of three.  sync = four uint32 of device memory,
 * zero before the first call and owned by the library afterwards (sync[3] != 0: a barrier timed out, results of
 * that call are invalid).  FFA_ERR_UNSUPPORTED when dy + x do not fit the chip's register files (use ffa_bn_bwd). */
int ffa_bn_bwd_fused(int dtype, const void* x, const void* dy, const void* y, const float* gamma, const float* beta,
                     const float* mean, const float* rstd, void* dx, void* dres, float* dgamma, float* dbeta,
                     long long npix, int C, int relu, void* workspace, long long workspace_bytes, unsigned* sync,
                     ffa_stream_t stream);
/* ffa_bn_bwd (ReLU mask recomputed from x) when sum(g) / sum(g*x) per tile already exist (ffa_conv_run with bnx) */
int ffa_bn_bwd_partials(int dtype, const void* x, const void* dy, const float* partials, long long nparts,
                        const float* gamma, const float* beta, const float* mean, const float* rstd, void* dx,
                        float* dgamma, float* dbeta, long long npix, int C, void* workspace, long long workspace_bytes,
                        ffa_stream_t stream);
int ffa_channel_sums(int dtype, const void* x, long long npix, int C, float* sum_out, float* sumsq_out,
                     void* workspace, long long workspace_bytes, ffa_stream_t stream);
int ffa_maxpool3x3s2_fwd(int dtype, const void* x, void* y, uint8_t* idx, int B, int H, int W, int C,
                         ffa_stream_t stream);
/* add (optional, shape of dx): a second gradient of the same tensor, e.g. the U-Net skip branch of the stem output */
int ffa_maxpool3x3s2_bwd(int dtype, const void* dy, const uint8_t* idx, const void* add, void* dx, int B, int H, int W,
                         int C, ffa_stream_t stream);

/* ---- layout hand-over at the model boundary (batch dict tensors are NCHW f32:
 *      flair_hub/data/dataloader.py:105-257, flair_zonal_detection/dataset.py:174-209) -------------- */
int ffa_nchw_to_nhwc(int dtype, const float* src, void* dst, int B, int C, int H, int W, int Cp, ffa_stream_t stream);
/* uint8 NCHW raster tiles -> (x - mean[c]) / std[c] as NHWC compute tensor (the zonal dataset's normalisation,
 * flair_hub/data/utils_data/norm.py:37-44 reached from flair_zonal_detection/dataset.py:174-209, done on the device) */
int ffa_u8_nchw_to_nhwc(int dtype, const uint8_t* src, void* dst, int B, int C, int H, int W, int Cp,
                        const float* mean, const float* stdv, ffa_stream_t stream);
/* the same pass for the other sample types rasters come in (uint16 SPOT / Sentinel reflectances, int16, float32
 * elevation models): dst = (src - mean[c]) / std[c] */
#define FFA_SRC_U8 0
#define FFA_SRC_U16 1
#define FFA_SRC_I16 2
#define FFA_SRC_F32 3
int ffa_raw_nchw_to_nhwc(int dtype, int src_kind, const void* src, void* dst, int B, int C, int H, int W, int Cp,
                         const float* mean, const float* stdv, ffa_stream_t stream);
int ffa_nhwc_to_nchw(int dtype, const void* src, float* dst, int B, int C, int H, int W, int Cp, ffa_stream_t stream);

/* ---- training augmentation inside the layout / label passes (flair_hub/data/utils_data/augmentations.py:6-48):
 *      per-sample flips and rotations by k * 90 degrees as a gather on the read side.  codes: uint8 on the device, one
 *      per sample, bit 0 horizontal flip, bit 1 vertical flip, bits 2-3 k (masked with 15); the reference's order (flip
 *      axis -1, flip axis -2, rot90(k)): out[i][j] = in[si][sj], (si, sj) = (i, j), k times (si, sj) <- (sj, n-1-si),
 *      vflip: si <- n-1-si, hflip: sj <- n-1-sj.  Planes must be square (H == W). */
/* The work of ffa_nchw_to_nhwc / ffa_u8_nchw_to_nhwc / ffa_raw_nchw_to_nhwc with that gather: src_kind FFA_SRC_*; mean and
 * stdv both null (FFA_SRC_F32 only) = plain layout without normalisation; image b reads codes[b / group] (group = T for a
 * [B,T,C,h,w] series viewed as B*T images).  Bit-identical to the plain kernel run on a pre-permuted input. */
int ffa_d4_nchw_to_nhwc(int dtype, int src_kind, const void* src, void* dst, int B, int C, int H, int W, int Cp,
                        const float* mean, const float* stdv, const uint8_t* codes, int group, ffa_stream_t stream);
int ffa_d4_labels_u8(const uint8_t* src, uint8_t* dst, int B, int H, int W, const uint8_t* codes, ffa_stream_t stream);
/* ffa_onehot_to_index (first maximum) of the permuted one-hot map */
int ffa_d4_onehot_to_index(const float* onehot, uint8_t* idx, int B, int K, int H, int W, const uint8_t* codes,
                           ffa_stream_t stream);

/* ---- decoder resampling (smp DecoderBlock nearest x2 + cat; flair_model.py:318-327 interpolate_map) */
int ffa_upsample_nearest2x_concat_fwd(int dtype, const void* lo, const void* skip, void* out, int B, int Hl, int Wl,
                                      int C1, int C2, ffa_stream_t stream);
/* dskip may be null: only dlo (2x2 sums of the first C1 channels) is written and the caller uses dcat[..., C1:] */
int ffa_upsample_nearest2x_concat_bwd(int dtype, const void* dcat, void* dlo, void* dskip, int B, int Hl, int Wl,
                                      int C1, int C2, ffa_stream_t stream);
int ffa_bilinear_fwd(int dtype, const void* x, void* y, int B, int Hi, int Wi, int Ho, int Wo, int C,
                     ffa_stream_t stream);
/* backward in gather form (each source value sums its destination footprint in a fixed order); the workspace
 * arguments are kept for ABI stability: the query returns 0 and workspace may be null */
long long ffa_bilinear_bwd_workspace_bytes(int B, int Hi, int Wi, int C);
int ffa_bilinear_bwd(int dtype, const void* dy, void* dx, int B, int Hi, int Wi, int Ho, int Wo, int C,
                     void* workspace, long long workspace_bytes, ffa_stream_t stream);

/* ---- loss / prediction (flair_hub/tasks/module_setup.py:150-161 CrossEntropyLoss(weight);
 *      flair_hub/tasks/tasks_module.py:153,155,158; flair_zonal_detection/inference.py:300;
 *      flair_zonal_detection/postprocess.py:9-30) --------------------------------------------------- */
long long ffa_softmax_ce_workspace_bytes(void);
int ffa_softmax_ce(int dtype, const void* logits, const uint8_t* targets, const float* class_weights,
                   const float* grad_scale, float* loss, float* wsum_out, void* dlogits, uint8_t* pred,
                   long long npix, int K, int Cp, void* workspace, long long workspace_bytes, ffa_stream_t stream);
/* ffa_softmax_ce that also returns dlogit_sums[Cp]: per class, the sum over all pixels of the dlogits values it wrote
 * = the bias gradient of the convolution that produced the logits (torch: grad of segmentation_head.0.bias,
 * flair_hub/models/checkpoint.py:226), taken in the same pass instead of a column-sum pass over dlogits.  Needs dlogits
 * and 16-byte aligned tensors; FFA_ERR_UNSUPPORTED otherwise (then: ffa_channel_sums over dlogits). */
int ffa_softmax_ce_sums(int dtype, const void* logits, const uint8_t* targets, const float* class_weights,
                        const float* grad_scale, float* loss, float* wsum_out, void* dlogits, uint8_t* pred,
                        float* dlogit_sums, long long npix, int K, int Cp, void* workspace, long long workspace_bytes,
                        ffa_stream_t stream);

/* x[0..n) *= scale[0] in place, scale a device scalar; a no-op pass when the scalar is exactly 1.  Used on the
 * dlogits ffa_softmax_ce wrote in the forward pass (for an upstream gradient of 1) when autograd hands the loss a
 * different grad_output -- replaces the second softmax pass torch.autograd would make (tasks_module.py:155). */
int ffa_scale_inplace(int dtype, void* x, long long n, const float* scale, ffa_stream_t stream);
/* Margin crop (y0, x0, h, w) + uint8 conversion of NHWC logits [B][H][W][Cp] (K classes, pitch Cp a multiple of 8):
 * mode 0: out [B][h][w] = argmax (first maximum); mode 1: out [B][K][h][w] = rint(softmax * 255), half to even;
 * mode 2: out [B][2][h][w] = the argmax plane of mode 0 and a confidence plane = rint(255 * largest softmax
 * probability), bit for bit the maximum over the K bands mode 1 writes for the pixel, in one pass over the logits. */
int ffa_predict_u8(int dtype, int mode, const void* logits, uint8_t* out, int B, int H, int W, int K, int Cp, int y0,
                   int x0, int h, int w, ffa_stream_t stream);
/* Test-time augmentation: a tile predicted under several flips / rotations ("views", the codes of ffa_d4_nchw_to_nhwc:
 * bit 0 horizontal flip, bit 1 vertical flip, bits 2-3 k of rot90), the softmax probabilities averaged in the tile's
 * own frame.  `logits` is ONE view's NHWC tensor [B][H][W][Cp] (bf16 or f32, K classes, H == W, else
 * FFA_ERR_UNSUPPORTED) in the VIEW's frame, `code` (0..15, one host int: all samples of a launch share it) the forward
 * code that made the view.  For every pixel (y0 + y, x0 + x) of the crop window, stated in the TILE's frame, the kernel
 * finds the pixel's position in the view (the gather of the inverse transform), takes the softmax there in the
 * arithmetic of ffa_predict_u8 mode 1 (f32: maximum, expf(z - m), sum in class order, e / se) and stores it into the
 * accumulator (first != 0) or adds it (first == 0).
 * Accumulator layout: f32, pixel-major over the crop window at the logits' pitch, acc[B][h][w][Cp], 16-byte aligned;
 * the pad channels K..Cp-1 hold 0.  One thread owns an element and views add up in call order: no atomics, equal
 * calls give equal bytes.  Both the logits and the accumulator are moved in whole runs of consecutive bytes for every
 * code (the transposition of odd k happens in LDS). */
int ffa_tta_accumulate(int dtype, const void* logits, float* acc, int B, int H, int W, int K, int Cp, int y0, int x0,
                       int h, int w, int code, int first, ffa_stream_t stream);
/* The outputs of ffa_predict_u8 from an accumulator of `views` (>= 1) views, computed on p = acc / (float)views:
 * mode 0: out [B][h][w] = first maximum of p; mode 1: out [B][K][h][w] = rintf(p * 255.f); mode 2: out [B][2][h][w] =
 * the label plane of mode 0 and rintf(255 * max p), bit for bit the maximum over the mode-1 bands of the pixel.  With
 * one identity view (code 0, first != 0, views 1) all three equal ffa_predict_u8's outputs bit for bit. */
int ffa_tta_predict_u8(int mode, const float* acc, uint8_t* out, int B, int K, int Cp, int h, int w, int views,
                       ffa_stream_t stream);
/* The mean probabilities themselves: out f32 [B][K][h][w] = acc / (float)views */
int ffa_tta_probabilities(const float* acc, float* out, int B, int K, int Cp, int h, int w, int views,
                          ffa_stream_t stream);
int ffa_onehot_to_index(const float* onehot, uint8_t* idx, int B, int K, int H, int W, ffa_stream_t stream);
/* counts[target][pred] += 1 (int64, accumulating): the IoU-metric state of tasks_module.py:210-212 */
int ffa_confusion_matrix(const uint8_t* pred, const uint8_t* target, long long n, int K, long long* counts,
                         ffa_stream_t stream);
/* The evaluation entry points (labels, confusion counts and per-class loss sums from one pass over the logits) are
 * declared in flairhip_eval.h, which this header brings along. */
#include "flairhip_eval.h"
/* The sample-store entry points (a batch gathered by index from raw samples resident on the device, with the layout
 * pass, the elevation pre-processing and the label rule on the way) are declared in flairhip_gather.h, likewise. */
#include "flairhip_gather.h"
/* The ragged time-series store (the padded U-TAE batch and its pad flags gathered by index from series of variable
 * length resident on the device) is declared in flairhip_series.h, likewise. */
#include "flairhip_series.h"
/* Calibrated class thresholds (per-class histograms of the score bytes over a validation split, and the label /
 * confidence outputs of ffa_predict_u8 and ffa_tta_predict_u8 under per-class thresholds) are declared in
 * flairhip_calib.h, likewise. */
#include "flairhip_calib.h"
/* Object matching (the overlaps between the regions of two class rasters: region tables and the list of region pairs
 * that share pixels, with the size of each intersection) is declared in flairhip_objects.h, likewise. */
#include "flairhip_objects.h"
/* Zonal statistics (for a layer of zones over a class raster: the pixel count per zone and class, and the sum of a
 * confidence raster over the same pixels) are declared in flairhip_zonestats.h, likewise. */
#include "flairhip_zonestats.h"
/* Land-cover change (for two class rasters on one grid: the class transition matrix per zone over the same zone
 * tables, and a recode of the two rasters into one raster of change codes) is declared in flairhip_change.h,
 * likewise. */
#include "flairhip_change.h"

/* ---- host-side tile bookkeeping, bit-exact with the reference's float64 arithmetic
 *      (flair_zonal_detection/slicing.py:51-112, flair_zonal_detection/inference.py:318-335) -------- */
typedef struct {
  double left, bottom, right, top; /* kept area (margins removed, clipped to the zone) */
  double x0, y0, x1, y1;           /* full tile box */
  long long row, col;              /* id = "1-{row}-{col}" */
} ffa_tile_t;
/* returns the number of tiles (<= capacity written to out; call with capacity 0 to count), < 0 on error.
 * clamp_is_pyfloat: 1 when the zone bounds are Python floats (rasterio array_bounds), which selects
 * Python's correctly-rounded round(v, 6) for clamped coordinates in the duplicate filter. */
long long ffa_slice_grid(double min_x, double min_y, double max_x, double max_y, double ref_left, double ref_bottom,
                         int patch_size, int margin, double resolution, ffa_tile_t* out, long long capacity);
typedef struct {
  int col_off, row_off, width, height; /* rasterio Window */
  int skip;                            /* 1 when the clipped window is empty */
} ffa_window_t;
int ffa_write_window(double left, double top, double img_left, double img_bottom, double img_right, double img_top,
                     double out_res, int pred_h, int pred_w, ffa_window_t* out);

/* ---- GeoTIFF block codecs (host side, no GPU): flair_zonal_detection/geotiff.py -------------------- */
/* The reference reads its input rasters and writes its LZW-compressed uint8 prediction rasters through
 * rasterio / GDAL / libtiff (flair_zonal_detection/dataset.py:89-117, inference.py:157-208 "compress": "lzw",
 * :342-352 dst.write).  These are the per-block byte codecs of that format: libtiff-compatible LZW (MSB-first
 * codes, early width change, table reset at 4094 entries) and the Predictor = 2 horizontal differencing. */
long long ffa_tiff_lzw_bound(long long n);
/* returns bytes written (stops at EndOfInformation, end of input or cap), < 0 on a corrupt stream */
long long ffa_tiff_lzw_decode(const uint8_t* src, long long n, uint8_t* dst, long long cap);
/* returns the encoded size, FFA_ERR_WORKSPACE when cap < what the stream needs (ffa_tiff_lzw_bound(n) suffices) */
long long ffa_tiff_lzw_encode(const uint8_t* src, long long n, uint8_t* dst, long long cap);
/* in place over rows x row_samples native-endian samples of sample_bytes (1, 2, 4); stride = samples between
 * horizontal neighbours of one band; undo != 0 accumulates (read), 0 differences (write) */
int ffa_tiff_hpredict(void* buf, long long rows, long long row_samples, int sample_bytes, int stride, int undo);

/* ---- polygonisation of a class raster (flair_zonal_detection/inference.py raster_to_polygons) ------------------ */
/* The reference turns the uint8 prediction raster into polygons with rasterio.features.shapes (GDAL's polygonizer) once
 * per class, 4-connected, then shapely's simplify(preserve_topology=True) (inference.py:359-413).  Here: one polygon per
 * 4-connected component of equal class (all classes in one pass), pixel-corner vertices as exact integers.
 * Two phases keep the ABI rules (no synchronisation, caller workspace) although the output size depends on the data:
 *   1. ffa_polygonize_label runs everything up to the sizes and writes counts_dev[4] (int64, device memory):
 *      polygons P, rings R, vertices V, boundary edges;
 *   2. the caller reads the counts, allocates the outputs and calls ffa_polygonize_emit with them (same workspace,
 *      untouched in between, same stream):
 *        poly_class[P] (int32), poly_pixels[P] (int64), poly_ring_offsets[P + 1] (int32, rings of polygon q are
 *        poly_ring_offsets[q] .. [q + 1] - 1), ring_vertex_offsets[R + 1] (int32), vertices[V][2] (int32 col, row).
 * Polygons are sorted by (class, label = row-major index of the component's first pixel); the first ring of a polygon
 * is its exterior, then its holes in ring-id order (ring id = the smallest boundary edge id 4 * pixel + side on the
 * ring); a ring starts at the first direction change at or after its ring-id edge's start corner and is not closed
 * (no repeated first vertex), has no collinear or repeated vertices and is simple; exteriors are counter-clockwise and
 * holes clockwise in map coordinates (x = col, y = -row).  A component touching itself diagonally gives an exterior
 * and a hole that meet at one vertex.  Components with fewer than min_pixels pixels are dropped; background = -1 makes
 * every value a class.  Deterministic: equal inputs give equal bytes.  Limit: 4 * H * W < 2^31. */
long long ffa_polygonize_workspace_bytes(int H, int W); /* < 0 (FFA_ERR_ARG) beyond the limit */
int ffa_polygonize_label(const uint8_t* classes, int H, int W, int background, long long min_pixels, void* ws,
                         long long ws_bytes, long long* counts_dev, ffa_stream_t stream);
int ffa_polygonize_emit(const void* ws, long long ws_bytes, int H, int W, long long n_polys, long long n_rings,
                        long long n_vertices, int32_t* poly_class, int64_t* poly_pixels, int32_t* poly_ring_offsets,
                        int32_t* ring_vertex_offsets, int32_t* vertices, ffa_stream_t stream);
/* Optional, after ffa_polygonize_label on the same untouched workspace and stream, before or after
 * ffa_polygonize_emit (it reads the labels and the polygon index, which emit leaves alone; the workspace size is
 * unchanged): sums[q] = the exact sum of values[H][W] (uint8, device) over the pixels of polygon q, in the polygon
 * order of ffa_polygonize_emit; sums[n_polys] (int64, device) is written, not accumulated.  Background pixels and
 * components dropped by min_pixels contribute nowhere.  Integer atomics only: equal inputs give equal bytes.
 * n_polys = counts_dev[0]; with n_polys == 0 nothing is written. */
int ffa_polygonize_zonal_sum_u8(const void* ws, long long ws_bytes, int H, int W, const uint8_t* values,
                                long long n_polys, int64_t* sums, ffa_stream_t stream);
/* The count-sized path: the same polygons from workspaces sized by what the raster holds, for rasters beyond
 * 4 * H * W < 2^31 and for the many below it where a workspace of 184 bytes per pixel is mostly never touched.
 * Normative: for every input both paths accept, poly_class, poly_pixels, poly_ring_offsets, ring_vertex_offsets,
 * vertices and the zonal sums are byte-identical to those of ffa_polygonize_label / _emit / _zonal_sum_u8 (same
 * order, ring starts and winding; everything said above holds).  Four steps, one host synchronisation more:
 *   1. ffa_polygonize_count labels the raster and counts: counts_dev[2] (int64, device) = boundary edges E (a side of
 *      a pixel of a kept component whose other side is outside the raster or in another component; accumulated in
 *      64 bits, so a value of 2^31 or more is reported, never wrapped) and polygons P.  Its pixel workspace ws_px
 *      holds labels, pixel counts, edge offsets and the polygon index: ffa_polygonize_count_bytes(H, W) <=
 *      16 * H * W + 2 MiB.  Host only: no device memory is touched by either size function.
 *   2. the caller reads E and P.  E == 0 or P == 0: there are no polygons and nothing more to call.  Else
 *      ffa_polygonize_trace_bytes(E, P) is the size of the trace workspace ws_tr, a function of E and P only:
 *      seven int32 arrays of E + 1, the ring arrays by the ring bound E / 4 (a ring has at least 4 edges), the polygon
 *      arrays and radix buffers by max(P, E / 4); about 42 bytes per edge, at most 48 * E + 64 * P + 64 KiB.
 *   3. ffa_polygonize_trace(the classes, H, W and min_pixels of step 1, ws_px untouched since, E, P, ws_tr) traces
 *      the rings in ceil(log2 max(E, 2)) pointer-jumping rounds and writes counts_dev[4] like ffa_polygonize_label:
 *      P, R, V, E.  E and P must be the values step 1 wrote: they size what the kernels index.
 *   4. ffa_polygonize_counted_emit and, optionally, ffa_polygonize_counted_zonal_sum_u8 on the pair of workspaces,
 *      with the outputs and the rules of ffa_polygonize_emit / ffa_polygonize_zonal_sum_u8.
 * Limits: H * W < 2^30 (FFA_ERR_ARG from ffa_polygonize_count_bytes and ffa_polygonize_count); E < 2^31 - 1, which
 * also keeps V <= E below 2^31 (FFA_ERR_ARG from ffa_polygonize_trace_bytes and every later call, with the numbers
 * in ffa_last_error, before anything sized by E exists).  Edge ids 4 * pixel + side are unsigned 32-bit throughout;
 * labels, compact edge indices, ring and vertex numbers are below 2^31.  All calls on one stream. */
long long ffa_polygonize_count_bytes(int H, int W); /* < 0 (FFA_ERR_ARG) beyond the limit */
int ffa_polygonize_count(const uint8_t* classes, int H, int W, int background, long long min_pixels, void* ws_px,
                         long long ws_px_bytes, long long* counts_dev, ffa_stream_t stream);
long long ffa_polygonize_trace_bytes(long long n_edges, long long n_polys); /* < 0 (FFA_ERR_ARG) beyond the limits */
int ffa_polygonize_trace(const uint8_t* classes, int H, int W, long long min_pixels, void* ws_px,
                         long long ws_px_bytes, long long n_edges, long long n_polys, void* ws_tr,
                         long long ws_tr_bytes, long long* counts_dev, ffa_stream_t stream);
int ffa_polygonize_counted_emit(const void* ws_px, long long ws_px_bytes, int H, int W, const void* ws_tr,
                                long long ws_tr_bytes, long long n_edges, long long n_polys, long long n_rings,
                                long long n_vertices, int32_t* poly_class, int64_t* poly_pixels,
                                int32_t* poly_ring_offsets, int32_t* ring_vertex_offsets, int32_t* vertices,
                                ffa_stream_t stream);
int ffa_polygonize_counted_zonal_sum_u8(const void* ws_px, long long ws_px_bytes, int H, int W, const void* ws_tr,
                                        long long ws_tr_bytes, long long n_edges, const uint8_t* values,
                                        long long n_polys, int64_t* sums, ffa_stream_t stream);
/* Host only: topology-preserving Douglas-Peucker (shapely / JTS TopologyPreservingSimplifier semantics within each
 * polygon; csrc/polygon_simplify.cpp) over float64 map coordinates xy[V][2] laid out as above; keep[V] receives 1 for
 * the vertices that stay.  tolerance 0 keeps all; n_threads (1 .. 16) splits the polygons between host threads. */
int ffa_polygon_simplify(const double* xy, const int32_t* ring_offsets, const int32_t* poly_ring_offsets,
                         long long n_polys, double tolerance, int n_threads, uint8_t* keep);

/* ---- sieve filter on a class raster (the gdal_sieve / rasterio.features.sieve companion of the polygoniser) -------- */
/* In place over classes[H][W] (uint8, device): regions below a size are merged into their greatest neighbour, so the
 * map stays a coverage with no gaps -- where ffa_polygonize_label(min_pixels) only drops them and leaves a hole.
 * 4-connected like the polygoniser; exact and independent of the block schedule.
 *
 * Definition (normative).  A component is a 4-connected set of pixels of equal class that are not `background`
 * (-1: every value is a class); its root is its smallest row-major pixel index (the polygoniser's label); it is small
 * when it has fewer than min_pixels pixels.  Two components are neighbours when a pixel of one shares a side with a
 * pixel of the other (corners do not count).  key(C) = (pixel count, -root), compared lexicographically: more pixels
 * win, at equal counts the smaller root wins.  One call runs ONE round, every step on the state at its start:
 *   1. label the raster, count the pixels per root;
 *   2. for each small component S: best(S) = the neighbour of S with the greatest key (background is no neighbour);
 *   3. S is relabelled when best(S) exists and key(best(S)) > key(S); its new class is the class best(S) had at the
 *      start of the round, even when best(S) is small itself and relabelled in the same round;
 *   4. all relabelled components are written at once.
 * Background pixels never change and are never a target; a component that is not small at the start of a round keeps
 * its class in that round.  The key travels as one unsigned 64-bit word, count << 32 | (0x7FFFFFFF - root), through a
 * 64-bit atomicMax: the limit 4 * H * W < 2^31 keeps both fields in range, and a maximum does not depend on the order
 * of its arguments, so equal inputs give equal bytes.
 * counts_dev[4] (int64, device memory, written): components that were small at the start of the round, components
 * relabelled, pixels relabelled, components in all (at the start).  The caller reads them and repeats the call until
 * a round relabels nothing; each round that relabels something removes at least one component, so that ends.  A
 * small component may remain at the end: one with no neighbour (alone in the raster or enclosed by background), or
 * the greatest of its neighbourhood.  min_pixels <= 1: nothing is small, the call only labels and counts
 * (counts_dev = 0, 0, 0, components).  Workspace contents are irrelevant on entry. */
long long ffa_sieve_workspace_bytes(int H, int W); /* < 0 (FFA_ERR_ARG) beyond 4 * H * W < 2^31 */
int ffa_sieve_round_u8(uint8_t* classes, int H, int W, int background, long long min_pixels, void* ws,
                       long long ws_bytes, long long* counts_dev, ffa_stream_t stream);

/* ---- geozone clipping on the pixel grid (flair_zonal_detection/zone.py, raster_to_polygons(zone=, classes=)) ------ */
/* The reference clips its polygons to the zone contour in vector space (shapely intersection).  Here the zone is
 * rasterised on the class raster's own grid and applied before polygonisation: a pixel belongs to the zone when its
 * centre is inside the contour (rasterio.mask.mask / GDAL rasterize with all_touched = False), which keeps the
 * polygoniser's integer vertices, valid rings and byte-equal outputs.
 *
 * Definition (normative).  Rings arrive in pixel coordinates as float64 pairs xy_pix[V][2] = (px, py) with
 * px = (x - left) / xres, py = (top - y) / yres; ring k owns the vertices ring_offsets[k] .. ring_offsets[k + 1] - 1
 * (int32, ring_offsets[n_rings] = V), need not be closed and may have either orientation; holes are further rings:
 * the rule is even-odd over all rings of one call.  For an edge (x0, y0) -> (x1, y1) with y0 != y1 (the last vertex
 * of a ring connects to its first) and a row r with yc = r + 0.5:
 *   - the edge crosses the row iff (y0 <= yc) != (y1 <= yc);
 *   - xc = x0 + ((yc - y0) * (x1 - x0)) / (y1 - y0), every operation rounded separately in IEEE float64 (no fma);
 *   - the crossing toggles column c0 = floor(xc - 0.5) + 1, clamped to [0, W]; a toggle at W has no effect;
 *   - inside(r, c) = XOR of the toggles of row r at columns <= c.
 * A box with corners on the pixel centres (10.5, 20.5) and (30.5, 40.5) covers rows 20..39 and columns 11..30.
 * Edges with a non-finite coordinate are ignored.
 *
 * ffa_zone_mask_u8 writes mask[H][W] (uint8, 0 / 1); with accumulate != 0 it ORs into the existing mask instead (one
 * call per polygon gives the union of a MultiPolygon).  All pointers are device memory; the workspace
 * (ffa_zone_mask_workspace_bytes(H, W, V) bytes, contents irrelevant on entry) also bounds the vertices the kernels
 * read: vertices beyond the count it was sized for are ignored.  XOR atomics on single bits: equal inputs give equal
 * bytes.
 * ffa_zone_clip_u8: classes[i] = mask[i] ? lut256[classes[i]] : fill, in place over n pixels.  mask == NULL: every
 * pixel is inside (a class filter alone); lut256 == NULL: the identity.  lut256 is 256 bytes of device memory.
 * ffa_zone_window_counts: counts[k] (int64, device, written) = the number of non-zero mask pixels in rows
 * windows[k][0] .. windows[k][2] - 1 and columns windows[k][1] .. windows[k][3] - 1 (int32 (r0, c0, r1, c1), device),
 * clamped to the raster; empty or inverted rectangles give 0. */
long long ffa_zone_mask_workspace_bytes(int H, int W, long long n_vertices); /* < 0 (FFA_ERR_ARG) on bad arguments */
int ffa_zone_mask_u8(const double* xy_pix, const int32_t* ring_offsets, int n_rings, int H, int W, uint8_t* mask,
                     int accumulate, void* ws, long long ws_bytes, ffa_stream_t stream);
int ffa_zone_clip_u8(uint8_t* classes, const uint8_t* mask, const uint8_t* lut256, long long n, int fill,
                     ffa_stream_t stream);
int ffa_zone_window_counts(const uint8_t* mask, int H, int W, const int32_t* windows, int n_windows, int64_t* counts,
                           ffa_stream_t stream);

/* ---- coordinate reference systems: points from one CRS to another (flair_zonal_detection/crs.py) ------------------ */
/* One elementwise pass over float64 points in[n][2] = (x, y) -> out[n][2] (device memory, 16-byte aligned; in == out
 * is allowed, partial overlap is not).  A transform is the source CRS's step to geodetic (longitude, latitude) in
 * radians followed by the destination CRS's step from it; projected -> projected runs both in the one pass.
 *
 * FfaCrs (angles in degrees, lengths in metres; fields a method does not use are ignored):
 *   FFA_CRS_GEOGRAPHIC  x = longitude, y = latitude in degrees (the always_xy order), nothing else is read
 *   FFA_CRS_LCC2SP      Lambert conformal conic with two standard parallels lat1, lat2 (EPSG method 9802), origin
 *                       (lon0, lat0), false easting / northing
 *   FFA_CRS_TMERC       transverse Mercator (EPSG method 9807) by the Krueger series in the third flattening through
 *                       n^6 (Karney 2011), origin (lon0, lat0), scale k0 on the central meridian
 * with the ellipsoid (a, inv_flattening) of the CRS itself.
 *
 * Datum rule (normative).  Every supported CRS sits on GRS80 or WGS 84, and geodetic longitude and latitude are carried
 * across unchanged between the two datums: the EPSG registry's RGF93 -> WGS 84 operation is the null transformation
 * (as are the RGAF09 / RGR92 / RGFG95 / RGM04 / RGSPM06 ones), which is what PROJ applies for EPSG:2154 -> EPSG:4326.
 * Each projection uses the ellipsoid of its own CRS.  Hence geographic -> geographic is the identity.
 *
 * The inverse latitude is the fixed point sin(lat) = tanh(psi + e atanh(e sin(lat))) of the isometric latitude psi,
 * iterated a fixed 8 times (no data-dependent exit).  A point with a non-finite coordinate, a geographic latitude
 * beyond +-90 degrees, a conic radius of 0 or a non-finite result comes out as (NaN, NaN); a thread reads and writes
 * its own point only.  No atomics: equal inputs give equal bytes.  The constants derived from FfaCrs (eccentricity,
 * cone constant, rectifying radius, series coefficients) are computed once per call on the host in float64. */
#define FFA_CRS_GEOGRAPHIC 0
#define FFA_CRS_LCC2SP 1
#define FFA_CRS_TMERC 2
typedef struct {
  int kind;              /* FFA_CRS_* */
  double a;              /* semi-major axis */
  double inv_flattening; /* 298.257222101 (GRS80), 298.257223563 (WGS 84) */
  double lon0, lat0;     /* origin: central meridian, latitude of origin */
  double lat1, lat2;     /* standard parallels (LCC2SP) */
  double k0;             /* scale factor on the central meridian (TMERC) */
  double false_easting, false_northing;
} FfaCrs;
int ffa_crs_transform_f64(const double* in, double* out, long long n, const FfaCrs* src, const FfaCrs* dst,
                          ffa_stream_t stream);

/* ---- overview pyramid of a uint8 raster (the reduced-resolution images of a cloud-optimised GeoTIFF) --------------- */
/* Definition (normative).  base is uint8 [bands][H][W] in device memory.
 *   - Sizes.  Level 0 is the base; level l >= 1 has H_l = ceil(H / 2^l) rows and W_l = ceil(W / 2^l) columns.
 *   - Storage.  pyr holds the levels 1 .. levels back to back, each [bands][H_l][W_l], dense
 *     (ffa_overview_pyramid_bytes(bands, H, W, levels) bytes).
 *   - Level count.  ffa_overview_levels returns the smallest L >= 0 with max(H_L, W_L) <= block: GDAL's COG driver
 *     stops adding overviews once the smallest fits one block.
 *   - Block structure.  Bands are independent.  Pixel (r, c) of level l is computed from the block of level l - 1 at
 *     rows 2r .. min(2r + 1, H_{l-1} - 1) and columns 2c .. min(2c + 1, W_{l-1} - 1): n = 1, 2 or 4 pixels.
 *   - method 0, nearest: the block's top-left pixel; level l pixel (r, c) therefore equals base (r * 2^l, c * 2^l),
 *     which is always in range.
 *   - method 1, mode: the value occurring most often in the block, among equally frequent values the smallest.  With
 *     ignore >= 0 pixels equal to ignore do not vote, and a block made only of them gives ignore; ignore = -1: every
 *     value votes.  For class rasters; the zone clip's 255 is what ignore is for.
 *   - method 2, average: (2 s + n) / (2 n) in integer arithmetic, s the sum of the block -- the mean rounded half up,
 *     exact.  ignore must be -1.  For class-probability and confidence rasters.
 *   - Cascade.  Mode and average cascade: level l comes from level l - 1, not from the base.
 *   - Determinism.  Integer arithmetic only, every output byte has one writer: equal inputs give equal bytes.
 *   - Limits.  bands * H * W < 2^31, 0 <= levels <= 30 (levels beyond the 1 x 1 one repeat it; levels = 0 writes
 *     nothing).  Bad arguments return FFA_ERR_ARG (the two size queries return it as their value).
 * One launch writes up to four levels from one read of its source (csrc/overview.hip); the bytes are those of a
 * level-by-level chain. */
int ffa_overview_levels(int H, int W, int block);
long long ffa_overview_pyramid_bytes(int bands, int H, int W, int levels);
int ffa_overview_pyramid_u8(const uint8_t* base, uint8_t* pyr, int bands, int H, int W, int levels, int method,
                            int ignore, ffa_stream_t stream);

/* ---- hardware layout probes (tests only) ---------------------------------------------------------- */
int ffa_probe_tr16(const uint16_t* src, uint16_t* dst, ffa_stream_t stream);
int ffa_probe_mfma(const float* A, const float* B, float* D, int use_f32, ffa_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* FLAIRHIP_H */
