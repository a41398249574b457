/*
 * vlnce_hip.h -- C ABI of libvlnce_hip.so: hand-written CDNA4 (gfx950) kernels
 * for VLN-CE's per-step policy hot path (vlnce_baselines/models/ of the
 * reference).  The reference is pure Python on torch/cuDNN and has no FFI of
 * its own; each entry point below names the torch operator call site in the
 * reference that it replaces (file:line relative to /root/reference).
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on error; the message is
 *     available through vlnce_last_error() (thread-local).
 *   - all pointers are DEVICE pointers valid on `stream`; the library never
 *     allocates, never synchronises and never reads the environment.  Its only
 *     mutable state is the thread-local error string and the process-wide
 *     dispatch options below (vlnce_set_option), which select between kernels
 *     that compute the same function.  Workspaces are caller-allocated.
 *   - activations are fp32, channels-last: images [N,H,W,C], matrices row-major.
 *   - `stream` is a hipStream_t passed as void* (0 = default stream).
 */
#ifndef VLNCE_HIP_H
#define VLNCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* vlnce_stream_t;

enum { VLNCE_ACT_NONE = 0, VLNCE_ACT_RELU = 1, VLNCE_ACT_SIGMOID = 2, VLNCE_ACT_TANH = 3 };

int vlnce_version(void); /* major*100 + minor; 155 = this header */
int vlnce_option_count(void);              /* length of vlnce_prologue.options                        */
int vlnce_option_index(const char* name);  /* index of a named dispatch option in it, -1 if unknown   */
const char* vlnce_last_error(void);

/* Dispatch options: which of the library's equivalent kernels a launch is given to.  Explicit
 * state instead of environment variables, so that a host (or a test) can force a kernel onto a
 * shape in-process and restore the default afterwards.  No reference counterpart (torch picks its
 * cuDNN / MIOpen algorithm through torch.backends.cudnn.benchmark, never set by the reference).
 *   name               default  meaning
 *   "conv_math"        2        0: v_mfma_f32_32x32x2_f32 only; non-zero: the plane kernels (conv_p3 /
 *                               conv_u3 / conv_s3 / conv_m3 / conv_x3 / stem7) on the 16-bit matrix pipe.
 *                               The library tests zero / non-zero only; the HOST reads the value as the
 *                               plane format in which it packs the weights (vlnce_prologue.w_format):
 *                               1 = three bf16 planes, six products per multiply (fp32's exponent range);
 *                               2 = fp16 planes, THREE products per multiply (ABI 142; |x| < 65504,
 *                               |w| < 32, forward operands -- see vlnce_conv2d_pack_weights)
 *   "p3"               2        conv_p3_kernel: 0 off, 1 every layer it covers, 2 KxK only, 3 1x1 only
 *   "p3_tile"          0        0: by CU fill; 1..6: forced tile shape
 *   "s3"               1        conv_s3_kernel (short-K wide 1x1): 0 off, 1 default rule, 2 every eligible shape
 *   "u3"               1        conv_u3_kernel (wide 1x1): 0 off, 1 default rule, 2 / 3 force 64- / 128-row tiles
 *   "u3_waves"         8        8, or 4 (one wave per SIMD)
 *   "x3_tile"          0        conv_x3_kernel: 0 by CU fill, 1..4 forced tile shape
 *   "igemm_tile"       0        igemm_kernel: 0 rule, 1 128x128, 2 128x64, 3 64x64
 *   "igemm_nobuf"      0        1: no buffer-descriptor operand loads
 *   "igemm_no_splitk"  0        1: no split-K
 *   "wgrad_tile"       64       vlnce_conv2d_wgrad: 1 = the fp32-MFMA kernel everywhere (64x64 tiles; A/B against the
 *                               bf16-plane kernel that takes Cin % 32 == 0, Cout % 32 == 0 layers otherwise), 64 / 128 =
 *                               tile of the fp32-MFMA kernel where that one runs
 *   "rollout_one_xcd"  0        1: all workgroups of vlnce_gru_rollout_* on one XCD
 *   "m3"               1        conv_m3_kernel (small launches): 0 off, 1 default rule, 2 / 3 every layer it covers
 *   "r3"               1        the regenerating block end (vlnce_prologue.regen, conv_r3_kernel; ABI 148).  The
 *                               library launches what a call asks for; the HOST reads this option to choose
 *                               between the two routes of a block end: 0 conv3 stores its raw output and the
 *                               next 1x1 reads it back, 1 the layers on which the regenerating pair was measured
 *                               faster (launches of at least four 64-row tiles per CU), 2 every block end the
 *                               kernel covers
 *   "s3_wgs"           0        conv_s3_kernel / conv_r3_kernel: 0 = one workgroup per CU; n > 0 = at most n
 *                               workgroups (tests: many tiles per workgroup at a small M)
 *   "waypoint_dist"    0        read by the HOST (ABI 151): 1 = WaypointPolicy.evaluate_actions computes its
 *                               log-probability and entropies through vlnce_waypoint_eval / _bwd instead of
 *                               torch's distribution classes (the same as policy.fused_distributions = True)
 *   "waypoint_act"     0        read by the HOST (ABI 154): 1 = WaypointPolicy.act draws and scores the whole action
 *                               through vlnce_waypoint_act instead of torch's distribution classes (the same as
 *                               policy.fused_act = True)
 * Set options between launches, not concurrently with them (relaxed atomics).  Unknown names
 * return non-zero. */
int vlnce_set_option(const char* name, int value);
int vlnce_get_option(const char* name, int* value);
int vlnce_option_default(const char* name, int* value);

/* ---------------------------------------------------------------- conv / GEMM
 * Implicit-GEMM convolution on v_mfma_f32_32x32x2_f32 (exact fp32):
 *   Y[m, co] = epilogue( sum_{r,q,ci} prologue(X[n, ho*s-p+r, wo*s-p+q, ci]) * W[co, r, q, ci] )
 * with m = (n*Ho + ho)*Wo + wo.  Replaces nn.Conv2d(+BatchNorm2d/+ReLU/+add) of
 * the torchvision trunk (models/encoders/resnet_encoders.py:136-139,199) and of
 * habitat's GroupNorm ResNetEncoder (resnet_encoders.py:31-43,95).
 */
typedef struct {
  int N, H, W, Cin;   /* input  [N,H,W,Cin], pixel stride ldx floats (>= Cin) */
  int Cout, KH, KW;   /* weight [Cout,KH,KW,Cin] ("OHWI"), contiguous          */
  int stride, pad;
  int Ho, Wo;         /* output [N,Ho,Wo,Cout], row stride ldy floats (>= Cout) */
  int ldx, ldy;
} vlnce_conv_desc;

/* The launch's input REGENERATED instead of read (ABI 148; vlnce_prologue.regen): x of the launch
 * would have been the raw output of the stride-1 1x1 expansion
 *   x[m, :] = conv1x1(act((rx[m, :] - in_center) * in_scale + in_shift), w)      Cin -> 4 Cin channels
 * and the launch computes it again, tile by tile in registers, from rx -- a quarter of the bytes --
 * instead of reading it back.  Train-mode ResNet-50 layers 1-2: conv3 of a bottleneck runs as a
 * statistics-only launch (vlnce_epilogue.stats_only), and the block end inside the next block's
 * first 1x1 (dual-input prologue below) regenerates conv3's output from conv2's.  The values are
 * those the statistics were taken from (same kernel arithmetic), so side_out is what the storing
 * route writes.  conv_r3_kernel: Cin = 64 / 128, Cout of the launch 64 / 128 (Cin 64) or 128 / 256
 * (Cin 128); needs x2, in_scale / in_shift (the expansion's BatchNorm), side_out, w_frag, a raw output
 * (no epilogue arithmetic) and x == NULL.  Anything else is an error, never another kernel. */
typedef struct {
  const float* x;         /* rx: [N,H,W,Cin] of the launch's geometry, pixel stride ldx floats (>= Cin)  */
  int Cin, ldx;
  const void* w_frag;     /* the expansion's weights [4 Cin, 1, 1, Cin] as B fragments, format w_format */
  const float* in_scale;  /* its operand prologue (NULL scale = identity, NULL center = 0)             */
  const float* in_shift;
  const float* in_center;
  int in_relu;
} vlnce_regen;

typedef struct {
  /* input transform applied in the A-operand loader BEFORE zero padding:
   *   x' = act((x - in_center[ci]) * in_scale[ci] + in_shift[ci]);  NULL scale = identity,
   *   NULL center = 0.
   * Used for the RGB stem's /255 (+ImageNet mean/std, resnet_encoders.py:171-192)
   * and to apply the previous layer's BatchNorm+ReLU on the fly. */
  const float* in_scale;
  const float* in_shift;
  const float* in_center;
  int in_relu;
  /* Optional second input (1x1 / stride-1 / pad-0 convolutions with Cin % 32 == 0 only): the
   * end of a residual block, out = relu(bn3(conv3) + identity) (torchvision Bottleneck.forward),
   * is evaluated inside the NEXT block's first convolution instead of in a pass of its own:
   *   x' = act((x - in_center)*in_scale + in_shift + ((x2 - in2_center)*in2_scale + in2_shift))
   * x2 has the layout of x; in2_scale NULL = x2 is added as is (identity skip), non-NULL = the
   * downsample branch's raw conv output with its BatchNorm.  side_out (same layout as x, or
   * NULL) receives x' -- the block output the following layers read as their skip input. */
  const float* x2;
  const float* in2_scale;
  const float* in2_shift;
  const float* in2_center;
  float* side_out;
  /* Optional: the weights w_ohwi pre-split into three bf16 planes by
   * vlnce_conv2d_split_weights() (layout [3][Cout*KH*KW*Cin] of 16-bit words).  With it,
   * convolutions on the buffer-descriptor hot path (Cin % 32 == 0) run as six bf16 plane
   * products on the bf16 matrix pipe (conv_x3_kernel: fp32-equivalent result, DESIGN.md
   * section 6); without it (NULL) they run on v_mfma_f32_32x32x2_f32. */
  const void* w_split;
  /* Optional: the weights as bf16-plane MFMA B fragments (vlnce_conv2d_pack_weights()).  With it,
   * stride-1 KxK and all 1x1 convolutions with Cin % 32 == 0 and Cout % 32 == 0 run on
   * conv_p3_kernel (A operand transformed once per workgroup into an LDS patch, B fragments
   * straight from L2); NULL = conv_x3_kernel / igemm_kernel as above. */
  const void* w_frag;
  /* Optional: the dispatch options of THIS launch -- vlnce_option_count() ints indexed by
   * vlnce_option_index(name), a negative entry = the process value (vlnce_set_option); NULL = the
   * process values.  Two policies (or a test forcing a kernel) in one process then do not share
   * mutable dispatch state: the library only reads what the call hands it. */
  const int* options;
  /* Plane format of w_split / w_frag (ABI 142) = the arithmetic of the plane kernels for this
   * launch: 0 or 1 = three bf16 planes (six plane products per multiply), 2 = fp16 planes (three
   * products); must be the `format` the two buffers were made with. */
  int w_format;
  /* Optional (ABI 148): the launch's input is computed again instead of read; see vlnce_regen. */
  const vlnce_regen* regen;
} vlnce_prologue;

/* Train-mode BatchNorm statistics taken BY the convolution (torch.nn.BatchNorm2d.forward in
 * training mode on the convolution's output: resnet_encoders.py:136-139 leaves the frozen trunk's
 * BatchNorm on batch statistics).  Every workgroup adds the {sum x, sum x^2} of
 * its raw output columns to `acc` with fp64 device-scope atomics (per 32-row block: the block
 * sum in fp32, x^2 as M2_block + sum^2 / rows evaluated in fp64 -- the same function of the
 * accumulators as the tile-moment path below); vlnce_bn_finalize_sums, one workgroup, then turns
 * the sums into the pending normalisation and the running statistics and leaves `acc` zero
 * again.  Together they replace convolution + [coarsen] + finalize over thousands of tile
 * moments (9-21 us behind every convolution of the train-mode trunk) by convolution + ~4 us.
 * A kernel without this epilogue (fp32-MFMA kernel, split-K) writes its tile moments to
 * `workspace` and the library reduces them into `acc` itself: the caller sees the same thing. */
#define VLNCE_BN_SHARDS 16 /* copies of the sums: workgroup b adds to copy b % 16 (atomic contention) */
typedef struct {
  double* acc;            /* [VLNCE_BN_SHARDS][Cout][2] {sum x, sum x^2}; added to, not overwritten */
  void* workspace;        /* vlnce_conv2d_bn_workspace_bytes(d) bytes, uninitialised               */
  long workspace_bytes;
} vlnce_bn_sums;

typedef struct {
  const float* scale;     /* [Cout] per-channel multiplier or NULL (folded eval-BN gamma/sqrt(var+eps)) */
  const float* shift;     /* [Cout] per-channel add or NULL (bias / folded BN shift)                    */
  const float* residual;  /* [M,Cout] (row stride ldr) added before the activation, or NULL            */
  int ldr;
  int act;                /* VLNCE_ACT_*                                                               */
  int accumulate;         /* Y += result (after activation) instead of Y = result                      */
  /* train-mode BatchNorm: per-(M-tile, channel) partial statistics of the RAW
   * accumulator (before scale/shift): float2 {sum, M2 about the tile mean}.
   * Layout [tiles_m][Cout][2]; tiles_m from vlnce_conv2d_tiles_m(). NULL = off. */
  float* stat_partial;
  /* train-mode BatchNorm statistics added by the convolution (see vlnce_bn_sums); excludes
   * stat_partial, scale, shift, residual, act and accumulate.  NULL = off. */
  const vlnce_bn_sums* bn;
  /* Statistics-only launch (ABI 148): non-zero = the launch takes the statistics of the RAW output
   * (bn or stat_partial, one of them is required) and stores NO output; y must be NULL.  For a
   * convolution whose output is cheaper to compute again than to read back: the stride-1 1x1
   * expansions with Cin = 64 / 128 and Cout % 256 == 0 that conv_s3_kernel covers (w_frag
   * required).  Any other problem is an error, never another kernel.  The sums are those of the
   * storing launch up to the order of the atomic adds. */
  int stats_only;
} vlnce_epilogue;

long vlnce_conv2d_bn_workspace_bytes(const vlnce_conv_desc* d); /* vlnce_bn_sums.workspace */
/* The sums of vlnce_bn_sums (all VLNCE_BN_SHARDS copies, M values per channel) -> scale_out =
 * gamma * rstd, mean_out = batch mean [, shift_out = beta - mean * scale, rstd_out]; running
 * statistics updated like torch (momentum, unbiased variance); `acc` is zero afterwards. */
int vlnce_bn_finalize_sums(double* acc, int M, int C, const float* gamma, const float* beta,
                           float eps, float momentum, float* running_mean, float* running_var,
                           float* scale_out, float* shift_out, float* mean_out, float* rstd_out,
                           vlnce_stream_t stream);

int vlnce_conv2d_tiles_m(const vlnce_conv_desc* d);   /* rows of stat_partial  */
int vlnce_conv2d_tile_rows(const vlnce_conv_desc* d); /* BM chosen for `d`      */

/* planes[q][i], q = 0..2; `planes` holds 3 * count 16-bit words.
 * format 1: bf16 words with w[i] == planes[0][i] + planes[1][i] + planes[2][i] exactly
 *   (round-to-nearest three-way split, 8 + 8 + 8 mantissa bits); a product of two operands split
 *   this way is six plane products (dropped terms <= 2^-26 relative).
 * format 2 (ABI 142): fp16 words {h * 2^11, (w - h) * 2^11 rounded, h} with h = fp16(w) -- 11 + 11
 *   mantissa bits (+ the sign of the second term: |w - h - l| <= 2^-22 |w|); the activations are
 *   split the same way in the operand loader ({a1, a2 * 2^11}) and a product is the THREE plane
 *   products a1 b1 + a1 b2 + a2 b1, all at the scale 2^11 (the low planes stay clear of fp16's
 *   subnormals; the accumulator is multiplied by 2^-11 where it leaves the registers).  Measured
 *   against fp64 the result is as close as format 1's (fp32 accumulation dominates both, and
 *   format 2 does half as many accumulator updates) at half the matrix-pipe time.  Range:
 *   |w| < 32 and |activation| < 65504, beyond that the output is inf / NaN (never a wrong finite
 *   value); operands far below 6e-5 (gradients) lose relative precision: backward launches use
 *   format 1. */
int vlnce_conv2d_split_weights(const float* w, void* planes, long count, int format,
                               vlnce_stream_t stream);

/* frag = the weights of `d` as bf16-plane MFMA B fragments, layout
 * [Cout/32][K/16][3 planes][64 lanes][8 bf16] with the k-slabs ordered (32-channel chunk, filter
 * tap, 16-channel half) and w == plane0 + plane1 + plane2 exactly (round-to-nearest split).
 * vlnce_conv2d_pack_bytes() = bytes `frag` must hold (Cout*K*6), or 0 where the fragment kernel
 * does not apply (Cin % 32 != 0 or Cout % 32 != 0).  Replaces nothing upstream: a cached
 * re-layout of nn.Conv2d.weight (resnet_encoders.py:136-139). */
long vlnce_conv2d_pack_bytes(const vlnce_conv_desc* d);
int vlnce_conv2d_pack_weights(const float* w_ohwi, void* frag, const vlnce_conv_desc* d,
                              int format /* as vlnce_conv2d_split_weights */, vlnce_stream_t stream);

/* Every weight image of a TRAINABLE trunk in one launch (ABI 143).  With
 * MODEL.{RGB,DEPTH}_ENCODER.trainable (resnet_encoders.py:45-46,141-143) the filters change every
 * optimizer step; per convolution the step needs the forward bank W[Cout,T,Cin] (T = KH*KW taps) and
 * the data-gradient bank W'[Cin,T,Cout] with the taps reversed, each as fp32, as planes
 * (vlnce_conv2d_split_weights' layout) and as fragments (vlnce_conv2d_pack_weights' layout) -- bit
 * for bit what those entry points write for the permuted tensors.  A job names ONE of these outputs
 * and reads the parameter where it lies, in nn.Conv2d's own [Cout, Cin, KH, KW] layout.
 *   kind 0: fp32 [N,T,C];  1: planes [3][N*T*C];  2: fragments (N % 32 == 0 and C % 32 == 0)
 *   with (N, C) = (Cout, Cin), or (Cin, Cout) when `transposed`; C % 8 == 0 throughout.
 * vlnce_weight_job_items() = the work items of a job (-1: not eligible).  `jobs_dev` and
 * `first_item_dev` (njobs + 1 running item counts, first_item[0] = 0) are DEVICE arrays the host
 * builds once per trunk; total_items = first_item[njobs]. */
typedef struct vlnce_weight_job {
  const float* w_oihw;
  void* dst;
  int Cout, Cin, T;
  int kind;
  int transposed;
  int format; /* plane format of kinds 1 and 2 (1 = three bf16 planes, 2 = fp16 planes) */
} vlnce_weight_job;
long vlnce_weight_job_items(const vlnce_weight_job* job);
int vlnce_conv2d_prepare_weights(const vlnce_weight_job* jobs_dev, const long* first_item_dev,
                                 int njobs, long total_items, vlnce_stream_t stream);

/* Which kernel the calling thread's last vlnce_conv2d_fwd was dispatched to: the measurement
 * harness prices bf16-pipe launches (6 plane products per multiply) and fp32-MFMA launches
 * against their own peaks.  No reference counterpart. */
#define VLNCE_CONV_PATH_F32 0 /* igemm_kernel, v_mfma_f32_32x32x2_f32 (incl. split-K)            */
#define VLNCE_CONV_PATH_X3 1  /* conv_x3_kernel, bf16 planes, im2col K-tiles through LDS          */
#define VLNCE_CONV_PATH_P3 2  /* conv_p3_kernel, bf16 planes, patch-resident A / fragment-order B */
#define VLNCE_CONV_PATH_M3 3  /* conv_m3_kernel, bf16 planes, small launches: no LDS staging, 4-way k split */
int vlnce_conv2d_last_path(void);

/* Which kernel INSTANCE that launch went to (ABI 146): behind each family sit several template
 * instances with their own product schedule, scaling and epilogue, and the tests name the one a case
 * must land on.  Set by the host code that picks the instance; -1 before the thread's first launch.
 *   bits  0..1  family, = vlnce_conv2d_last_path()
 *   bits  2..3  plane format of the launch: 1 / 2 (vlnce_prologue.w_format), 0 for the fp32 kernel
 *   bits  4..7  kernel within the family (VLNCE_CONV_KERNEL_*)
 *   bits  8..15 A, 16..23 B, 24..30 C: what tells that kernel's instances apart
 *     P3 / conv_p3:  A = tile 1..6 ({128,256} {64,256} {256,128} {128,128} {256,64} {128,64} rows x
 *                    columns, option "p3_tile"'s numbering), B = VLNCE_CONV_P3_DENSE / _GATHER / _DUAL
 *     P3 / conv_u3:  A = tile rows (64 / 128), B = kind (0 one input, 1 two inputs, 2 two inputs
 *                    each with its own normalisation), C = waves (4 / 8)
 *     P3 / conv_s3:  A = Cin (64 / 128), B = 1 for the statistics-only instance (ABI 148)
 *     P3 / conv_r3:  A = channels of the regenerated expansion's input (64 / 128), B = Cout / 32,
 *                    C = skip kind (1 identity, 2 with its own normalisation)
 *     M3:            A = NT (32-column blocks per wave), B = KSPLIT (waves sharing a reduction),
 *                    C = RB (32-row blocks per workgroup)
 *     X3:            A = tile 1..4 ({128,128} {64,128} {128,64} {64,64}, option "x3_tile"'s
 *                    numbering), B = 1 with the two-input prologue
 *     F32:           A = the split-K factor of VLNCE_CONV_KERNEL_F32_SPLITK, else 0 */
#define VLNCE_CONV_KERNEL(family, format, kernel, a, b, c) \
  ((family) | ((format) << 2) | ((kernel) << 4) | ((a) << 8) | ((b) << 16) | ((c) << 24))
#define VLNCE_CONV_KERNEL_FAMILY(v) ((v) & 3)
#define VLNCE_CONV_KERNEL_FORMAT(v) (((v) >> 2) & 3)
#define VLNCE_CONV_KERNEL_KIND(v) (((v) >> 4) & 15)
#define VLNCE_CONV_KERNEL_A(v) (((v) >> 8) & 255)
#define VLNCE_CONV_KERNEL_B(v) (((v) >> 16) & 255)
#define VLNCE_CONV_KERNEL_C(v) (((v) >> 24) & 127)
/* family P3 */
#define VLNCE_CONV_KERNEL_P3 0 /* conv_p3_kernel */
#define VLNCE_CONV_KERNEL_U3 1 /* conv_u3_kernel */
#define VLNCE_CONV_KERNEL_S3 2 /* conv_s3_kernel */
#define VLNCE_CONV_KERNEL_R3 3 /* conv_r3_kernel */
#define VLNCE_CONV_P3_DENSE 0  /* KxK: the patch in LDS            */
#define VLNCE_CONV_P3_GATHER 1 /* 1x1: rows gathered               */
#define VLNCE_CONV_P3_DUAL 2   /* 1x1 with the two-input prologue  */
/* family F32 (igemm_kernel) */
#define VLNCE_CONV_KERNEL_F32_BUF 0    /* A_BUF / B_BUF tiles (buffer-descriptor loaders)          */
#define VLNCE_CONV_KERNEL_F32_SPLITK 1 /* 64x64 A_BUF tiles, reduction split A ways, atomic adds    */
#define VLNCE_CONV_KERNEL_F32_V4 2     /* A_IM2COL_V4 / B_NK_V4 tiles (Cin % 4 == 0)               */
#define VLNCE_CONV_KERNEL_F32_S 3      /* A_IM2COL_S / B_NK_S tiles (scalar loaders)               */
#define VLNCE_CONV_KERNEL_F32_STEM3 4  /* 7x7 stem, Cin 3                                          */
#define VLNCE_CONV_KERNEL_F32_STEM1 5  /* 7x7 stem, Cin 1                                          */
#define VLNCE_CONV_KERNEL_F32_DUAL 6   /* A_BUF tiles with the two-input prologue                  */
/* families X3 and M3 have one kernel each: 0 */
int vlnce_conv2d_last_kernel(void);

int vlnce_conv2d_fwd(const float* x, const float* w_ohwi, float* y,
                     const vlnce_conv_desc* d, const vlnce_prologue* pro,
                     const vlnce_epilogue* epi, vlnce_stream_t stream);

/* General GEMM  C[M,N] = act( op(A)[M,K] * op(B)[K,N] * scale[n] + shift[n] + R )
 *   transA = 0: A is [M,K] row-major (lda)     transA = 1: A is stored [K,M] (lda)
 *   transB = 0: B is [N,K] row-major (ldb)  -- i.e. an nn.Linear weight
 *   transB = 1: B is stored [K,N] row-major (ldb)
 * Replaces nn.Linear / 1x1 nn.Conv1d forward and their dgrad/wgrad
 * (cma_policy.py:103-119,140-170; seq2seq_policy.py:109-121;
 * waypoint_predictors.py:76-180; policy.py:19-21).
 * Operands: A, B, C and epi->residual need only be 4-byte aligned with any row stride when
 * transA = transB = 0 (the scalar loaders / the scalar epilogue take what the 16-byte ones cannot);
 * with transB = 1, B (and with transA = 1 also A) must be 16-byte aligned, else the call is an
 * error.  epi->scale and epi->shift must be 16-byte aligned whatever route the call takes (the
 * vectorised epilogue reads four columns of them at once; ABI 150: a 4-byte-aligned view of a
 * bias is refused with an error, it launches nothing).  transA = 1 requires transB = 1.
 */
int vlnce_gemm(const float* A, int lda, int transA, const float* B, int ldb, int transB,
               float* C, int ldc, int M, int N, int K,
               const vlnce_epilogue* epi, vlnce_stream_t stream);

/* Which igemm_kernel instance the calling thread's last vlnce_gemm launched and what ran around
 * it (ABI 150): behind the one entry point sit six loader pairs, three tiles, the split reduction
 * with its zero-fill and its second bias / activation pass, and the tests name the route a call
 * must take.  Set by the host code that picks the launch (no device work); -1 before the thread's
 * first launch; a call refused with an error leaves it as it was.
 *   bits  0..1  A loader (VLNCE_GEMM_A_*)      bits 2..3  B loader (VLNCE_GEMM_B_*)
 *   bits  4..5  tile (VLNCE_GEMM_TILE_*, option "igemm_tile"'s numbering)
 *   bit   6     C was zero-filled first (a split reduction that does not accumulate)
 *   bit   7     the second pass C = act(C + shift) ran (a split reduction with a bias / activation)
 *   bits  8..15 split-K factor: K ranges added atomically, 1 = not split */
#define VLNCE_GEMM_KERNEL(a, b, tile, splitk, zero, pass2) \
  ((a) | ((b) << 2) | ((tile) << 4) | ((zero) ? 1 << 6 : 0) | ((pass2) ? 1 << 7 : 0) | ((splitk) << 8))
#define VLNCE_GEMM_KERNEL_A(v) ((v) & 3)
#define VLNCE_GEMM_KERNEL_B(v) (((v) >> 2) & 3)
#define VLNCE_GEMM_KERNEL_TILE(v) (((v) >> 4) & 3)
#define VLNCE_GEMM_KERNEL_ZERO(v) (((v) >> 6) & 1)
#define VLNCE_GEMM_KERNEL_PASS2(v) (((v) >> 7) & 1)
#define VLNCE_GEMM_KERNEL_SPLITK(v) (((v) >> 8) & 255)
#define VLNCE_GEMM_A_BUF 0       /* buffer-descriptor loads: K % 32 == 0, rows 16-byte aligned, < 2 GiB */
#define VLNCE_GEMM_A_IM2COL_V4 1 /* 16-byte loads: K % 4 == 0, lda % 4 == 0, A 16-byte aligned          */
#define VLNCE_GEMM_A_IM2COL_S 2  /* 4-byte loads: anything else                                         */
#define VLNCE_GEMM_A_TRANS 3     /* transA = 1: A stored [K,M]                                          */
#define VLNCE_GEMM_B_BUF 0       /* [N,K], buffer-descriptor loads */
#define VLNCE_GEMM_B_NK_V4 1     /* [N,K], 16-byte loads           */
#define VLNCE_GEMM_B_NK_S 2      /* [N,K], 4-byte loads            */
#define VLNCE_GEMM_B_KN 3        /* transB = 1: B stored [K,N]     */
#define VLNCE_GEMM_TILE_128X128 1
#define VLNCE_GEMM_TILE_128X64 2
#define VLNCE_GEMM_TILE_64X64 3
int vlnce_gemm_last_kernel(void);

/* Skinny linear layers (M <= 128 rows = one row per environment; N % 4 == 0, K % 4 == 0; rows of x,
 * w, dy, y 16-byte aligned), ABI 141: y = act(x W^T + b) in ONE launch and the whole backward --
 * dx [M,K] = dz W, dw [N,K] = dz^T x, db [N] = colsum dz with dz = dy * act'(y) -- in ONE launch
 * (each of dx / dw / db may be NULL), exact fp32 MFMA, no atomics, no pre-zeroed outputs.
 * Replace nn.Linear / the nn.GRU projections of the nets at one row per environment and their
 * autograd (cma_policy.py:103-131,140-177; seq2seq_policy.py:109-121; waypoint_predictors.py:76-180),
 * which through vlnce_gemm are 3 launches forward and 5 backward per layer. */
int vlnce_linear_rows_supported(int M, int N, int K);
int vlnce_linear_rows_fwd(const float* x, int ldx, const float* w, int ldw, const float* bias,
                          int act, float* y, int ldy, int M, int N, int K, vlnce_stream_t stream);
int vlnce_linear_rows_bwd(const float* x, int ldx, const float* w, int ldw, const float* dy,
                          int lddy, const float* y, int ldy, int act, float* dx, float* dw,
                          float* db, int M, int N, int K, vlnce_stream_t stream);

/* column sums: out[n] (+)= sum_m X[m,n]  (bias gradients) */
int vlnce_colsum(const float* x, int ldx, int M, int N, float* out, int accumulate,
                 vlnce_stream_t stream);

/* ------------------------------------------------------------- normalisation
 * BatchNorm2d (torchvision trunk; eps 1e-5, momentum 0.1; SURVEY App. B-1:
 * runs on batch statistics whenever the policy was not .eval()'d).
 * vlnce_bn_finalize reduces the conv epilogue's partials (Chan's parallel
 * variance, fp64 combine) into per-channel scale/shift and updates the running
 * statistics exactly like torch (unbiased running_var). */
size_t vlnce_bn_finalize_workspace_bytes(int tiles_m, int C); /* 0 unless tiles_m > 4096 */
int vlnce_bn_finalize(const float* stat_partial, int tiles_m, int tile_rows, int M, int C,
                      const float* gamma, const float* beta, float eps, float momentum,
                      float* running_mean, float* running_var, /* may be NULL */
                      float* scale_out, float* shift_out,
                      float* mean_out, float* rstd_out, /* may be NULL; saved for backward */
                      void* workspace, size_t workspace_bytes, /* caller-allocated scratch */
                      vlnce_stream_t stream);

/* y = act((x - center[s, c]) * scale[s, c] + shift[s, c] + residual)   with s = row / rows_per_sample
 * (rows_per_sample = 0 => one vector for all rows: BatchNorm apply; > 0 => per-sample vectors
 * [Nsamples, C]: GroupNorm apply).  center may be NULL (= 0).  Batch-statistics normalisation
 * passes center = mean, scale = gamma*rstd, shift = beta: the reference's own arithmetic
 * ((x - mean) * rstd * gamma + beta), which keeps fp32 accuracy when |mean| >> std. */
int vlnce_scale_shift_act(const float* x, const float* scale, const float* shift,
                          const float* center, int rows_per_sample, const float* residual,
                          float* y, long M, int C, int act, vlnce_stream_t stream);

/* y = act(x1*scale1[c]+shift1[c] + x2*scale2[c]+shift2[c]); y may alias x1.  End of a residual
 * block with a conv+BatchNorm downsample: both raw conv outputs normalised in one pass. */
int vlnce_scale_shift_add_act(const float* x1, const float* scale1, const float* shift1,
                              const float* center1, const float* x2, const float* scale2,
                              const float* shift2, const float* center2, float* y, long M, int C,
                              int act, vlnce_stream_t stream);

/* GroupNorm (habitat depth trunk: ngroups 16, and GroupNorm(1,C) in the
 * compression block; eps 1e-5).  Two launches: partial sums per
 * (sample, pixel-chunk, channel) then a finalize that emits per-(sample,channel)
 * scale/shift for vlnce_scale_shift_act. */
int vlnce_gn_chunks(int HW);
int vlnce_gn_partial(const float* x, int Nimg, int HW, int C, float* partial /* [N,chunks,C,2] */,
                     vlnce_stream_t stream);
int vlnce_gn_finalize(const float* partial, int Nimg, int HW, int C, int groups,
                      const float* gamma, const float* beta, float eps,
                      float* scale_out, float* shift_out, /* [N,C] */
                      float* center_out, /* [N,C] or NULL: if given, shift_out = beta and
                                            center_out = mean (unfolded form) */
                      float* mean_out, float* rstd_out,   /* [N,groups] or NULL */
                      vlnce_stream_t stream);
/* Same result from the convolution epilogue's tile statistics (vlnce_epilogue.stat_partial,
 * {sum, M2} per tile of tile_rows output pixels): usable when HW % tile_rows == 0, i.e. no tile
 * straddles two samples; saves the vlnce_gn_partial pass over the activation. */
int vlnce_gn_finalize_tiles(const float* stat_partial, int tile_rows, int Nimg, int HW, int C,
                            int groups, const float* gamma, const float* beta, float eps,
                            float* scale_out, float* shift_out, float* center_out,
                            float* mean_out, float* rstd_out, vlnce_stream_t stream);
/* y = act(GroupNorm(x) + residual) of a small activation x [N, HW, C] in ONE launch (one
 * workgroup per (sample, group): mean, centred second moment, apply): what the policy uses at
 * one to a few environments (act(), resnet_encoders.py:31-43 GroupNorm trunk), where the three
 * launches of the pipeline above are latency, not bandwidth.  residual may be NULL; y may alias x. */
int vlnce_group_norm_small(const float* x, int Nimg, int HW, int C, int groups, const float* gamma,
                           const float* beta, float eps, const float* residual, int act, float* y,
                           vlnce_stream_t stream);

/* ------------------------------------------------------------------ pooling
 * NHWC. maxpool 3x3/s2/p1 (torchvision + habitat stems), avg_pool2d(2)
 * (ResNetEncoder.forward), adaptive_avg_pool2d -> (OH,OW)
 * (resnet_encoders.py:154-162; also the global 1x1 pool). */
/* maxpool over act(x*in_scale[c]+in_shift[c]) when in_scale != NULL: the stem's BatchNorm+ReLU
 * is applied on the fly to the raw conv output (train mode), saving one HBM round trip. */
int vlnce_maxpool3x3s2(const float* x, float* y, int N, int H, int W, int C, int Ho, int Wo,
                       const float* in_scale, const float* in_shift, const float* in_center,
                       int in_relu, vlnce_stream_t stream);
int vlnce_avgpool2x2(const float* x, float* y, int N, int H, int W, int C, vlnce_stream_t stream);

/* 2x2 space-to-depth with explicit zero border and optional per-channel input transform:
 *   y[n, pb_h, pb_w, (dy*2+dx)*C + c] = x[n, 2*(pb_h-pad_lo)+dy, 2*(pb_w-pad_lo)+dx, c]*scale[c]+shift[c]
 * y is [N, H/2+pad_lo+pad_hi, W/2+pad_lo+pad_hi, 4C].  With pad_lo=2, pad_hi=1 a 7x7/stride-2/pad-3
 * stem convolution (torchvision ResNet conv1, resnet_encoders.py:136-139; habitat ResNet conv1)
 * over x equals a 4x4/stride-1/pad-0 convolution over y with the taps regrouped: the 3-channel
 * gather becomes contiguous 16-byte loads (K = 64*C instead of 49*C scattered elements).  The
 * transform (/255, ImageNet mean/std: resnet_encoders.py:184-190) is applied before the zero
 * border, exactly like the reference normalises before the padded convolution. */
int vlnce_space_to_depth2(const float* x, float* y, int N, int H, int W, int C, int pad_lo,
                          int pad_hi, const float* scale, const float* shift,
                          vlnce_stream_t stream);
/* ------------------------------------------------------------- observation ingest
 * What habitat's batch_obs (fp32 cast), CenterCropperPerSensor / ObsStack
 * (habitat_extensions/obs_transformers.py:21-145), the waypoint net's concatenation of 12
 * panorama frames with the done-masked history frame (waypoint_predictors.py:330-375) and the
 * encoders' own input handling (/255, avg_pool2d(2): resnet_encoders.py:95,198-199) do in four
 * passes over fp32 frames, in one pass over the frames in their STORAGE type (uint8 RGB). */
#define VLNCE_DT_F32 0
#define VLNCE_DT_U8 1
typedef struct {
  const void* x;              /* [N, F, Hs, Ws, C] frames (F = 1: a plain [N, Hs, Ws, C] sensor)      */
  const void* x2;             /* optional extra frame per env [N, Hs, Ws, C], appended as frame F      */
  const unsigned char* mask2; /* optional [N]: the extra frame is multiplied by it (not-done mask)     */
  int dtype;                  /* VLNCE_DT_F32 | VLNCE_DT_U8: element type of x and x2                  */
  int N, F, Hs, Ws, C;
  int y0, x0, H, W;           /* centre-crop window: rows [y0, y0+H), columns [x0, x0+W) of each frame */
} vlnce_frames;
/* RGB stem input: 2x2 space-to-depth of every (cropped) frame with the per-channel input
 * transform, y [N*(F + (x2 != NULL)), H/2+pad_lo+pad_hi, W/2+pad_lo+pad_hi, 4C] fp32; image index
 * n*(F+1) + f as torch.cat([frames, history.unsqueeze(1)], 1).flatten(0, 1) orders them. */
int vlnce_frames_s2d(const vlnce_frames* frames, float* y, int pad_lo, int pad_hi,
                     const float* scale, const float* shift, vlnce_stream_t stream);
/* RGB stem in one launch, from the frames: y[img, ho, wo, :] = conv 7x7 / stride 2 / pad 3 of
 * (frame * in_scale[c] + in_shift[c]) (zero outside the frame) with `Cout` = 32 | 64 filters --
 * torchvision ResNet.conv1 behind the encoder's /255 (+ ImageNet mean/std),
 * resnet_encoders.py:131-139,171-199 -- on the 16-bit matrix pipe (w_format 1: three exact bf16
 * planes per operand, six plane products; 2: fp16 planes, three products -- the formats of
 * vlnce_conv2d_split_weights; fp32 accumulation).  w_frag: the filters as B fragments
 * [Cout/32][11 k-slabs][3 planes][64 lanes][8 x 16 bit], k' = kh * 24 + kw * 3 + c (21 of every 24
 * used, the rest and k' >= 168 zero), lane (l, h) = output channel 32 nb + l, k' = 16 ks + 8 h + [0, 8).
 * epi: NULL, {scale, shift, act} (eval: folded BatchNorm + ReLU) or {bn} (train: raw output, the
 * launch adds its column sums to bn->acc; workspace unused). */
int vlnce_stem7_fwd(const vlnce_frames* frames, const float* in_scale, const float* in_shift,
                    const void* w_frag, int w_format, float* y, int Cout, const vlnce_epilogue* epi,
                    vlnce_stream_t stream);
/* depth stem input: F.avg_pool2d(x, 2) of every frame, y [N*(F+..), H/2, W/2, C] fp32 */
int vlnce_frames_avgpool2(const vlnce_frames* frames, float* y, vlnce_stream_t stream);
/* the frames as fp32 [N*(F+..), H, W, C] (x*scale+shift when given): stems that cannot take the
 * space-to-depth form, trainable encoders */
int vlnce_frames_f32(const vlnce_frames* frames, float* y, const float* scale, const float* shift,
                     vlnce_stream_t stream);
/* eager ObsStack + CenterCropperPerSensor: out[n, f, h, w, :] = srcs[f][n, y0+h, x0+w, :] for F
 * (<= 16) source sensors [N, Hs, Ws, C] of elem_bytes-wide elements; `srcs` is a HOST array of
 * device pointers; out [N, F, H, W, C] in the source element type (bytes are moved as they are). */
int vlnce_frames_gather(const void* const* srcs, int F, int elem_bytes, int N, int Hs, int Ws,
                        int C, int y0, int x0, int H, int W, void* out, vlnce_stream_t stream);

/* habitat's ResizeShortestEdge [3P, habitat-lab v0.1.7 habitat_baselines/common/obs_transformers.py;
 * enabled by every RxR config, rxr_baselines/rxr_cma_en.yaml:27-30, applied at
 * base_il_trainer.py:284-285] = image_resize_shortest_edge = F.interpolate(mode="area") to
 * (OH, OW) = (int(Hs*size/min(Hs,Ws)), int(Ws*size/min(Hs,Ws))), cast back to the sensor dtype --
 * fused with the CenterCropperPerSensor window that follows it:
 *   out[i, h, w, c] = cast(mean of x[i, hs0:hs1, ws0:ws1, c]),  hs0 = floor((y0+h)*Hs/OH),
 *   hs1 = ceil((y0+h+1)*Hs/OH), columns likewise (at::adaptive_avg_pool2d's windows and
 *   summation order; uint8 truncates).  x [NF, Hs, Ws, C] and out [NF, H, W, C] in `dtype`
 *   (VLNCE_DT_U8 | VLNCE_DT_F32); (y0, x0, H, W) = (0, 0, OH, OW) is the plain resize. */
int vlnce_frames_resize_area(const void* x, int dtype, int NF, int Hs, int Ws, int C, int OH, int OW,
                             int y0, int x0, int H, int W, void* out, vlnce_stream_t stream);

int vlnce_adaptive_avgpool(const float* x, float* y, int N, int H, int W, int C, int OH, int OW,
                           int ldy, vlnce_stream_t stream);

/* ------------------------------------------------- backward of the visual trunks
 * (only reached with MODEL.RGB_ENCODER / DEPTH_ENCODER .trainable = True; the reference
 * default keeps both encoders frozen).  Data gradients of stride-1 convolutions reuse
 * vlnce_conv2d_fwd with the flipped / transposed weights. */
/* dW[Cout,KH,KW,Cin] = sum_m dY[m,co] * im2col(X)[m,(r,q,ci)]   (split over output pixels, fp32 atomics
 * into dW, which the call zeroes itself).  Cin % 32 == 0 and Cout % 32 == 0: six bf16-plane products
 * per multiply on the 16-bit matrix pipe (plane format 1: the operands are gradients); else, and with
 * option "wgrad_tile" = 1, v_mfma_f32_32x32x2_f32.
 * dy_pow2 / P (ABI 143, may be NULL / 0): the [2][P] power-of-two buffer vlnce_bn_bwd / vlnce_gn_bwd filled
 * for this dy (dy_pow2[0] = 2^k, dy_pow2[P] = 2^-k) -- with it the plane kernel runs in format 2:
 * x on the two-plane side (|x| < 65504), dy * 2^(k-10) on the three-plane side, three plane
 * products per multiply, the result scaled back exactly.
 * accumulate != 0 (ABI 143): dW += instead of dW = (the call does not zero dW). */
int vlnce_conv2d_wgrad(const float* x, const float* dy, float* dw_ohwi, const vlnce_conv_desc* d,
                       const float* dy_pow2, int P, int accumulate, vlnce_stream_t stream);
/* Which kernel the calling thread's last vlnce_conv2d_wgrad was dispatched to (ABI 145; -1 before the
 * thread's first call).  No reference counterpart. */
#define VLNCE_WGRAD_PATH_F32 0     /* igemm_kernel<A_TRANS, B_IM2COL>, v_mfma_f32_32x32x2_f32 */
#define VLNCE_WGRAD_PATH_X6_BF16 1 /* wgrad_x6_kernel, three bf16 planes per operand          */
#define VLNCE_WGRAD_PATH_X6_F16 2  /* wgrad_x6_kernel, fp16 planes (dy_pow2 given)            */
int vlnce_conv2d_wgrad_last_path(void);
/* ... and which instance (ABI 146; -1 before the thread's first call):
 *   bits 0..3  vlnce_conv2d_wgrad_last_path()
 *   bits 4..11 row tile over Cout: TM of wgrad_x6_kernel (64 / 128), or the square tile of the fp32 kernel
 *   bit  12    the reduction over the pixels was split over workgroups (atomic adds into dW) */
#define VLNCE_WGRAD_KERNEL(path, tm, split) ((path) | ((tm) << 4) | ((split) ? 1 << 12 : 0))
#define VLNCE_WGRAD_KERNEL_PATH(v) ((v) & 15)
#define VLNCE_WGRAD_KERNEL_TM(v) (((v) >> 4) & 255)
#define VLNCE_WGRAD_KERNEL_SPLIT(v) (((v) >> 12) & 1)
int vlnce_conv2d_wgrad_last_kernel(void);
/* BatchNorm2d backward through y = act(x*gamma*rstd + (beta - mean*gamma*rstd) (+ residual)):
 * g = dy*[y>0] when relu; dbeta = sum g; dgamma = sum g*xhat;
 * dx = gamma*rstd*(g - dbeta/M - xhat*dgamma/M) with batch statistics, gamma*rstd*g with
 * running statistics (use_batch_stats = 0).  dres (may be NULL) receives g.  workspace (ABI 143):
 * vlnce_bn_bwd_workspace_floats(M, C) floats -- the per-block partial sums of the two reductions
 * (no same-address atomics); 0 floats / may be NULL when C % 4 != 0.
 * pow2 (ABI 143, may be NULL; needs C % 4 == 0): [2][P] floats, on return P copies of 2^k followed by P
 * copies of 2^-k, with k the power of two at which dx fits the fp16 planes of plane format 2
 * (bound(|dx|) * 2^k in (2^13, 2^14], the bound computed from the per-channel maxima of |g| and
 * |x - mean| gathered by the reduction pass).  They are the prologue / epilogue vectors
 * (vlnce_prologue.in_scale with a zero in_shift; vlnce_epilogue.scale) of the data-gradient
 * convolution that reads dx, and the `dy_pow2` of vlnce_conv2d_wgrad: gradients live far below
 * fp16's normal range, scaled by an exact power of two they take format 2's three plane products
 * instead of format 1's six. */
size_t vlnce_bn_bwd_workspace_floats(long M, int C);
int vlnce_bn_bwd(const float* dy, const float* y, const float* x, const float* mean,
                 const float* rstd, const float* gamma, long M, int C, int relu,
                 int use_batch_stats, float* dx, float* dres, float* dgamma, float* dbeta,
                 float* workspace, float* pow2, int P, vlnce_stream_t stream);
/* GroupNorm backward (same conventions; mean/rstd are [N,groups]); workspace from
 * vlnce_gn_bwd_workspace_floats() floats ([N,chunks,C,2] partial sums, [N,groups,2] group sums padded to a
 * multiple of 4 floats, [N,chunks,C,2] partial maxima, [N] bounds, [N,C,2] per-sample shares of dbeta /
 * dgamma, which are added up in sample order: no atomics, the same bits on every call; chunks =
 * ceil(HW / 128)); pow2 / P as vlnce_bn_bwd. */
size_t vlnce_gn_bwd_workspace_floats(int Nimg, int HW, int C, int groups);
int vlnce_gn_bwd(const float* dy, const float* y, const float* x, const float* mean,
                 const float* rstd, const float* gamma, int Nimg, int HW, int C, int groups,
                 int relu, float* dx, float* dres, float* dgamma, float* dbeta, float* workspace,
                 float* pow2, int P, vlnce_stream_t stream);
/* max-pool forward that also records the arg-max tap (0..8), and its backward */
int vlnce_maxpool3x3s2_argmax(const float* x, float* y, uint8_t* argmax, int N, int H, int W,
                              int C, int Ho, int Wo, vlnce_stream_t stream);
int vlnce_maxpool3x3s2_bwd(const float* dy, const uint8_t* argmax, float* dx, int N, int H, int W,
                           int C, int Ho, int Wo, vlnce_stream_t stream);
int vlnce_adaptive_avgpool_bwd(const float* dy, float* dx, int N, int H, int W, int C, int OH,
                               int OW, vlnce_stream_t stream);

/* ---------------------------------------------------------------- categorical action head
 * habitat-lab CategoricalNet (built at models/policy.py:19-21; the distribution is utils.py:269-289):
 *   z = x W^T + b;  torch.distributions.Categorical(logits=z) keeps  z - logsumexp(z, -1)  and its
 *   argument validation raises when that holds a NaN.
 * fwd: x [M,K] (row stride ldx), w [A,K], b [A] or NULL, A <= 16  ->  logits_out [M,A] (normalised);
 *      *nan_count (device int, or NULL) is incremented once per row that holds a NaN -- the host
 *      reads it where the reference's validation reads its own flag.
 * bwd: logits = what fwd returned, dlogits = gradient w.r.t. it;  dx [M,K], dw [A,K], db [A]
 *      (each may be NULL; db needs dw).  One launch (plus a zero-fill when M > 1024, where the rows
 *      of dw are reduced by several workgroups). */
int vlnce_action_head_fwd(const float* x, int ldx, const float* w, const float* b, int M, int K,
                          int A, float* logits_out, int* nan_count, vlnce_stream_t stream);
int vlnce_action_head_bwd(const float* x, int ldx, const float* w, const float* logits,
                          const float* dlogits, int M, int K, int A, float* dx, float* dw,
                          float* db, vlnce_stream_t stream);

/* ---------------------------------------------------------------- attention
 * One query per batch row against P keys:  logits[i] = <q, K[i]>;
 *   mask_mode 1 (additive, CMANet._attn cma_policy.py:207-217): logits -= mask*1e8
 *   mask_mode 2 (multiplicative, DotProductAttention utils.py:173-177): logits *= mask
 *   attn = softmax(logits * scale);  out = sum_i attn[i] * V[i]
 * K: [B,P,Dk] (row stride ldk), V: [B,P,Dv] (row stride ldv), mask: uint8 [B,P] or NULL.
 * attn_out [B,P] is saved for the backward.  P <= 1024. */
int vlnce_attn_fwd(const float* q, const float* K, int ldk, const float* V, int ldv,
                   const uint8_t* mask, int mask_mode, float scale,
                   float* out, float* attn_out, int B, int P, int Dk, int Dv,
                   vlnce_stream_t stream);
int vlnce_attn_bwd(const float* dout, const float* q, const float* K, int ldk,
                   const float* V, int ldv, const uint8_t* mask, int mask_mode, float scale,
                   const float* attn, float* dq, float* dK, int lddk, float* dV, int lddv,
                   int B, int P, int Dk, int Dv, vlnce_stream_t stream);

/* The same attention with K / V / mask SHARED by groups of queries: query row b attends over block
 * kv_index[b] (0 <= kv_index[b] < U) of K [U,P,Dk], V [U,P,Dv], mask [U,P].  A sequence-mode batch
 * (T*N rows: a cached-feature DAgger batch, dagger_trainer.py:39-114) repeats every episode's
 * instruction T times; the instruction encoder runs once per DISTINCT instruction and the text
 * attention (cma_policy.py:260) reads the distinct blocks in place instead of a T-fold expanded
 * copy.  bwd: dq [B,Dk]; dK [B,P,Dk] / dV [B,P,Dv] are PER QUERY ROW (as vlnce_attn_bwd writes
 * them) -- vlnce_segment_sum reduces them to the U blocks. */
int vlnce_attn_fwd_shared(const float* q, const float* K, int ldk, const float* V, int ldv,
                          const uint8_t* mask, int mask_mode, float scale, const int64_t* kv_index,
                          float* out, float* attn_out, int B, int P, int Dk, int Dv,
                          vlnce_stream_t stream);
int vlnce_attn_bwd_shared(const float* dout, const float* q, const float* K, int ldk,
                          const float* V, int ldv, const uint8_t* mask, int mask_mode, float scale,
                          const int64_t* kv_index, const float* attn, float* dq, float* dK,
                          int lddk, float* dV, int lddv, int B, int P, int Dk, int Dv,
                          vlnce_stream_t stream);
/* out[u, :] = sum of the rows b of x [B, row_elems] with index[b] == u, added in row order
 * (deterministic; the backward of a row gather `x_u.index_select(0, index)`).  row_elems % 4 == 0,
 * U <= 65535. */
int vlnce_segment_sum(const float* x, const int64_t* index, int B, int U, long row_elems,
                      float* out, vlnce_stream_t stream);
/* mask[b,i] = all_c(x[b,i,c] == 0)   (text_mask, cma_policy.py:260) */
int vlnce_rowzero_mask(const float* x, int ld, long rows, int C, uint8_t* mask,
                       vlnce_stream_t stream);

/* --------------------------------------------------------- recurrent cells
 * GRU / LSTM pointwise gate stage (torch.nn.GRU/LSTM semantics, gate order
 * r,z,n / i,f,g,o) with the done-mask already applied to h_prev by the caller
 * through `mask` (h_prev_eff = h_prev * mask[b]); gi = x W_ih^T + b_ih and
 * gh = h_prev_eff W_hh^T + b_hh come from vlnce_gemm.  Replaces habitat's
 * RNNStateEncoder single/seq forward (seq2seq_policy.py:164, cma_policy.py:
 * 249-256,287-294, waypoint_predictors.py:420-427,532-545). */
int vlnce_gru_gates_fwd(const float* gi, const float* gh, const float* h_prev,
                        const uint8_t* mask, /* [B] or NULL */
                        float* h_out, float* gates_out /* [B,3H] r,z,n saved */,
                        float* hn_out /* [B,H] saved W_hn h + b_hn */,
                        int B, int H, vlnce_stream_t stream);
int vlnce_gru_gates_bwd(const float* dh_out, const float* gates, const float* hn,
                        const float* h_prev, const uint8_t* mask,
                        float* dgi, float* dgh, float* dh_prev, int B, int H,
                        vlnce_stream_t stream);
int vlnce_lstm_gates_fwd(const float* gi, const float* gh, const float* c_prev,
                         const uint8_t* mask, float* h_out, float* c_out,
                         float* gates_out /* [B,4H] i,f,g,o activated */, int B, int H,
                         vlnce_stream_t stream);
int vlnce_lstm_gates_bwd(const float* dh_out, const float* dc_out, const float* gates,
                         const float* c_prev, const float* c_out, const uint8_t* mask,
                         float* dgates /* [B,4H] */, float* dc_prev, int B, int H,
                         vlnce_stream_t stream);

/* Packed-sequence instruction RNN (instruction_encoder.py:27-32,80-94): the whole
 * time loop (and its BPTT) in ONE launch, one workgroup per (direction, 16-sample
 * tile), recurrent weights resident in registers, h W_hh^T on v_mfma_f32_16x16x4_f32.
 * kind 0 = LSTM (gates i|f|g|o), 1 = GRU (r|z|n); dirs 1 or 2 (index 1 = reverse).
 * All per-direction arguments are HOST arrays of `dirs` device pointers.
 *   gi[d]      [L,B,G*H]  x W_ih^T + b_ih, time-major
 *   w_hh[d]    [G*H,H], b_hh[d] [G*H]
 *   out[d]     [L,B,H]    must be pre-zeroed: steps t >= lengths[b] emit zeros
 *   h_final[d] [B,H]      state after each sample's last step
 *   gates_save[d] [L,B,G*H], aux_save[d] [L,B,H] (LSTM: c_t; GRU: W_hn h + b_hn) or NULL arrays
 * Steps t >= lengths[b] leave the state untouched; the reverse direction walks
 * t = lengths[b]-1 .. 0 (pack_padded_sequence / pad_packed_sequence semantics). */
int vlnce_rnn_seq_supported(int kind, int H);
int vlnce_rnn_seq_fwd(int kind, int dirs, const float* const* gi, const float* const* w_hh,
                      const float* const* b_hh, const int* lengths, float* const* out,
                      float* const* h_final, float* const* gates_save, float* const* aux_save,
                      int B, int L, int H, vlnce_stream_t stream);
/* BPTT: w_hh_t[d] = W_hh^T [H,G*H]; dout[d] [L,B,H] / dh_final[d] [B,H] may be NULL;
 * dgi[d] [L,B,G*H] (pre-zeroed) receives d/d gi; GRU additionally fills dgh[d]
 * (gradient wrt h W_hh^T + b_hh; its n-gate differs by the factor r). */
int vlnce_rnn_seq_bwd(int kind, int dirs, const float* const* w_hh_t, const int* lengths,
                      const float* const* out, const float* const* gates_save,
                      const float* const* aux_save, const float* const* dout,
                      const float* const* dh_final, float* const* dgi, float* const* dgh,
                      int B, int L, int H, vlnce_stream_t stream);
/* Second-generation entry points (ABI 141): the same two kernels, self-contained -- the launch
 * writes the zeros past each row's length itself (no pre-zeroed buffers), the forward also stores
 * the outputs in the CONSUMER's layout (`seq`, may be NULL: element (t, b, direction d, unit u) at
 * seq[t * seq_st + b * seq_sb + d * H + u]; [B, L, dirs*H] rows = the reference's
 * pad_packed_sequence output permuted, instruction_encoder.py:88-94, with seq_st = dirs*H,
 * seq_sb = L*dirs*H) next to the time-major copy `out_tm[d]` [L,B,H] the backward needs, BPTT takes
 * the output gradient in that same addressing (`dseq`, may be NULL; regrouped into `dout_ws` by a
 * small launch of the same call) and W_hh as the module stores it ([G*H, H], no transposed copy).
 * dgi / dgh [L,B,G*H] are written everywhere. */
int vlnce_rnn_seq_fwd2(int kind, int dirs, const float* const* gi, const float* const* w_hh,
                       const float* const* b_hh, const int* lengths, float* const* out_tm,
                       float* seq, long seq_st, long seq_sb, float* const* h_final,
                       float* const* gates_save, float* const* aux_save, int B, int L, int H,
                       vlnce_stream_t stream);
int vlnce_rnn_seq_bwd2(int kind, int dirs, const float* const* w_hh, const int* lengths,
                       const float* const* out_tm, const float* const* gates_save,
                       const float* const* aux_save, const float* dseq, long dseq_st, long dseq_sb,
                       float* dout_ws /* dirs*L*B*H floats, needed with dseq */,
                       const float* const* dh_final, float* const* dgi, float* const* dgh,
                       int B, int L, int H, vlnce_stream_t stream);
/* Every parameter gradient of the recurrent layer, and the gradient of its input rows, from what
 * BPTT left in dgi / dgh, behind ONE call (torch: the autograd of nn.LSTM / nn.GRU's weight_ih,
 * weight_hh, bias_ih, bias_hh): dw_hh[d] [G*H,H] = dGh^T Hprev, db_hh[d] = colsum dGh (dGh = dgh
 * for a GRU, dgi for an LSTM), dw_ih[d] [G*H,E] = dgi^T X, db_ih[d] = colsum dgi (skipped when
 * db_ih[d] == db_hh[d]: an LSTM's two bias gradients are equal), dx_tm [L*B, E] (may be NULL) =
 * sum_d dgi[d] W_ih[d].  x_tm: the time-major input rows [L*B, E] (row stride ldx).  first_dir: the
 * direction element 0 of the arrays is (0 forward, 1 reverse: a call for one direction alone, so that
 * a host can run the two directions on two streams). */
int vlnce_rnn_seq_wgrad(int kind, int dirs, int first_dir, const float* const* dgi, const float* const* dgh,
                        const float* const* out_tm, const float* x_tm, int ldx, int E,
                        const float* const* w_ih, float* const* dw_ih, float* const* dw_hh,
                        float* const* db_ih, float* const* db_hh, float* dx_tm, int B, int L, int H,
                        vlnce_stream_t stream);

/* ---------------------------------------------------------------- utilities */
/* y[b, c] = mean_p x[b, p, c]   (AdaptiveAvgPool1d(1) of rgb_linear, cma_policy.py:104) */
int vlnce_mean_rows(const float* x, float* y, int B, int P, int C, vlnce_stream_t stream);
/* x[b, :] *= mask[b]  (done-mask zeroing of the recurrent state; out may alias x) */
/* One step of a T-step state-encoder rollout over N <= 16 episodes, fused (habitat
 * RNNStateEncoder.seq_forward, call sites cma_policy.py:249-256,287-294; rollout_storage.py:154-276):
 *   fwd: hp = mask * h_prev; gates(gi + hp W_hh^T + b_hh); h (, c)          -- one launch
 *   bwd: dh = dout + carry; gate gradients (dgi, dgh);
 *        carry <- mask * (dh*z + dgh W_hh)  (GRU) | mask * (dgates W_hh)  (LSTM) -- two launches
 * w_hh_t is W_hh^T [H, G*H]; carry is read and overwritten; acc0 is [N,H] scratch.
 * aux = W_hn h + b_hn (GRU) | c_t (LSTM); gates = post-activation gates, torch order. */
int vlnce_rnn_step_supported(int N, int H, int lstm);
int vlnce_rnn_step_fwd(int lstm, const float* gi, const float* h_prev, const float* c_prev,
                       const uint8_t* mask, const float* w_hh, const float* b_hh, float* hp_out,
                       float* h_out, float* aux_out, float* gates_out, int N, int H,
                       vlnce_stream_t stream);
int vlnce_rnn_step_bwd(int lstm, const float* dout, float* carry, const float* dc,
                       const float* gates, const float* aux, const float* hp, const float* c_prev,
                       const uint8_t* mask, const float* w_hh_t, float* dgi, float* dgh,
                       float* acc0, float* dc_prev, int N, int H, vlnce_stream_t stream);
int vlnce_mask_rows(const float* x, const uint8_t* mask, float* out, int B, int H,
                    vlnce_stream_t stream);
/* The WHOLE T-step rollout of the masked GRU state encoder as one launch forward and one backward
 * (habitat RNNStateEncoder.seq_forward: h is multiplied by the not-done mask of step t before
 * step t; call sites cma_policy.py:249-256,287-294, seq2seq_policy.py:128-136) for N <= 16
 * episodes and H in {64,128,256,512}: H/16 workgroups keep their rows of W_hh in registers for
 * all T steps and hand each other the new state (backward: the gate gradients) as (value, step
 * tag) pairs, one 64-bit device-scope atomic store / polling load each: no fence, no counter.  Same arithmetic (fp32 FMA) and the same saved tensors as T calls of
 * vlnce_rnn_step_fwd / _bwd:
 *   fwd: gi [T,N,3H] (x W_ih^T + b_ih), h0 [N,H], mask [T,N] -> hp [T,N,H] (mask_t * h_{t-1}),
 *        out [T,N,H], gates [T,N,3H] (r, z, n), aux [T,N,H] (W_hn hp + b_hn);
 *   bwd: dout [T,N,H] (NULL = zeros), dh_final [N,H] (NULL = zeros), w_hh_t = W_hh^T [H,3H]
 *        -> dgi, dgh [T,N,3H], dh0 [N,H] (gradient wrt h0, the step-0 mask applied).
 * workspace: vlnce_gru_rollout_workspace_bytes(N, H) bytes of device memory owned by the caller
 * for the duration of the launch (the double-buffered exchange area of (value, step tag) pairs;
 * zeroed by the call).  All H/16 workgroups must become resident: do not run it beside a kernel
 * that holds every CU for longer than a few seconds (a lost workgroup traps). */
int vlnce_gru_rollout_supported(int N, int H);
long vlnce_gru_rollout_workspace_bytes(int N, int H);
int vlnce_gru_rollout_fwd(const float* gi, const float* h0, const uint8_t* mask, const float* w_hh,
                          const float* b_hh, float* hp, float* out, float* gates, float* aux,
                          void* workspace, int T, int N, int H, vlnce_stream_t stream);
int vlnce_gru_rollout_bwd(const float* dout, const float* dh_final, const float* gates,
                          const float* aux, const float* hp, const uint8_t* mask,
                          const float* w_hh_t, float* dgi, float* dgh, float* dh0,
                          void* workspace, int T, int N, int H, vlnce_stream_t stream);
/* The same for an LSTM state encoder (ABI 144; STATE_ENCODER.rnn_type = LSTM), gate order i, f, g, o:
 * the decomposition, the exchange and its tags are the GRU's.  The cell state is unit-local: the
 * thread that finishes (unit, episode) keeps c_t (backward: dc) in a register for all T steps, so
 * only h crosses workgroups forward and the 4H pre-activation gate gradients backward (dgi is also
 * the recurrent gradient: an LSTM has no separate dgh).  Same arithmetic and the same saved tensors
 * as T calls of vlnce_rnn_step_fwd / _bwd with lstm = 1:
 *   fwd: gi [T,N,4H] (x W_ih^T + b_ih), h0, c0 [N,H], mask [T,N] -> hp [T,N,H] (mask_t * h_{t-1}),
 *        out [T,N,H], gates [T,N,4H] (i, f, g, o activated), aux [T,N,H] (c_t; step t uses
 *        mask_t * c_{t-1}, c_{-1} = c0);
 *   bwd: dout [T,N,H], dh_final, dc_final [N,H] (each NULL = zeros), c0 as given to fwd,
 *        w_hh_t = W_hh^T [H,4H] -> dgi [T,N,4H], dh0, dc0 [N,H] (the step-0 mask applied).
 * workspace: vlnce_lstm_rollout_workspace_bytes(N, H) = 2 * N * 4H pairs of 8 bytes, owned by the
 * caller for the duration of the launch and zeroed by the call.  _supported: N in 1..16, H in
 * {64,128,256,512}, at least H/16 compute units, and the LDS one workgroup of this (N, H) instance
 * needs (up to 152 KB: the backward at N > 8, H = 512) within the device's limit per workgroup;
 * where it returns 0 the entry points return an error and launch nothing.  Residency as above. */
int vlnce_lstm_rollout_supported(int N, int H);
long vlnce_lstm_rollout_workspace_bytes(int N, int H);
int vlnce_lstm_rollout_fwd(const float* gi, const float* h0, const float* c0, const uint8_t* mask,
                           const float* w_hh, const float* b_hh, float* hp, float* out, float* gates,
                           float* aux, void* workspace, int T, int N, int H, vlnce_stream_t stream);
int vlnce_lstm_rollout_bwd(const float* dout, const float* dh_final, const float* dc_final,
                           const float* gates, const float* aux, const float* hp, const float* c0,
                           const uint8_t* mask, const float* w_hh_t, float* dgi, float* dh0,
                           float* dc0, void* workspace, int T, int N, int H, vlnce_stream_t stream);

/* out[b, :] = mask[b] ? a[b, :] : b[b, :]  (NULL operand = zeros): packed-sequence
 * semantics of the instruction RNN (steps past a sample's length keep the state
 * and emit zeros, instruction_encoder.py:80-94). */
int vlnce_select_rows(const uint8_t* mask, const float* a, const float* b, float* out, int B, int H,
                      vlnce_stream_t stream);
/* Backward of nn.Embedding (instruction_encoder.py:41-45,72-73: the learned token embedding):
 * grad_weight[tokens[r], :] += grad_rows[r, :] for rows with tokens[r] != padding_idx, fp32
 * atomics into a grad_weight the caller has zeroed (one launch instead of torch's sort /
 * segment / scatter chain).  tokens int64 [rows], grad_rows [rows, E], grad_weight [vocab, E]. */
int vlnce_embedding_bwd(const long* tokens, const float* grad_rows, float* grad_weight, long rows,
                        int E, long padding_idx, long vocab, vlnce_stream_t stream);
/* dz = dy * act'(.) written through the activation output y (ReLU/Sigmoid/Tanh backward). */
int vlnce_act_bwd(const float* dy, const float* y, float* dz, long n, int act,
                  vlnce_stream_t stream);

/* ---- cached-feature DAgger data path ----------------------------------
 * Replaces dagger_trainer.py:39-114 `collate_fn` (+ the .to(device, float32) that follows it at
 * :562-571) and the inflection weights of IWTrajectoryDataset.__next__ (:196-208): B ragged
 * trajectories, rows of all of them concatenated ([sum T_b, D], fp32 or fp16 as the LMDB cache
 * stores them) and an offsets vector [B+1] on the device, become the padded time-major batch
 * [Tmax*B, D] (row t*B + b) in one pass.  Observations are padded with 1.0 (sic, :77), actions
 * and weights with 0. */
enum { VLNCE_SRC_F32 = 0, VLNCE_SRC_F16 = 1, VLNCE_SRC_I64 = 2 };
/* observation sensors: any source type -> fp32 (upstream casts every sensor, tokens included) */
int vlnce_ragged_pad_rows(const void* src, int src_dtype, const int* offsets, int B, int Tmax,
                          long D, float fill, float* dst, vlnce_stream_t stream);
int vlnce_ragged_pad_rows_i64(const int64_t* src, const int* offsets, int B, int Tmax, long D,
                              int64_t fill, int64_t* dst, vlnce_stream_t stream);
/* corrected_actions [Tmax,B] (0 past the end), inflection weights [Tmax,B] (coef at t = 0 and
 * where the oracle action changes, 1 elsewhere, 0 past the end), not_done_masks [Tmax,B]
 * (0 in row t = 0, 1 elsewhere -- also past the end, as upstream). */
int vlnce_dagger_targets(const int64_t* oracle_actions, const int* offsets, int B, int Tmax,
                         float inflection_coef, int64_t* corrected_out, float* weights_out,
                         uint8_t* masks_out, vlnce_stream_t stream);

/* ---- DAgger rollout collection (ABI 147): the WRITE half of the feature cache ---------------
 * What dagger_trainer.py:294-314 (feature hooks: o.cpu() per step), :420-435 (per-environment
 * .item() read-backs) and :339-356 (host re-stack + astype(float16) per finished episode) do on
 * the host, kept on the device: every recorded sensor has an arena [num_envs][capacity][C*P] in
 * its STORAGE dtype, and one launch appends one step of every sensor for every live environment.
 * Source row r of a sensor goes to dst + ((long)slots[r]*capacity + steps[r]) * C*P, c-major
 * (NCHW order) whatever the source's strides -- the trunks hand out a permuted NHWC view (c_stride
 * 1, p_stride C), read coalesced along c, each lane writing its P outputs contiguously; contiguous
 * sources (P = 1, c_stride 1) move 4 elements per lane where pointers, row_stride and C allow.
 * ONLY P = 16 and P = 4 (the 4x4 and 2x2 maps of the cached trunks) with c_stride 1 take that
 * transposed path; any other strided view (P = 49, P = 8, c_stride > 1, ...) is correct but goes one
 * output element per lane: coalesced stores, loads strided by p_stride across the wave.
 * Conversions: f32 -> f16 rounds to nearest even, subnormals kept, overflow to infinity (numpy's
 * astype(float16)); i64 -> f16 goes through f32 (batch_obs casts to float first); u8 -> f16 / f32
 * and same-type copies are exact; f32 / u8 -> i64 truncate like a C cast.
 * sensors / slots / steps are HOST arrays copied into the launch arguments: no H2D copy, no
 * allocation, no synchronisation.  At most VLNCE_TRAJ_MAX_SENSORS sensors and VLNCE_TRAJ_MAX_ROWS
 * rows per call (more: error; the caller splits); every steps[r] in [0, capacity), slots[r] >= 0
 * (the arena's first extent is the caller's to respect).  All index arithmetic is 64-bit. */
enum { VLNCE_TRAJ_F32 = 0, VLNCE_TRAJ_F16 = 1, VLNCE_TRAJ_I64 = 2, VLNCE_TRAJ_U8 = 3 };
#define VLNCE_TRAJ_MAX_SENSORS 8
#define VLNCE_TRAJ_MAX_ROWS 128
typedef struct {
  const void* src;      /* element (row r, c, p) at src + (r*row_stride + c*c_stride + p*p_stride) * elem */
  void* dst;            /* arena [num_envs][capacity][C*P] in the storage dtype                            */
  long row_stride, c_stride, p_stride;   /* in elements of the source dtype, >= 0                         */
  int C, P;             /* a row is written as C*P contiguous elements, c-major (NCHW order)              */
  int src_dtype;        /* VLNCE_TRAJ_F32 | _I64 | _U8                                                     */
  int dst_dtype;        /* VLNCE_TRAJ_F16 | _F32 | _I64                                                    */
} vlnce_traj_sensor;
int vlnce_traj_append(const vlnce_traj_sensor* sensors, int n_sensors, const int* slots,
                      const int* steps, int n_rows, long capacity, vlnce_stream_t stream);
/* dagger_trainer.py:414-442 in one launch, per row: e = (long)expert; a = uniform < beta ? e :
 * action (fp32 comparison, as torch compares with a Python float); skip = (e == -1); a = skip ? 0
 * : a; prev_actions = a; stepped = {a, skip}.  expert_dtype: VLNCE_TRAJ_F32 | VLNCE_TRAJ_I64.
 * `uniform` is the caller's torch.rand_like(actions, dtype=float): the RNG stream stays torch's. */
int vlnce_dagger_mix_actions(const int64_t* actions, const void* expert, int expert_dtype,
                             const float* uniform, float beta, int n, int64_t* prev_actions,
                             int64_t* stepped /* [2][n] */, vlnce_stream_t stream);

/* DD-PPO returns: RolloutStorage.compute_returns (rollout_storage.py:127-152).
 * rewards [T,N]; value_preds, masks, returns [T+1,N]; next_value [N].  GAE: value_preds[T] is set
 * to next_value and returns[0..T) = gae + value_preds; otherwise returns[T] = next_value and the
 * discounted sum runs backwards. */
int vlnce_ppo_returns(const float* rewards, float* value_preds, const float* masks,
                      const float* next_value, float* returns, int T, int N, float gamma, float tau,
                      int use_gae, vlnce_stream_t stream);

/* WDDPPO minibatch loss (ddppo_alg.py:78-121: entropy terms, clipped surrogate,
 * clipped value loss, offset L1 term) and its gradients in ONE launch (ABI 141).  All inputs [B]
 * (one value per rollout row); radians may be NULL (no "offset" action component).  stats[8] =
 * {loss, value_loss, action_loss, entropy_loss, mean pano / offset / distance entropy, offset_loss};
 * grads [5][B] = d loss / d {values, logp, ent_pano, ent_offset, ent_distance} for a unit upstream
 * gradient (torch's tie rules for max / min / clamp). */
int vlnce_ppo_loss(const float* values, const float* returns, const float* value_preds,
                   const float* logp, const float* old_logp, const float* adv,
                   const float* ent_pano, const float* ent_offset, const float* ent_distance,
                   const float* radians, int B, float clip, float value_coef, float entropy_coef,
                   float pano_coef, float offset_coef, float distance_coef, float reg_coef,
                   int use_clipped, float* stats, float* grads, vlnce_stream_t stream);

/* The imitation-learning objective of BaseVLNCETrainer._update_agent (base_il_trainer.py:159-172)
 * and its gradient in ONE launch of one workgroup (ABI 149).  logits [T,N,A] fp32 contiguous (rows
 * time-major, t * N + n; raw or normalised: the log-softmax is taken again, as F.cross_entropy
 * does), targets [T,N] int64, weights [T,N] fp32, aux a device scalar or NULL, inv_scalar = 1 /
 * loss_accumulation_scalar.
 *   ce[t,n]  = logsumexp(logits[t,n,:]) - logits[t,n,targets[t,n]]
 *   action   = mean_n( sum_t w ce / sum_t w )
 *   stats[3] = {(action + aux) * inv_scalar, action, aux or 0}
 *   dlogits [T*N,A] = (softmax - onehot) * w[t,n] / sum_t w[:,n] / N * inv_scalar
 * (the gradient of stats[0] for a unit upstream gradient; d stats[0] / d aux = inv_scalar).
 * torch's arithmetic: w * ce is a product (a padded row, w = 0, is multiplied, not skipped: a
 * non-finite ce there gives NaN), and a column whose weights sum to zero divides 0 / 0.  A target
 * outside [0, A) reads nothing outside its row: that row's ce and dlogits are NaN, and so are
 * action and stats[0].  fp64 accumulators, fixed reduction order, no atomics: two runs give the
 * same bits.  Shapes: T >= 1, 1 <= N <= 1024 (the column sums are kept in LDS), 1 <= A <= 16;
 * vlnce_il_loss_supported says so, the launch refuses anything else. */
int vlnce_il_loss_supported(int T, int N, int A);
int vlnce_il_loss(const float* logits, const int64_t* targets, const float* weights,
                  const float* aux, float inv_scalar, int T, int N, int A, float* stats,
                  float* dlogits, vlnce_stream_t stream);

/* The progress monitor's auxiliary term without its [R,E] matrix (ABI 149): F.mse_loss of estimate
 * [E] against target [R,1] broadcasts to element (i,j) = (e_j - t_i)^2 (cma_policy.py:296-307), and
 * AuxLosses.reduce's masked_select with a mask [E] picks COLUMNS j (aux_losses.py:24-32):
 *   value[0]      = sum_j m_j sum_i (e_j - t_i)^2 / (R * sum m)
 *   d_estimate[j] = m_j * 2 sum_i (e_j - t_i) / (R * sum m)
 * E != R is allowed (under data parallelism the targets are those of all ranks).  mask: one byte
 * per column, non-zero = selected; no selected column gives 0 / 0 like the mean of nothing.  The
 * column sum is evaluated in fp64 as R d^2 - 2 d S1 + S2 around the targets' mean (d = e_j - mean,
 * S1 = sum_i (t_i - mean), S2 = sum_i (t_i - mean)^2), which does not cancel when the estimates sit
 * on the targets.  One workgroup, fixed reduction order, no atomics. */
int vlnce_pair_mse(const float* estimate, const float* target, const uint8_t* mask, int E, int R,
                   float* value, float* d_estimate, vlnce_stream_t stream);

/* The distribution arithmetic of WaypointPolicy.evaluate_actions (waypoint_policy.py:258-347 over
 * TruncatedNormal / CustomFixedCategorical of models/utils.py:24-152, 269-289) as ONE launch forward
 * and ONE backward (ABI 151): the composite log-probability and the three entropies of a stored
 * action under the heads' outputs.  One thread per row, every row in fp64, one rounding to fp32 at
 * each store, no floating-point atomics: two runs give the same bits.
 *
 * A component ("offset", "distance") is described by a vlnce_wp_part:
 *   kind     VLNCE_WP_ABSENT (contributes nothing, its entropy is 0), VLNCE_WP_CONTINUOUS (truncated
 *            normal on [lo, hi]) or VLNCE_WP_DISCRETE (categorical over K classes)
 *   first    [B,P] means, or [B,P,K] logits (raw or normalised)
 *   second   [B,P] variances (continuous only)
 *   element  the stored sub-action: float [B] (continuous) or int64 [B] (class index)
 *   lo, hi   the truncation window, as fp32 (what torch's fp32 arithmetic makes of the Python floats)
 *   weight   the 0 / 1 `predict_*` switch
 * With c = pano[b] (int64, 0..P; P = STOP), h = c mod P and gate = (c != P):
 *   out[0][b] = log_softmax(logits[b,:])[c] + sum_part gate * weight * logp_part(element[b])
 *   out[1][b] = the categorical entropy of logits[b,:]  (a class of probability 0 contributes 0)
 *   out[2][b] = gate * weight * H_offset,   out[3][b] = gate * weight * H_distance   (continuous)
 * out is one float buffer: log_prob [B], pano entropy [B], then the offset's and the distance's
 * entropy blocks.  A continuous (or absent) part's block is [B] as above.  A DISCRETE part's block is
 * [B][B], E[i][j] = gate_i * weight * H_j: the reference multiplies its [B,1] weight with the
 * categorical's [B] entropy, which broadcasts (for B = 1 the one value); E[i][j] is NaN where row j
 * is flagged or pano[i] is out of range, and its gradient reaches row j as sum_i gate_i weight g[i][j]
 * (rows in order).  out_floats = the buffer's capacity (>= B (2 + n + n), n = 1 or B; checked).
 * continuous, with loc = first[b,h], scale = sqrt(second[b,h]), [a, b] = ([lo, hi] - loc) / scale,
 * mass = cdf(b) - cdf(a), z = (element - loc) / scale:
 *   logp = -z^2 / 2 - log(sqrt(2 pi) scale mass)
 *   H    = log(sqrt(2 pi e) scale mass) + (a pdf(a) - b pdf(b)) / (2 mass)
 * discrete: logp / H of the categorical over first[b,h,:].  gate * weight MULTIPLIES a value that was
 * computed (torch's arithmetic: 0 * inf is NaN); a weight-0 or STOP row is not skipped.
 *
 * flags[b] (int32) collects what the reference asserts on, whatever the row's weight:
 * VLNCE_WP_FLAG_PANO (pano outside [0, P]), and per component, shifted left by
 * VLNCE_WP_FLAG_SHIFT_OFFSET / _DISTANCE: VLNCE_WP_FLAG_LOC (loc outside the window, or NaN),
 * VLNCE_WP_FLAG_ELEMENT (element outside the window), VLNCE_WP_FLAG_VARIANCE (sqrt(variance) >= 0
 * fails), VLNCE_WP_FLAG_CLASS (class index outside [0, K)).  A flagged row is NaN in every output
 * and every gradient of that row, and nothing is read through its out-of-range index.
 *
 * saved [S][B] fp32 holds the partial derivatives (gate * weight folded in) the backward multiplies
 * with the incoming gradients (a discrete part's entropy planes without gate * weight, which its
 * backward takes from pano): S = 2 (P + 1) + n(offset) + n(distance), n = 0 / 4 / 2 K for an
 * absent / continuous / discrete part; saved_floats = the buffer's capacity (>= S * B, checked).
 *
 * vlnce_waypoint_eval_bwd: g_* = the gradient arriving at each block of out, in the block's shape
 * (NULL = zero); vlnce_wp_part_grad repeats the part's kind, K and weight; writes the DENSE
 * gradients d_logits [B,P+1] and, per part, d_first (shape of first) and d_second [B,P] (continuous
 * only) -- the zeros outside the chosen heading included, so nothing is zero-filled first.
 *
 * Shapes: B >= 1, 1 <= P <= 63, K <= 32 per discrete part (K_* = 0 for a part that is not discrete);
 * vlnce_waypoint_eval_supported says so, and both launches refuse anything else, and null pointers,
 * before they launch. */
enum { VLNCE_WP_ABSENT = 0, VLNCE_WP_CONTINUOUS = 1, VLNCE_WP_DISCRETE = 2 };
enum {
  VLNCE_WP_FLAG_PANO = 1,
  VLNCE_WP_FLAG_LOC = 1,
  VLNCE_WP_FLAG_ELEMENT = 2,
  VLNCE_WP_FLAG_VARIANCE = 4,
  VLNCE_WP_FLAG_CLASS = 8,
  VLNCE_WP_FLAG_SHIFT_OFFSET = 4,
  VLNCE_WP_FLAG_SHIFT_DISTANCE = 8
};
typedef struct {
  int kind;
  int K;
  float lo;
  float hi;
  float weight;
  const float* first;
  const float* second;
  const void* element;
} vlnce_wp_part;
typedef struct {
  int kind;
  int K;
  float weight;
  float* d_first;
  float* d_second;
} vlnce_wp_part_grad;
int vlnce_waypoint_eval_supported(int B, int P, int K_offset, int K_distance);
int vlnce_waypoint_eval(const float* logits, const int64_t* pano, const vlnce_wp_part* offset,
                        const vlnce_wp_part* distance, int B, int P, float* out,
                        long out_floats, float* saved, long saved_floats, int32_t* flags,
                        vlnce_stream_t stream);
int vlnce_waypoint_eval_bwd(const float* g_logp, const float* g_ent_pano, const float* g_ent_offset,
                            const float* g_ent_distance, const int64_t* pano, const float* saved,
                            const int32_t* flags, const vlnce_wp_part_grad* offset,
                            const vlnce_wp_part_grad* distance, int B, int P, float* d_logits,
                            vlnce_stream_t stream);

/* The optimizer step of both reference trainers over a LIST of fp32 tensors (ABI 152): torch.optim.Adam
 * (base_il_trainer.py:69-77, ddppo_waypoint_trainer.py:441) with torch.nn.utils.clip_grad_norm_ in front
 * (WDDPPO.before_step), as two launches: vlnce_grad_sumsq (only when clipping), then vlnce_adam_step.
 * No atomics, no grid-wide and no host synchronisation; every element is evaluated in fp64 and rounded
 * once per store, and the reduction orders are fixed: two runs from the same state give the same bits.
 *
 * table (device, int64 words) is the stable half of the list, built by the caller once per parameter set:
 *   n_tensors x { p, m, v (addresses of fp32 arrays), numel }, then n_chunks words, one per
 *   vlnce_adam_chunk() elements of a tensor: tensor index << 32 | chunk index inside that tensor.
 * A launch takes at most vlnce_adam_max_tensors() tensors; a longer list is split by the caller, each
 * part with a table of its own.  The half that changes every step is read from HOST arrays at the call and
 * travels by value in the kernel arguments (nothing is staged that a later call could overwrite):
 *   grads[t]         the gradient's address; NULL skips the tensor entirely (torch: grad is None).  Read only.
 *   step_size[t]     lr / (1 - beta1^t),  inv_bc2_sqrt[t] = 1 / sqrt(1 - beta2^t), t = the tensor's OWN step
 *                    count after increment, computed in double as torch does
 * Arrays may be views: 16-byte accesses are used where p, g, m, v of a chunk are all 16-byte aligned, a
 * scalar path otherwise (decided per workgroup); either way element i of a chunk belongs to the same thread.
 *
 * vlnce_grad_sumsq: workgroup w of VLNCE_ADAM_PARTIALS adds the squares of the gradients in chunks w,
 * w + VLNCE_ADAM_PARTIALS, ... in fp64 and stores partials[w] (accumulate = 0) or adds to it (accumulate != 0:
 * the second and later parts of a split list), so the norm spans every part.
 * vlnce_adam_step: with partials != NULL every workgroup adds the VLNCE_ADAM_PARTIALS values in one fixed
 * order, total_norm = sqrt(sum), coef = min(1, max_norm / (total_norm + 1e-6)) (NaN stays NaN), and
 * workgroup 0 stores (float) total_norm to norm_out (if not NULL); partials == NULL: coef = 1.  Then
 *   g = coef * g;  g += weight_decay * p  (weight_decay != 0)
 *   m += (g - m) (1 - beta1);  v = beta2 v + (1 - beta2) g g
 *   p -= step_size * m / (sqrt(v) * inv_bc2_sqrt + eps)
 * The gradients themselves stay unclipped: the one observable difference from clip_grad_norm_.
 * A NULL table, grads or partials of vlnce_grad_sumsq, n_tensors outside 1..vlnce_adam_max_tensors() and
 * n_chunks outside 0..2^31-1 are refused before anything is launched (vlnce_adam_supported says so). */
enum { VLNCE_ADAM_PARTIALS = 512 };
int vlnce_adam_supported(int n_tensors, long n_chunks);
int vlnce_adam_max_tensors(void);
int vlnce_adam_chunk(void);
int vlnce_grad_sumsq(const int64_t* table, int n_tensors, long n_chunks, const float* const* grads,
                     double* partials, int accumulate, vlnce_stream_t stream);
int vlnce_adam_step(const int64_t* table, int n_tensors, long n_chunks, const float* const* grads,
                    const double* step_size, const double* inv_bc2_sqrt, const double* partials,
                    double max_norm, double beta1, double beta2, double eps, double weight_decay,
                    float* norm_out, vlnce_stream_t stream);

/* DD-PPO rollout storage (ABI 153): ActionDictRolloutStorage of
 * vlnce_baselines/common/rollout_storage.py keeps its arenas [T+1, N, ...] on the device and moves rows
 * with ~17 copy_ launches per simulator step (insert, :85-111), ~11 per after_update (:113-125) and a
 * Python loop over environments with ~25 stack / view launches per minibatch (recurrent_generator,
 * :154-276).  Here each of those is ONE launch over a TABLE of fields, the large sensors and the
 * one-element rows alike.  The tables and the environment indices are HOST arrays, read during the call
 * and carried in the kernel arguments: no upload, no allocation, no synchronisation.  Plain vector loads
 * and stores only; all index arithmetic is 64-bit; element dtypes are the VLNCE_TRAJ_* codes.
 *
 * vlnce_rollout_copy: for every field f and row r < n_rows, E_f contiguous elements go from
 * src_f + r*src_row_stride_f to dst_f + r*dst_row_stride_f (strides in elements of the own dtype; with
 * n_rows == 1 they are not read), converted from src_dtype to dst_dtype.  Supported pairs, exactly:
 * f32->f32, i64->i64, u8->u8 (a bool source is u8), i64->f32, u8->f32, and f32->i64 / f32->u8, which are
 * defined only for finite values that the target represents exactly (masks, action indices).
 * vlnce_rollout_copy_supported says so; any other pair is refused before anything is launched.  A row is
 * dealt out in chunks of VLNCE_ROLLOUT_CHUNK elements, one workgroup each (a 7 MB row is spread over the
 * machine); rows shorter than 256 elements are packed, one thread per element (a 1-element row costs one
 * thread).  A field takes 16-byte accesses when both pointers and both row strides IN BYTES are 16-byte
 * aligned and the dtypes are equal (a chunk's offset always is); otherwise, and for the tail of a row
 * behind its last whole 16 bytes, one element per access.  Source and destination ranges of one call must
 * not overlap (after_update with step == 0 is the caller's no-op).  At most VLNCE_ROLLOUT_MAX_FIELDS
 * fields per call: the caller splits a longer table.
 *
 * vlnce_rollout_gather: the minibatch of recurrent_generator.  For every field and t < T_f (T_f = T, or 1
 * for a field with once != 0: the initial hidden state, whose output is [n_envs, L, H]):
 *   out_f[(t*out_N_f + j)*E_f + e] = arena_f[(t*N_f + envs[j])*E_f + e],   j < n_envs, e < E_f
 * without conversion (elem_bytes 1 | 2 | 4 | 8).  Rows are time-major, t*n' + j.  At most
 * VLNCE_ROLLOUT_MAX_ENVS environments per call: with more, the caller issues one call per 64, each with
 * `out` advanced by 64*E_f elements and out_N_f the environment count of the WHOLE output (the output's
 * time stride), which is why out_N is a field of its own and not n_envs.  Every envs[j] in [0, N_f).  The
 * 16-byte path as above: arena and out 16-byte aligned and E_f*elem_bytes a multiple of 16.
 *
 * vlnce_ppo_advantages: WDDPPO.get_advantages (ddppo_alg.py:30-35) in one launch of ONE workgroup.
 * returns / value_preds [T+1, N] (they carry the bootstrap row), adv [T, N].  d = returns - value_preds in
 * fp32, one rounding, as torch; normalize == 0: adv = d, bit for bit.  Otherwise the mean and the unbiased
 * standard deviation (divisor T*N - 1, as torch.std) of the fp32 d are taken in fp64 in a fixed order (two
 * runs give the same bits), and adv = (d - mean) / (std + eps) is evaluated in fp64 and rounded once.
 * T*N == 1 gives NaN, as torch does. */
#define VLNCE_ROLLOUT_MAX_FIELDS 32
#define VLNCE_ROLLOUT_MAX_ENVS 64
#define VLNCE_ROLLOUT_CHUNK 4096
typedef struct {
  const void* src;      /* row 0 of the source                                           */
  void* dst;            /* row 0 of the destination                                      */
  long E;               /* elements per row, > 0                                         */
  long src_row_stride;  /* in elements of src_dtype, >= 0                                */
  long dst_row_stride;  /* in elements of dst_dtype, >= E                                */
  int src_dtype;        /* VLNCE_TRAJ_F32 | _I64 | _U8                                   */
  int dst_dtype;        /* VLNCE_TRAJ_F32 | _I64 | _U8                                   */
} vlnce_rollout_field;
typedef struct {
  const void* arena;    /* [>= T_f, N, E]                                                */
  void* out;            /* [T_f, out_N, E], at its first environment column of this call */
  long E;               /* elements per (step, environment), > 0                         */
  long N;               /* environments of the arena                                     */
  long out_N;           /* environments of the whole output, >= n_envs                   */
  int elem_bytes;       /* 1 | 2 | 4 | 8                                                 */
  int once;             /* != 0: T_f = 1 whatever T                                      */
} vlnce_rollout_gfield;
int vlnce_rollout_copy_supported(int src_dtype, int dst_dtype);
int vlnce_rollout_copy(const vlnce_rollout_field* fields, int n_fields, int n_rows,
                       vlnce_stream_t stream);
int vlnce_rollout_gather(const vlnce_rollout_gfield* fields, int n_fields, const int* envs, int n_envs,
                         int T, vlnce_stream_t stream);
int vlnce_ppo_advantages(const float* returns, const float* value_preds, float* adv, int T, int N,
                         int normalize, float eps, vlnce_stream_t stream);

/* The rollout step of the Waypoint DD-PPO trainer on the device (ABI 154): everything
 * WaypointPolicy.act does behind the net (waypoint_policy.py:129-247 over the distributions of
 * models/utils.py) in ONE launch, and the trainer's pick of the observation history
 * (ddppo_waypoint_trainer.py:190-200) in one more.
 *
 * vlnce_waypoint_act: one thread per row, every row in fp64, one rounding to fp32 per store, no atomics.
 * It draws no random numbers itself: u [B,3] holds fp32 uniforms in [0, 1) (column 0 the panorama
 * choice, 1 the offset, 2 the distance; NULL, and not read, when deterministic != 0), so the launch is a
 * pure function of its inputs: two runs give the same bits.
 *
 * logits [B,P+1] are the RAW panorama logits; offset / distance are vlnce_wp_part descriptors as for
 * vlnce_waypoint_eval, `element` unused, and for a discrete part lo / hi unused.  Per row:
 *   panorama   c = the first maximum of logits[b,:] (deterministic), else with p_j = exp(z_j - max z) and
 *              S = sum_j p_j added up in index order, the first k with sum_{j<=k} p_j > u0 * S, and the last
 *              class of non-zero probability when there is none.  h = c mod P, gate = (c != P).
 *   continuous loc = first[b,h], scale = sqrt(second[b,h]), [a, b] = ([lo, hi] - loc) / scale.  The element is
 *              loc (deterministic), else loc + scale * ncdfinv(cdf(a) + u_k (cdf(b) - cdf(a))): the truncated
 *              normal of the reference exactly, by inverse CDF (the device library's normcdfinv) where the
 *              reference samples by rejection.  It is rounded to fp32 and clamped into [lo, hi].  mode = loc,
 *              variance = scale^2 (1 + e2 - e1^2), e1 = (pdf(a) - pdf(b)) / mass, e2 = (a pdf(a) - b pdf(b)) / mass.
 *   discrete   the element is the class drawn from first[b,h,:] by the panorama's rule with its own u_k
 *              (deterministic: the first maximum), mode = the first maximum.  The variance is NaN, [B]: what
 *              torch.distributions.Categorical.variance of the reference's class holds.
 *   log_prob   log_softmax(z)[c] + gate * weight * logp_distance + gate * weight * logp_offset, each part's
 *              term evaluated FROM THE ROUNDED fp32 ELEMENT by the formulas of vlnce_waypoint_eval (shared
 *              code), so the number a rollout stores is the one evaluate_actions scores; a part of weight 0 adds
 *              nothing, as the reference skips it.
 *   metric     what the simulator gets: the continuous element itself, or the bin centre
 *              bin_lo + k (bin_hi - bin_lo) / (K - 1) of class k.
 * A part of weight 0 (`predict_* = False`, WaypointPolicy._draw) stores off_element (continuous) or class 0
 * as its element, hands off_metric to the simulator, and has variance 0; its mode stays.
 * norm_logits [B,P+1] = z - logsumexp(z): the returned distribution needs no further launch.
 * theta = (h 2 pi / P + the offset's metric) mod 2 pi, in [0, 2 pi).
 *
 * flags[b] take the place of the reference's constructor assertions: VLNCE_WP_FLAG_PANO = a panorama logit
 * that is not finite, and per part (shifted as for vlnce_waypoint_eval) VLNCE_WP_FLAG_LOC and
 * VLNCE_WP_FLAG_VARIANCE at the chosen heading.  A flagged row is STOP in host_rows, NaN in every float
 * output, pano = P and class 0.
 * host_rows [B,8] fp32, the ONE buffer the host reads back: stop (0 | 1), r (the distance's metric), theta,
 * the stored distance element in metres, the stored offset element in radians (what the trainer logs: they
 * differ from r / theta's offset only for a part of weight 0), distance variance, offset variance, flags
 * (small integers, exact in fp32).
 *
 * Shapes as vlnce_waypoint_eval_supported; anything else, and null pointers, are refused before launch.
 *
 * vlnce_waypoint_history_pick: one launch over a table of fields (at most VLNCE_WP_HISTORY_MAX_FIELDS),
 * carried in the kernel arguments.  src_f is [B,P,E_f] with src_row_stride elements between environments
 * (a slice of a larger arena), dst_f [B,E_f] contiguous, dtype VLNCE_TRAJ_F32 or VLNCE_TRAJ_U8:
 *   dst_f[b,:] = src_f[b, pano[b], :] when 0 <= pano[b] < P, zeros otherwise (STOP, or a flagged row)
 * pano (int64 [B]) is read on the device: the previous launch's output on the same stream.  Rows are dealt
 * out in VLNCE_ROLLOUT_CHUNK pieces, one workgroup each; 16-byte accesses where both pointers, the row stride
 * in bytes and E_f * elem_bytes are multiples of 16, one element per access otherwise.  Plain vector loads
 * and stores only. */
#define VLNCE_WP_HISTORY_MAX_FIELDS 8
typedef struct {
  double bin_lo;      /* discrete: the metric of class 0                                   */
  double bin_hi;      /* discrete: the metric of class K - 1                               */
  float off_metric;   /* weight 0: the metric handed to the simulator                      */
  float off_element;  /* weight 0, continuous: the stored element                          */
  void* element;      /* out: float [B] (continuous) or int64 [B] (discrete)               */
  void* mode;         /* out: as element                                                   */
  float* variance;    /* out: [B]                                                          */
} vlnce_wp_act_part;
typedef struct {
  const void* src;      /* [B, P, E], environments src_row_stride elements apart           */
  void* dst;            /* [B, E]                                                          */
  long E;               /* elements per (environment, panorama), > 0                       */
  long src_row_stride;  /* in elements, >= P * E                                           */
  int dtype;            /* VLNCE_TRAJ_F32 | VLNCE_TRAJ_U8                                  */
} vlnce_wp_history_field;
int vlnce_waypoint_act_supported(int B, int P, int K_offset, int K_distance);
int vlnce_waypoint_act(const float* logits, const vlnce_wp_part* offset, const vlnce_wp_part* distance,
                       const vlnce_wp_act_part* offset_out, const vlnce_wp_act_part* distance_out,
                       int deterministic, const float* u, int B, int P, int64_t* pano, float* log_prob,
                       float* norm_logits, float* host_rows, int32_t* flags, vlnce_stream_t stream);
int vlnce_waypoint_history_pick(const vlnce_wp_history_field* fields, int n_fields, const int64_t* pano,
                                int B, int P, vlnce_stream_t stream);

/* The trunk-feature cache of the Waypoint DD-PPO loop (ABI 155).  Both visual encoders of the Waypoint
 * trainer are frozen (models/encoders/resnet_encoders.py:46,142) and in eval mode while rollouts are
 * collected and while the agent is updated (ddppo_waypoint_trainer.py:496,526-530): a trunk's output is a
 * fixed function of one frame.  A rollout therefore keeps the trunk outputs beside the frames, and these
 * two entry points move them; both are pure data movement over a table of fp32 fields (at most
 * VLNCE_WP_FEATURE_MAX_FIELDS, carried in the kernel arguments) by the recipe of vlnce_rollout_copy and
 * vlnce_waypoint_history_pick: rows dealt out in VLNCE_ROLLOUT_CHUNK pieces, one workgroup each; 16-byte
 * accesses where every pointer of the field, every stride in bytes and F_f * 4 are multiples of 16, one
 * element per access otherwise; plain vector loads and stores only; no host synchronisation, no
 * allocation, nothing staged that a later call could overwrite.  Strides are in elements.  Refused before
 * anything is launched (non-zero, vlnce_last_error): a null pointer, n_fields outside
 * 1..VLNCE_WP_FEATURE_MAX_FIELDS, B <= 0, P <= 0, F_f <= 0, a stride smaller than its row, a pointer off
 * its 4 bytes, a mask dtype other than the two named.
 *
 * vlnce_waypoint_feature_pick: the next step's history features.  src_f is [B,P,F_f] with src_row_stride
 * elements between environments (a slice of an arena), zero_f [F_f], dst_f [B,F_f] contiguous:
 *   dst_f[b,:] = src_f[b, pano[b], :] when 0 <= pano[b] < P, zero_f otherwise (STOP, or a flagged row)
 * pano (int64 [B]) is read on the device: vlnce_waypoint_act's output on the same stream.  zero_f is the
 * trunk's output for an all-zero frame: what the encoder makes of the zeros vlnce_waypoint_history_pick
 * stores for such a row.
 *
 * vlnce_waypoint_feature_rows: the encoder's batch of B * (P + 1) frames, from features
 * (waypoint_predictors.py:330-341: the history frame times its not-done mask behind the panorama).
 * pano_f [B,P,F_f] and hist_f [B,F_f], each with its own row stride, zero_f [F_f], out_f [B,P+1,F_f]
 * contiguous:
 *   out_f[b,j,:] = pano_f[b,j,:] for j < P;   out_f[b,P,:] = hist_f[b,:] when masks[b] != 0, else zero_f
 * masks [B] is uint8 (mask_dtype VLNCE_TRAJ_U8) or fp32 (VLNCE_TRAJ_F32), the two dtypes in which the
 * storage and the net hold it. */
#define VLNCE_WP_FEATURE_MAX_FIELDS 8
typedef struct {
  const float* src;     /* [B, P, F], environments src_row_stride elements apart           */
  const float* zero;    /* [F]                                                             */
  float* dst;           /* [B, F]                                                          */
  long F;               /* elements per (environment, panorama), > 0                       */
  long src_row_stride;  /* in elements, >= P * F                                           */
} vlnce_wp_feature_pick_field;
typedef struct {
  const float* pano;    /* [B, P, F], environments pano_row_stride elements apart          */
  const float* hist;    /* [B, F], environments hist_row_stride elements apart             */
  const float* zero;    /* [F]                                                             */
  float* out;           /* [B, P + 1, F]                                                   */
  long F;               /* elements per (environment, panorama), > 0                       */
  long pano_row_stride; /* in elements, >= P * F                                           */
  long hist_row_stride; /* in elements, >= F                                               */
} vlnce_wp_feature_rows_field;
int vlnce_waypoint_feature_pick(const vlnce_wp_feature_pick_field* fields, int n_fields, const int64_t* pano,
                                int B, int P, vlnce_stream_t stream);
int vlnce_waypoint_feature_rows(const vlnce_wp_feature_rows_field* fields, int n_fields, const void* masks,
                                int mask_dtype, int B, int P, vlnce_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VLNCE_HIP_H */
