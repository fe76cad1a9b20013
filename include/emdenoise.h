/* emdenoise.h -- C ABI of libemdenoise.so: MI355X (gfx950) kernels for the micrograph-denoising
 * hot path of Jeffrey-Ede/AI-CV-Automation-Elect-Micr.
 *
 * The reference has no FFI / plugin interface for this path: its arithmetic is a graph of stock
 * TensorFlow ops built by Python.  Each entry point below therefore replaces the
 * TensorFlow op call(s) cited next to it ("replaces: file:line"), and is bound from Python with
 * ctypes exactly as INTEGRATION.md shows.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ or torch types.
 *   - Every data pointer is a DEVICE pointer unless its name ends in _host.
 *   - Activations are NHWC float32 (reference: data_format='NHWC', machine_learning/denoiser.py:120;
 *     placeholders tf.float32, :613).  A tensor may be a channel slice of a wider buffer: it is
 *     described by its channel count C and its pixel stride ld (elements between consecutive
 *     pixels, ld >= C), which is how tf.concat (denoiser.py:203, :353, :365) is made free.
 *   - The caller owns every buffer; the library allocates no device memory and keeps no global
 *     mutable state.  Every call takes the hipStream_t to launch on (as void*), is asynchronous
 *     with respect to the host and is safe to capture into a hipGraph.
 *   - Return value: EMD_OK (0) or a negative EMD_E_* code; emd_last_error() returns a
 *     thread-local description of the last failure on the calling thread.  Nothing throws
 *     across the ABI.
 */
#ifndef EMDENOISE_H
#define EMDENOISE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMD_VERSION 100 /* 0.1.0 */

#define EMD_OK 0
#define EMD_E_INVALID (-1)     /* bad argument (null pointer, non-positive size, bad enum) */
#define EMD_E_UNSUPPORTED (-2) /* valid request this build has no kernel for */
#define EMD_E_ALIGN (-3)       /* pointer / stride alignment requirement not met */
#define EMD_E_LAUNCH (-4)      /* HIP reported an error at launch */
#define EMD_E_ALLOC (-5)       /* a device allocation or upload inside the library failed (emd_graph_create only) */

typedef void* emd_stream_t; /* hipStream_t */

int emd_version(void);
const char* emd_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Graph K: the learned symmetric-kernel ("dedicated kernel") denoiser.
 * replaces: misc_py/noise-removal-kernels.py:99-105 (tf.pad REFLECT), :378-399 (filter_fn:
 *           W0*P -> [ +Bi -> sigmoid -> fully_connected scalar -> Wi* ] x (depth-1) -> reduce_sum),
 *           :409-426 (the per-pixel Python loop that instantiates filter_fn at every pixel), and the
 *           per-pixel sess.run loop of misc_py/apply_kernels+MLPs.py:669-698.
 *
 * x, y     : [B,H,W] float32 (NHWC with C == 1); y may not alias x.
 * width    : odd kernel width w, 3..EMD_K_MAX_WIDTH; REFLECT padding needs w/2 < min(H,W).
 * depth    : 1..EMD_K_MAX_DEPTH.
 * params   : device float array, emd_kernel_params_count(width, depth) elements:
 *              wmaps [depth][w*w]   full w x w weight maps W0..W(depth-1)
 *              bmaps [depth][w*w]   bias maps (bmaps[0] is ignored)
 *              s     [depth]        fully_connected scalars (s[0] is ignored)
 * flags    : EMD_K_SYMMETRIC asserts that every map is D4-symmetric (as make_layer,
 *            noise-removal-kernels.py:107-358, always builds them); it enables the kernel that
 *            evaluates 3 sigmoids per input pixel instead of 9 per output pixel.  Results are
 *            undefined if the flag is set for maps that are not symmetric.
 * The image is returned un-transposed (the trainer's transposed assembly at :421-424 is undone by
 * the reference itself at :712).
 */
#define EMD_K_MAX_WIDTH 15
#define EMD_K_MAX_DEPTH 5
#define EMD_K_SYMMETRIC 1u

size_t emd_kernel_params_count(int width, int depth);
int emd_kernel_denoise_f32(const float* x, float* y, int B, int H, int W, int width, int depth,
                           const float* params, unsigned flags, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Graph K training (csrc/k_train.hip).
 * replaces: misc_py/noise-removal-kernels.py:409-446 (the unrolled per-pixel filter graph, its MSE loss, TF's gradient and
 *           one AdamOptimizer per filter), :665-678 (lr = lr0 (1 - t / (T + 1))), :450-538 (the host input path).
 *
 * The trainable state of one (depth, width) filter is `theta`, emd_k_train_scalar_count(width, depth) float32 make_layer
 * scalars (nsym = (o+1)(o+2)/2 per map, o = width/2, in make_layer's creation order x = 0..o, y = 0..x):
 *     w [depth][nsym]   the weight maps w0 .. w(depth-1)
 *     b [depth-1][nsym] the bias maps b1 .. b(depth-1)
 *     s [depth-1]       the fully_connected scalars s1 .. s(depth-1)
 * A scalar's gradient is the sum over the D4-symmetric taps that share it.
 *
 * emd_k_train_step_f32: one training (or evaluation) step on a device batch x [B,H,W] (any B, H, W; width/2 < min(H,W)).
 *   loss_mode EMD_K_LOSS_REFERENCE: mean((F(x)^T - x)^2), what the reference minimises (its output is assembled
 *             transposed, :421-424; H == W);  EMD_K_LOSS_IMAGE: mean((F(x) - x)^2).
 *   flags     EMD_K_TRAIN_UPDATE: apply TF's Adam to theta with adam_m / adam_v and the device step counter *step (completed
 *             steps; incremented), lr_t = lr sqrt(1-beta2^t)/(1-beta1^t), lr = float32(lr0 (1 - t/(total_steps+1))), t = *step + 1.
 *             EMD_K_TRAIN_LOSS_ONLY: forward pass and loss only (no backward, no update).  Neither: loss and gradient.
 *   grad_out  [nscal] dL/dtheta (NULL: not stored); loss_out [1] the loss with the parameters BEFORE the update (NULL: not
 *             stored); params_out: the packed block of emd_kernel_denoise_f32 (emd_kernel_params_count) expanded from the
 *             updated theta (NULL: not written).  All device pointers; adam_m / adam_v / step may be NULL without UPDATE.
 *   workspace device scratch of emd_k_train_workspace_bytes(B, H, W, width, depth) bytes.
 * Deterministic: no atomics; the same inputs give the same bits. */
#define EMD_K_LOSS_REFERENCE 0
#define EMD_K_LOSS_IMAGE 1
#define EMD_K_TRAIN_UPDATE 1u
#define EMD_K_TRAIN_LOSS_ONLY 2u
size_t emd_k_train_scalar_count(int width, int depth);
size_t emd_k_train_workspace_bytes(int B, int H, int W, int width, int depth);
int emd_k_train_step_f32(const float* x, int B, int H, int W, int width, int depth, int loss_mode, float* theta, float* adam_m,
                         float* adam_v, int* step, double lr0, long total_steps, float beta1, float beta2, float eps,
                         unsigned flags, float* grad_out, float* loss_out, float* params_out, void* workspace,
                         size_t workspace_bytes, emd_stream_t stream);
/* The K trainer's input path on the device: B crops of crop x crop from the device stack [N,H,W] (H, W > crop).  Crop b draws
 * Philox4x32-10(counter = (first_index + b, 0, tag 4), key = seed) -> image n, offsets x = randint(0, H-crop),
 * y = randint(0, W-crop) (:457-462), D4 element (flip_rotate, :498-515), then NaN/Inf -> 0, scale0to1 (constant -> 0.5),
 * / mean (preprocess, :517-529) and all-zero if any value is non-finite (record_parser, :531-538).  draws_out (int32 [B][4] =
 * n, x, y, element; may be NULL) records the draws.  The trainer passes first_index = step * B. */
int emd_k_sample_crops_f32(const float* stack, int N, int H, int W, float* crops, int B, int crop, unsigned long long seed,
                           unsigned long long first_index, int* draws_out, emd_stream_t stream);
/* The fused small-batch form (the reference's 32 x 10 x 10): one workgroup per filter runs `nsteps` (1..EMD_K_FUSED_MAX_STEPS)
 * complete steps in one launch per depth present -- sample (as emd_k_sample_crops_f32, crop index (t-1) * B + b for the 1-based
 * step t read from the filter's counter) or take fixed batch (it % nbatches) of `batches` [nbatches][B][crop][crop] when that is
 * not NULL, then forward + backward, the reduction in LDS and Adam -- and writes the loss of every step to losses[it] (the
 * parameters before update it).  Needs B * crop^2 <= EMD_K_FUSED_MAX_PIXELS (the batch lives in LDS) and square crops.
 * Deterministic; it sums in another order than emd_k_train_step_f32 (and the sampled crops' means may differ in the last bit),
 * so the two forms agree to rounding, not bit for bit.  params_out may be NULL; every other job pointer is required. */
#define EMD_K_FUSED_MAX_STEPS 1000
#define EMD_K_FUSED_MAX_PIXELS 8192
typedef struct {
    float* theta;      /* [emd_k_train_scalar_count] */
    float* adam_m;
    float* adam_v;
    int* step;         /* completed steps; advanced by nsteps */
    float* params_out; /* packed emd_kernel_denoise_f32 block after the last step, or NULL */
    float* losses;     /* [nsteps] */
    int width;
    int depth;
} emd_k_fused_job_t;
int emd_k_train_fused_f32(const emd_k_fused_job_t* jobs, int njobs, const float* stack, int N, int H, int W, const float* batches,
                          int nbatches, int B, int crop, unsigned long long seed, int nsteps, int loss_mode, double lr0,
                          long total_steps, float beta1, float beta2, float eps, emd_stream_t stream);

/* Paired training (csrc/k_pair.hip): the filter is trained to turn x into a second tensor, `truth`.
 * replaces: misc_py/noise_removal_kernels_duplicate.py:406-434 (the filter over the unpadded patch, the interior target, the MSE
 *           and its sqrt rule), :449 and :720-724 (Adam at beta1 = 0.5, lr = 0.01 (1 - t / 10001)) -- the caller passes those.
 *
 * emd_k_train_pair_step_f32: emd_k_train_step_f32 with two device batches x and truth, both [B,H,W].  theta, the Adam
 *   arguments, grad_out / loss_out / params_out and the workspace (emd_k_train_workspace_bytes(B, H, W, width, depth) bytes) are
 *   as there.  What differs:
 *   pad_mode  EMD_K_PAD_VALID: no padding (pad(inputs, (0, 0)), :406).  The filter is evaluated on the (H-w+1) x (W-w+1)
 *             interior only, no mirrored tap is read, and output pixel (r, c) is compared with truth[r + w/2][c + w/2]
 *             (:431-432).  Needs width <= min(H,W).  EMD_K_PAD_REFLECT: emd_k_train_step_f32's border rule, output H x W,
 *             compared with truth[r][c]; needs width/2 < min(H,W).
 *   target    F(x) against truth in image orientation.  The reference assembles its output transposed (:425-428) and is fed
 *             the truth transposed (:735-736); the two cancel, so there is no "reference" / "image" choice here.
 *   loss      L = mean((F(x) - truth)^2) over the compared pixels.  With EMD_K_TRAIN_SQRT_ABOVE_1 the loss is sqrt(L) when
 *             L > 1 (:433; at exactly L == 1 the plain branch holds) and the gradient is then dL/dtheta / (2 sqrt(L)); the
 *             factor is applied in the fixed-order reduction.  loss_out holds the value after this rule.
 *   flags     EMD_K_TRAIN_UPDATE, EMD_K_TRAIN_LOSS_ONLY or neither, as emd_k_train_step_f32; EMD_K_TRAIN_SQRT_ABOVE_1 with any.
 * Deterministic: no atomics; the same inputs give the same bits.
 *
 * emd_k_make_pairs_f32: misc_py/autoencoder_train-val-test.py:35-55 for a stack, one workgroup per image.  a (the autoencoder's
 *   input crops) and b (its outputs) are device [N,H,W].  Per image, separately for a[n] and b[n]: c = min (NaN if any pixel
 *   is, as np.min), m = float32(mean, accumulated in double) - c, img = (img - c) / m in float32 (:38-44).  One offset pair
 *   (i, j) per image, the same for both, each uniform in [lo, hi) (np.random.randint(lo, hi), :51-52; the reference's 20 and
 *   160 - 40): Philox4x32-10(counter = (first_index + n, 0, tag 6), key = seed), i from word 0 and j from word 1.
 *   x, t [N,patch,patch] receive a's and b's patch at (i, j); draws_out (int32 [N][2] = i, j; may be NULL) the draws.  If
 *   either patch holds a non-finite value (a flat image has m == 0) both become 0.5, the rule of the paired trainer's
 *   record_parser (noise_removal_kernels_duplicate.py:534-548).  Needs 0 <= lo < hi and hi - 1 + patch <= min(H,W). */
#define EMD_K_PAD_REFLECT 0
#define EMD_K_PAD_VALID 1
#define EMD_K_TRAIN_SQRT_ABOVE_1 4u
int emd_k_train_pair_step_f32(const float* x, const float* truth, int B, int H, int W, int width, int depth, int pad_mode,
                              float* theta, float* adam_m, float* adam_v, int* step, double lr0, long total_steps, float beta1,
                              float beta2, float eps, unsigned flags, float* grad_out, float* loss_out, float* params_out,
                              void* workspace, size_t workspace_bytes, emd_stream_t stream);
int emd_k_make_pairs_f32(const float* a, const float* b, int N, int H, int W, int patch, int lo, int hi, unsigned long long seed,
                         unsigned long long first_index, float* x, float* t, int* draws_out, emd_stream_t stream);
/* The inverse map of autoencoder.Micrograph_Autoencoder.denoise_crop (apply_autoencoders.py:376-381), one workgroup per crop:
 * pred, out [N][npix] (out may alias pred), crop_stats [N][2] = (offset, scale) as emd_tile_gather_f32 writes them.
 * out = scale * pred + offset in float32 (multiply, then add), or pred * offset / mean(pred) where scale == 0 (a flat crop; the
 * mean accumulated in double and rounded once). */
int emd_s_crop_unscale_f32(const float* pred, const float* crop_stats, int N, int npix, float* out, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Graph S training (misc_py/autoencoder.py:177-274 trains the separable autoencoder of apply_autoencoders.py:91-187).
 * The reverse pass of the encoder and decoder is the graph-D' entry points (batch-form norms with mask 4, relu); these
 * are the parts that are S's own.
 * emd_s_sample_crops_f32: emd_k_sample_crops_f32's input path with graph S's differences: Philox tag 5 (its own stream),
 *   a crop with any non-finite value after preprocess becomes ONES (autoencoder.py:271-272), and x4 (may be NULL)
 *   receives a copy of every crop in channel 0 of the [B][crop][crop][4] tensor the first separable block reads (its
 *   channels 1..3 are not touched: the caller keeps them zero).  crops [B][crop][crop] is the loss target.
 *   first_index_dev (device uint64, may be NULL) replaces first_index when given: a captured graph's crop index.
 * emd_s_head_bwd_f32: the loss and the reverse pass of the last two layers, a = relu(conv2d_transpose + bias) [B,H,W,C]
 *   (pitch lda) and out = conv2d(a, w9 [9][C], 3x3 SAME, no bias) [B,H,W], for L = sum (out - x)^2 / (B*H*W) with target
 *   x [B,H,W]: dout = 2 (out - x) / (B*H*W) is formed in registers and never written; dw9 [9][C] += dL/dw9;
 *   da (pitch ldo; may be a itself) = [a > 0] * (3x3 transpose of dout) = dL/d(pre-activation); dbias [C] += sum of da
 *   (may be NULL); loss_out[0] = L.  C a power of two, 4..256.  workspace: emd_s_head_bwd_workspace_bytes(B, H, W, C)
 *   bytes (per-tile partial sums, reduced in a fixed order: deterministic).
 * emd_s_mse_loss_f32: loss_out[0] = sum (out - x)^2 / n; dout (may be NULL) = 2 (out - x) / n.  workspace:
 *   emd_s_mse_loss_workspace_bytes() bytes.  With emd_conv3x3_cout1_wgrad_f32, emd_conv3x3_cout1_bwd_data_f32,
 *   emd_relu_mask_bwd_f32 and emd_bn_bwd_reduce_f32 (x NULL, accumulate_s1) it is the composed form of emd_s_head_bwd_f32.
 * emd_relu_mask_bwd_f32: dr = [a > 0] * g over n floats (n a multiple of 4; dr may be g). */
int emd_s_sample_crops_f32(const float* stack, int N, int H, int W, float* crops, float* x4, int B, int crop, unsigned long long seed,
                           unsigned long long first_index, const unsigned long long* first_index_dev, int* draws_out,
                           emd_stream_t stream);
size_t emd_s_head_bwd_workspace_bytes(int B, int H, int W, int C);
int emd_s_head_bwd_f32(const float* out, const float* x, const float* a, int lda, const float* w9, int B, int H, int W, int C, float* da,
                       int ldo, float* dw9, float* dbias, float* loss_out, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_s_mse_loss_workspace_bytes(void);
int emd_s_mse_loss_f32(const float* out, const float* x, long n, float* loss_out, float* dout, void* workspace, emd_stream_t stream);
int emd_relu_mask_bwd_f32(const float* a, const float* g, float* dr, long n, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Graph D: the depthwise-separable encoder-decoder (machine_learning/denoiser.py:58-398).
 *
 * Fused epilogue shared by the matrix-core entry points (per output channel n):
 *     v = acc * scale1[n] + shift1[n]          conv bias and the inference batch norm(s) folded
 *     if (act)    v = min(max(v,0),6)          tf.nn.relu6                        (denoiser.py:83)
 *     if (scale2) v = relu6(v*scale2[n]+shift2[n])   a second batch_then_activ  (:170,:176,:182)
 *     if (res)    v += res[pixel][n]           the "+=" residual that follows     (:264 ...)
 * scale*, shift*: device float[Cout]; scale2/shift2/res may be NULL.
 *
 * precision: EMD_PREC_BF16X3 (split-bf16, 3 MFMA passes, ~2^-16 relative: the parity mode) or
 *            EMD_PREC_BF16   (one bf16 MFMA pass, ~2^-9 relative per layer: the fast mode).
 */
#define EMD_PREC_BF16 1
#define EMD_PREC_BF16X3 3

/* activation codes of the `act` arguments (applied after the first affine, and after the second if present) */
#define EMD_ACT_NONE 0
#define EMD_ACT_RELU6 1 /* tf.nn.relu6: machine_learning/denoiser.py:83 */
#define EMD_ACT_RELU 2  /* tf.nn.relu:  misc_py/modified_Xception.py:209, :222, :312 */
#define EMD_ACT_LEAKY 4 /* tf.nn.leaky_relu, alpha 0.2: misc_py/gan-infilling-100.py:178 (matrix-core epilogues, emd_affine_act_f32) */
#define EMD_ACT_RELU6_CLIP01 3 /* relu6 then tf.clip_by_value(.,0,1), misc_py/denoiser-multi-gpu.py:534-538 (emd_affine_act_f32 only) */

/* Round 4: the two per-channel steps of the chain can run inside the kernel that finishes the reduction in front of them (one launch
 * less per layer and direction: ~700 launches of 4-5 us per training step, each a link in its stream's dependent chain).  The argument
 * blocks (host structs; every pointer a device pointer; [C], or [B][C] in the per-image forms, exactly as the separate calls take them):
 *   emd_bn_train_fold_t: emd_bn_train_fold[_images]_f32's parameters and outputs  -> emd_conv1x1_stats_fold_f32, emd_conv3x3_stats_fold_f32,
 *                        emd_deconv3x3s2_stats_fold_f32 (the conv, its output's statistics AND the fold: mean / var are still written)
 *   emd_bn_bwd_prep_t:   emd_bn_bwd_prep[_images]_f32's                            -> emd_bn_bwd_reduce_prep_f32, emd_dw3x3_bn_bwd_reduce_f32 */
typedef struct {
    const float *gamma1, *beta1, *gamma2, *beta2, *bias;   /* gamma1 / beta1 NULL: a single norm; bias NULL or the conv bias in front of it */
    float eps, pad_;
    float *scale, *shift, *rstd1, *rstd2;                  /* outputs (rstd2: the double norm only) */
    float *mm1, *mv1, *mm2, *mv2;                          /* moving statistics to update from image 0 / the batch, or all NULL */
    double decay;
} emd_bn_train_fold_t;
typedef struct {
    const float *gamma1, *gamma2, *rstd1, *rstd2;
    float eps, pad_;
    float *K, *m1, *m2;                                    /* outputs for the apply step */
    float *dgamma1, *dgamma2, *dbeta2;                     /* parameter gradients, ADDED into */
} emd_bn_bwd_prep_t;

/* Host-side weight packing for the matrix-core kernels (all pointers are HOST pointers).
 * w_host : taps x Cin x Cout float32 in TensorFlow order, [taps][Cin][Cout] (slim.conv2d /
 *          pointwise_weights, cout_major = 0) or [taps][Cout][Cin] (slim.conv2d_transpose, cout_major = 1).
 * hi/lo  : emd_packed_weight_elems(taps,Cin,Cout) bf16 words each: w = hi + lo (+2^-17), stored
 *          [Cout padded to 128][taps][Cin padded to 64], zero padded. */
size_t emd_packed_weight_elems(int taps, int Cin, int Cout);
int emd_pack_weights_bf16(const float* w_host, int taps, int Cin, int Cout, int cout_major,
                          uint16_t* hi_host, uint16_t* lo_host);

/* 1x1 convolution on the matrix cores, optional stride 2 (TF SAME for k=1: samples x[0::2]).
 * replaces: the pointwise half of slim.separable_convolution2d + normalizer BN + batch_then_activ
 *           (denoiser.py:113-134); slim.conv2d(kernel_size=1[,stride=2]) + bias + BN + relu6
 *           (:91-97 with :359/:371/:383, :159-164, :208-214, :220-227); the residual adds.
 * x [B,H,W,Cin] pixel stride ldx;  y [B,ceil(H/s),ceil(W/s),Cout] pixel stride ldy;  res like y, ldres.
 * Cin, Cout, ldx, ldy, ldres multiples of 4; x, y, res, whi, wlo, scale*, shift* 16-byte aligned.
 * wlo may be NULL with EMD_PREC_BF16. */
int emd_conv1x1_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo,
                    const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                    const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin,
                    int Cout, int stride, int act, int precision, emd_stream_t stream);
/* emd_conv1x1_f32 (stride 1) with a per-pixel shift: y = act((x . W) * scale1 + U), U = emd_resize_bilinear_f32 of up [B,Hu,Wu,Cout]
 * (pixel stride ldup) to [H,W], sampled in the epilogue with the resize kernel's arithmetic and never written.  For a 1x1 conv over
 * concat(resize(a), x): up = (a . W_a) * scale1 + shift1 at a's resolution, W = W_x (bilinear weights sum to 1).  scale2 / shift2 / res
 * must be NULL: EMD_E_UNSUPPORTED otherwise. */
int emd_conv1x1_up_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* up,
                       int ldup, int Hu, int Wu, const float* scale2, const float* shift2, const float* res, int ldres, float* y,
                       int ldy, int B, int H, int W, int Cin, int Cout, int act, int precision, emd_stream_t stream);

/* Dense 3x3 convolution on the matrix cores (9-tap implicit GEMM), TF SAME, stride 1 or 2, or stride 1 with
 * dilation `rate` <= 31.
 * replaces: tf.layers.conv2d(kernel_size=3[, dilation_rate=r]) + bias + BN + relu6 -- the ASPP rate branches
 *           of the training twin (misc_py/denoiser-multi-gpu.py:306-328).
 * whi/wlo: emd_pack_weights_bf16(taps = 9, w_host = [ky][kx][Cin][Cout]).  Alignment rules as emd_conv1x1_f32. */
int emd_conv3x3_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                    const float* shift1, const float* scale2, const float* shift2, const float* res, int ldres,
                    float* y, int ldy, int B, int H, int W, int Cin, int Cout, int stride, int rate, int act,
                    int precision, emd_stream_t stream);

/* tf.nn.pool(window_shape=(2,2), "AVG", "SAME", strides=(2,2)): y [B,ceil(H/2),ceil(W/2),C].
 * replaces: the image-level branch of the training twin's ASPP (misc_py/denoiser-multi-gpu.py:331-335). */
int emd_avgpool2x2_f32(const float* x, int ldx, float* y, int ldy, int B, int H, int W, int C,
                       emd_stream_t stream);

/* 3x3 stride-2 transposed convolution, output exactly 2H x 2W, as four output-phase GEMMs.
 * replaces: slim.conv2d_transpose(kernel_size=3, stride=2, padding='same') + bias + BN + relu6
 *           (denoiser.py:141-148):  y[2i+k] += x[i]*w[k], cropped at the end.
 * whi/wlo: HOST arrays of 4 DEVICE pointers, one packed block per phase (phase = 2*row_parity +
 *          col_parity) holding the taps emd_deconv_phase_taps lists, in that order, cout_major = 1. */
int emd_deconv_phase_taps(int phase, int* ky, int* kx);
int emd_deconv3x3s2_f32(const float* x, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                        const float* scale1, const float* shift1, float* y, int ldy, int B, int H, int W,
                        int Cin, int Cout, int act, int precision, emd_stream_t stream);

/* The whole strided_conv_block (denoiser.py:110-136) for stride 1 in ONE kernel: depthwise 3x3 (SAME) ->
 * pointwise 1x1 on the matrix cores -> fused epilogue (above).  The depthwise result never reaches HBM.
 * replaces: slim.separable_convolution2d + normalizer BN + batch_then_activ (+ the residual "+=").
 * Supported when emd_sep3x3_fused_supported() returns 1: stride 1, rate 1, H%8==0, W%16==0, Cin%32==0,
 * Cout%4==0, Cout<=128 (one N tile), or Cout<=256 with Cin<=256 (one 256-column tile on 4 x 16 pixels; no generated-input form);
 * otherwise call emd_dw3x3_f32 + emd_conv1x1_f32.
 * x [B,H,W,Cin] ldx; dw [3][3][Cin]; whi/wlo packed pointwise weights (taps=1); y [B,H,W,Cout] ldy. */
int emd_sep3x3_fused_supported(int H, int W, int Cin, int Cout, int stride, int rate);
int emd_sep3x3_fused_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                         const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                         const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin,
                         int Cout, int act, int precision, emd_stream_t stream);
/* The same block with stride 2 (strided_conv_block(stride=2), machine_learning/denoiser.py:258, :273, :288), one launch (round 3): x
 * [B,H,W,Cin] with H%8==0, W%32==0 (TF SAME on even sizes: no padding before, one pixel after), y [B,H/2,W/2,Cout], Cout <= 256,
 * res (optional) in the output's shape.  Split-bf16.  emd_sep3x3_fused_supported(H, W, Cin, Cout, 2, 1) says where it applies. */
int emd_sep3x3_fused_s2_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                            const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                            const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                            emd_stream_t stream);
/* The same with the residual GENERATED in the epilogue instead of read: res[b][oy][ox][c] = f(img[b][oy*img_stride][ox*img_stride] *
 * res_a[c] + res_t[c]), f = relu6 if res_act else the identity; img is a one-value-per-pixel tensor [B, H/2*img_stride, W/2*img_stride]
 * with pixel pitch ldimg floats.  Bit for bit emd_cin1_f32(img, NULL, res_a, res_t, res, ..., stride = img_stride, res_act) followed by
 * emd_sep3x3_fused_s2_f32(..., res, ...) -- the residual projection of the 1-channel input (residual0, machine_learning/denoiser.py:252)
 * is rank 1 and never exists in memory.  img_stride 1 or 2, ldimg <= 64; the image must be exactly H/2*img_stride rows of W/2*img_stride
 * pixels per batch entry (the kernel derives its row pitch from W; nothing else tells it).  Cout <= 128 with Cout/4 a divisor of 64
 * (emd_cin1_f32's rule); emd_sep3x3_fused_s2_genres_supported(H, W, Cin, Cout) says where it applies. */
int emd_sep3x3_fused_s2_genres_supported(int H, int W, int Cin, int Cout);
int emd_sep3x3_fused_s2_genres_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                   const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                   const float* img, int ldimg, int img_stride, const float* res_a, const float* res_t, int res_act,
                                   float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act, emd_stream_t stream);
/* The stride-1 block followed by a 3x3 SAME convolution to ONE channel (deconv0_b -> deconv_final, machine_learning/denoiser.py:383-387),
 * the convolution's channel sum folded into the block's epilogue.  With y the output emd_sep3x3_fused_f32 would have written (same
 * arithmetic, never stored), emd_sep3x3_fused_fold_f32 writes z [9][B][H][W]: z[t][b][h][w] = sum_c wfin[t][c] * y[b][h][w][c] in fp32
 * (fp32 matrix instruction, fixed order), wfin [3][3][Cout] as emd_conv3x3_cout1_f32 takes it.  emd_cout1_gather9_f32 finishes the convolution:
 * out[b][h][w] = act(scale * sum_t z[t][b][h + t/3 - 1][w + t%3 - 1] + shift), taps outside the image zero, added in the order t = 0..8;
 * scale / shift / act (0, 1, 2) as in emd_conv3x3_cout1_f32.  The pair computes emd_sep3x3_fused_f32 + emd_conv3x3_cout1_f32 up to the
 * order of the 576-term sum.  emd_sep3x3_fused_fold_supported: stride 1, split-bf16, H%8==0, W%16==0, Cin%32==0, Cout==64. */
int emd_sep3x3_fused_fold_supported(int H, int W, int Cin, int Cout);
int emd_sep3x3_fused_fold_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                              const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                              const float* res, int ldres, const float* wfin, float* z, int B, int H, int W, int Cin, int Cout,
                              int act, emd_stream_t stream);
int emd_cout1_gather9_f32(const float* z, float scale, float shift, float* y, int B, int H, int W, int act, emd_stream_t stream);
/* The same on the tf.pad(REFLECT, 1) image with VALID padding: graph G's down-sampling strided_conv_block(stride 2, pad_size = (1, 1))
 * (misc_py/gan-infilling-100.py:205-243, :345-352).  Same shape rules (emd_sep3x3_fused_supported(H, W, Cin, Cout, 2, 1)). */
int emd_sep3x3_fused_s2_reflect_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                    const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                    const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                                    emd_stream_t stream);

/* Depthwise 3x3, TF SAME padding, stride 1 or 2 (rate 1) or stride 1 with dilation `rate`.
 * replaces: the depthwise half of slim.separable_convolution2d (denoiser.py:113-131).
 * x [B,H,W,C] pixel stride ldx; w [3][3][C] (TF [3,3,C,1]); y [B,ceil(H/s),ceil(W/s),C] pixel stride ldy. */
int emd_dw3x3_f32(const float* x, int ldx, const float* w, float* y, int ldy, int B, int H, int W, int C,
                  int stride, int rate, emd_stream_t stream);

/* ---- "split32" activations: the pointwise GEMM fed entirely by LDS-DMA (csrc/gemm_split.hip).
 * A split32 tensor [npix][C] holds every value as bf16 hi + bf16 lo (x = hi + lo + O(2^-17 x), both round-to-nearest):
 * pixel pitch ld in 4-byte units (ld % 32 == 0, ld >= emd_split32_ld(C) = C rounded up to 32); inside a pixel, channel
 * group g = c/32 occupies bytes [128 g, 128 g + 128): 32 x hi, then 32 x lo; channels C..ld are zero.  Same bytes and
 * pitch as the fp32 NHWC tensor it stands for; base address 128-byte aligned.
 *
 * emd_dw3x3_split32_f32     = emd_dw3x3_f32 whose result is written in split32 form (the depthwise half of
 *                             slim.separable_convolution2d, machine_learning/denoiser.py:113-131).
 * emd_to_split32_f32        converts an fp32 tensor (pitch ldx floats).
 * emd_conv1x1_split32_f32   = emd_conv1x1_f32 (stride 1, EMD_PREC_BF16X3) on a split32 input: the pointwise half + BN x2
 *                             + relu6 + residual (:123, :134, :246); results are bit-identical to emd_conv1x1_f32 on the
 *                             fp32 twin of xs.  M = number of pixels.  256 x 128 tiles, 512 threads, K step 32, both
 *                             operands by global_load_lds_dwordx4, XOR-swizzled LDS rows.
 * emd_conv1x1_split32_supported: 1 where this kernel is the better choice (Cin, Cout >= 128 and >= 256 tiles). */
int emd_split32_ld(int C);
int emd_to_split32_f32(const float* x, int ldx, void* y, int ldy, long npix, int C, emd_stream_t stream);
int emd_dw3x3_split32_f32(const float* x, int ldx, const float* w, void* y, int ldy, int B, int H, int W, int C,
                          int stride, int rate, emd_stream_t stream);
int emd_dw3x3_reflect_split32_f32(const float* x, int ldx, const float* w, void* y, int ldy, int B, int H, int W, int C,
                                  int stride, emd_stream_t stream); /* emd_dw3x3_reflect_f32 (graph G) with split32 output */
/* emd_dw3x3_split32_f32 (stride 1, rate 1) over concat(emd_resize_bilinear_f32(lo [B,Hi,Wi,Cup] -> [H,W]), x [B,H,W,C-Cup]) along the
 * channels, without that tensor: the upsampled channels are formed in registers from lo (graph D's deconv2_a,
 * machine_learning/denoiser.py:350-356).  w [3][3][C], y split32 [B,H,W,C].  Bit-identical to the two launches over the concat.
 * Supported (emd_dw3x3_up_split32_supported; EMD_E_UNSUPPORTED otherwise): H >= Hi, W >= Wi, Cup a multiple of 64 and below C. */
int emd_dw3x3_up_split32_supported(int Hi, int Wi, int H, int W, int Cup, int C);
int emd_dw3x3_up_split32_f32(const float* lo, int ldlo, int Hi, int Wi, int Cup, const float* x, int ldx, const float* w, void* y,
                             int ldy, int B, int H, int W, int C, emd_stream_t stream);
int emd_conv1x1_split32_supported(long M, int Cin, int Cout);
/* emd_conv1x1_split32_f32 (no second affine, no residual) that also returns the per-channel batch mean and BIASED variance
 * of its output y -- what emd_bn_stats_f32 computes in a second pass over y (the batch-statistics norms that follow the
 * pointwise convs of misc_py/modified_Xception.py:302-323).  The GEMM epilogue leaves one double partial per (256-row tile,
 * channel); a fixed-order final reduction follows (deterministic).  workspace: emd_conv1x1_split32_stats_workspace_bytes(M,
 * Cout) bytes, 8-byte aligned. */
size_t emd_conv1x1_split32_stats_workspace_bytes(long M, int Cout);
int emd_conv1x1_split32_stats_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                  const float* shift1, float* y, int ldy, long M, int Cin, int Cout, int act, float* mean,
                                  float* var, void* workspace, emd_stream_t stream);
/* ... and folds the batch norm that uses those statistics in the same final-reduction launch (emd_bn_fold_f32's arithmetic on
 * the same float mean / var: scale = gamma / sqrt(var + eps), gamma NULL = 1; shift = beta - mean * scale, beta NULL = 0): one
 * launch instead of two between the GEMM and the kernel that applies the norm. */
int emd_conv1x1_split32_stats_fold_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                       const float* shift1, float* y, int ldy, long M, int Cin, int Cout, int act, float* mean,
                                       float* var, void* workspace, const float* gamma, const float* beta, float eps,
                                       float* scale, float* shift, emd_stream_t stream);
/* Dense 3x3 convolution (emd_conv3x3_f32: TF SAME, stride 1/2, dilation) and the 3x3 stride-2 transposed convolution
 * (emd_deconv3x3s2_f32) on a split32 input (csrc/conv_split.hip), same packed weights, same arithmetic (bit-identical results); out_split != 0
 * writes y itself as a split32 tensor (pitch ldy 4-byte units, % 32; channels Cout..ceil32(Cout) zero) for a following
 * split32 convolution -- tf.layers.conv2d / conv2d_transpose chains (misc_py/modified_Xception.py:215-229, :538-621;
 * machine_learning/denoiser.py:141-148) then never write an fp32 activation.  Cin <= 2048. */
int emd_conv3x3_split32_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                            const float* shift1, const float* scale2, const float* shift2, const float* res, int ldres,
                            void* y, int ldy, int B, int H, int W, int Cin, int Cout, int stride, int rate, int act,
                            int out_split, emd_stream_t stream);
int emd_deconv3x3s2_split32_f32(const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                const float* scale1, const float* shift1, void* y, int ldy, int B, int H, int W, int Cin,
                                int Cout, int act, int out_split, emd_stream_t stream);
int emd_conv1x1_split32_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                            const float* shift1, const float* scale2, const float* shift2, const float* res,
                            int ldres, float* y, int ldy, long M, int Cin, int Cout, int act, emd_stream_t stream);
/* emd_conv1x1_split32_f32 / emd_sep3x3_fused_f32 writing y as a split32 tensor (pitch ldy in 4-byte units, a multiple of 32;
 * y 128-byte aligned; channels Cout..ceil32(Cout) zero; the fused separable form needs Cout % 32 == 0): the producer of a
 * split32 convolution's input writes no fp32 activation and needs no emd_to_split32_f32 pass (graph D: deconv2_b -> deconv2to1,
 * deconv1_b -> deconv1to0, machine_learning/denoiser.py:357-362, :369-374).  Same values as the fp32 form, then split. */
int emd_conv1x1_split32_out_f32(const void* xs, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                const float* shift1, const float* scale2, const float* shift2, const float* res,
                                int ldres, void* y, int ldy, long M, int Cin, int Cout, int act, emd_stream_t stream);
int emd_sep3x3_fused_out_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                             const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                             const float* res, int ldres, void* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                             emd_stream_t stream);
/* 1 where a graph host should take emd_deconv3x3s2_fused_split32_f32 for this layer ([B,H,W,Cin] input): always where its
 * patch-resident kernel applies (H % 8 == 0, W % 32 == 0, Cin % 32 == 0 -- independent of B, because that kernel sums in another order
 * than the GEMM forms and a result must not depend on the batch size), otherwise from B*H*W >= 49152 on (speed only). */
int emd_deconv3x3s2_fused_preferred(int B, int H, int W, int Cin, int Cout);

/* emd_deconv3x3s2_split32_f32 as ONE launch: a workgroup computes the four output phases of its 256 input pixels back to
 * back, so the input is read from HBM once instead of once per phase launch.  Same arguments, bit-identical results. */
int emd_deconv3x3s2_fused_split32_f32(const void* xs, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4],
                                      const float* scale1, const float* shift1, void* y, int ldy, int B, int H, int W, int Cin,
                                      int Cout, int act, int out_split, emd_stream_t stream);

/* emd_dw3x3_f32 / emd_dw3x3_split32_f32 on relu(x * pre_scale + pre_shift) (per channel, device float[C]): the
 * batch-statistics norm + relu that ends the previous separable block of misc_py/modified_Xception.py (:302-323) applied
 * while the depthwise kernel loads its input, instead of in a pass of its own; padding is applied after it (TF pads the
 * activated tensor). */
int emd_dw3x3_pre_f32(const float* x, int ldx, const float* pre_scale, const float* pre_shift, const float* w, float* y,
                      int ldy, int B, int H, int W, int C, int stride, int rate, emd_stream_t stream);
int emd_dw3x3_pre_split32_f32(const float* x, int ldx, const float* pre_scale, const float* pre_shift, const float* w,
                              void* y, int ldy, int B, int H, int W, int C, int stride, int rate, emd_stream_t stream);
/* The same for the training step (round 4; graph D', slim.separable_convolution2d + _batch_norm_fn(is_training) + relu6,
 * machine_learning/denoiser.py:110-136 with phase = True; misc_py/denoiser-multi-gpu.py:752-782): the affine + activation of a
 * separable conv whose only consumer is the next one's depthwise stage is applied in that stage's loads.  act: EMD_ACT_RELU6 or
 * EMD_ACT_RELU; pre_images != 0: pre_scale / pre_shift are [B][C] (per-image statistics: a batched pass of one-image towers), else
 * [C].  Bits of emd_affine_act_f32 / emd_affine_act_images_f32 followed by emd_dw3x3_f32. */
int emd_dw3x3_pre_act_f32(const float* x, int ldx, const float* pre_scale, const float* pre_shift, int pre_images, int act,
                          const float* w, float* y, int ldy, int B, int H, int W, int C, int stride, int rate, emd_stream_t stream);

/* Dense 3x3 conv of a ONE-channel image + per-channel affine + activation (graph X's entry conv: tf.layers.conv2d(1 -> 32, k 3,
 * stride 2) + bias -> batch norm -> relu, misc_py/modified_Xception.py:356-364; the caller folds bias and norm into scale / shift):
 * x [B,H,W] fp32 contiguous, w [9][Cout] fp32 (tap-major), y [B,Ho,Wo,Cout] fp32 (pitch ldy floats) or, out_split != 0, a split32
 * tensor (pitch ldy 4-byte units, a multiple of 32; padding channels written as zero).  TF SAME, stride 1 or 2.  fp32 FMAs. */
int emd_conv3x3_cin1_f32(const float* x, const float* w, const float* scale, const float* shift, void* y, int ldy, int B, int H, int W,
                         int Cout, int stride, int act, int out_split, emd_stream_t stream);

/* Layers fed by the 1-channel image: y[pix][n] = act( d[pix]*a[n] + shift[n] ).
 * w9 != NULL: d = 3x3 SAME depthwise of x with the 9 weights w9 (stride 1)  -- cnn0 (denoiser.py:252),
 *             a[n] = pointwise_weights[0][n] * folded BN scale;
 * w9 == NULL: d = x sampled with `stride`                                   -- residual0 (:263),
 *             a[n] = weights[0][n] * folded BN scale, shift includes the bias.
 * x [B,H,W]; y [B,ceil(H/s),ceil(W/s),Cout] pixel stride ldy; Cout/4 must divide 64. */
int emd_cin1_f32(const float* x, const float* w9, const float* a, const float* shift, float* y, int ldy,
                 int B, int H, int W, int Cout, int stride, int act, emd_stream_t stream);

/* Dense 3x3 SAME convolution to ONE output channel + scalar affine + relu6.
 * replaces: the final slim.conv2d(num_outputs=1, kernel_size=3) + bias + BN + relu6 (denoiser.py:387).
 * x [B,H,W,Cin] pixel stride ldx; w [3][3][Cin]; y [B,H,W]; scale/shift: bias and BN folded.
 * act: 0 none, 1 relu6, 2 relu6 then tf.clip_by_value(.,0,1) (misc_py/denoiser-multi-gpu.py:534-538).
 * pre_relu != 0: the convolution is followed by "+pre_bias, relu" BEFORE the affine, i.e.
 *   tf.layers.conv2d(activation=relu) -> BN -> relu (conv_block, misc_py/modified_Xception.py:215-229, :621). */
int emd_conv3x3_cout1_f32(const float* x, int ldx, const float* w, float scale, float shift, float* y, int B,
                          int H, int W, int Cin, int act, float pre_bias, int pre_relu, emd_stream_t stream);

/* tf.image.resize_images(x,[Ho,Wo]): bilinear, align_corners=False, legacy (no half-pixel) sampling.
 * replaces: denoiser.py:199 (identity size) and :350 (32 -> 128). */
int emd_resize_bilinear_f32(const float* x, int ldx, float* y, int ldy, int B, int Hi, int Wi, int Ho, int Wo,
                            int C, emd_stream_t stream);

/* A lone inference batch norm (+ relu6): y = act(x*scale + shift) per channel.
 * replaces: batch_then_activ on the ASPP image-level branch (denoiser.py:200). */
int emd_affine_relu6_f32(const float* x, int ldx, const float* scale, const float* shift, float* y, int ldy,
                         long npix, int C, int act, emd_stream_t stream);

/* y = act(x*scale + shift) [+ res], act = EMD_ACT_*; y may be x (in place).  The normalise+activate step that
 * follows a batch-statistics batch norm, and the "+ residual" after it (misc_py/modified_Xception.py:397, :533). */
int emd_affine_act_f32(const float* x, int ldx, const float* scale, const float* shift, const float* res, int ldres,
                       float* y, int ldy, long npix, int C, int act, emd_stream_t stream);

/* Batch statistics for tf.contrib.layers.batch_norm called with its defaults (is_training=True) -- what the
 * separable convs of misc_py/modified_Xception.py:302-323 do even at inference: per-channel mean and BIASED
 * variance of x [npix, C] (pixel stride ldx), accumulated in double.  workspace: device buffer of
 * emd_bn_stats_workspace_bytes(npix, C) bytes, 8-byte aligned.  emd_bn_fold_f32 turns (mean, var, gamma|NULL,
 * beta|NULL, eps) into the (scale, shift) of one affine, on the device (no host round trip). */
/* Per-image forms (instance norms; the batch-statistics norms of misc_py/apply_autoencoders.py:105-116, which the reference
 * evaluates one crop per sess.run): x is [B][npix_img][C]; mean / var / scale / shift are [B][C]; workspace:
 * B x emd_bn_stats_workspace_bytes(npix_img, C) bytes.  Image b gets exactly the bits emd_bn_stats_f32 gives it alone. */
int emd_bn_stats_images_f32(const float* x, int ldx, int B, long npix_img, int C, float* mean, float* var, void* workspace,
                            emd_stream_t stream);

/* The convolutions of a TRAINING forward pass (misc_py/denoiser-multi-gpu.py:200-540 with phase = True, :752-782: every convolution is
 * followed by a batch norm on BATCH statistics): y = conv(x), no affine, no activation (ones / zeros: device vectors of Cout ones and
 * zeros, 16-byte aligned), plus the per-channel mean and biased variance of y, gathered in the GEMM's epilogue -- what
 * emd_bn_stats_f32 (images = 0: over all B * Ho * Wo pixels, mean / var [Cout]) or emd_bn_stats_images_f32 (images = 1: per image,
 * [B][Cout]) would return for y, without their pass over it (one partial per 128-row tile, reduced in a fixed order: deterministic;
 * the last bits differ from the two-launch form's, whose partials are cut differently).  images = 1 needs Ho * Wo % 128 == 0
 * (EMD_E_UNSUPPORTED otherwise: call the convolution and the statistics separately).
 * workspace: emd_conv_stats_workspace_bytes(B * Ho * Wo, Cout) bytes, 8-byte aligned.  emd_conv1x1_stats_f32: slim.conv2d 1x1 /
 * the pointwise half of slim.separable_convolution2d, stride 1 or 2 (TF SAME: samples x[0::2]); emd_conv3x3_stats_f32: dense 3x3,
 * stride 1, dilation `rate` (the ASPP branches of graph D', :330-353). */
size_t emd_conv_stats_workspace_bytes(long M, int Cout);
int emd_conv1x1_stats_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones, const float* zeros,
                          float* y, int ldy, int B, int H, int W, int Cin, int Cout, int stride, int precision, int images,
                          float* mean, float* var, void* workspace, emd_stream_t stream);
int emd_conv3x3_stats_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones, const float* zeros,
                          float* y, int ldy, int B, int H, int W, int Cin, int Cout, int rate, int precision, int images,
                          float* mean, float* var, void* workspace, emd_stream_t stream);
/* The transposed 3x3 stride-2 conv of a training forward pass (emd_deconv3x3s2_f32, no affine, no activation; machine_learning/
 * denoiser.py:141-148 under phase = True) + the batch statistics of its output from the four phase GEMMs' epilogues: mean / var [Cout]
 * over all B * 2H * 2W output pixels, or images != 0: [B][Cout] per image (needs H * W % 128 == 0: EMD_E_UNSUPPORTED otherwise).
 * workspace: emd_conv_stats_workspace_bytes(4 * B * H * W, Cout) bytes (the size allows for the ragged last tile of each of the four phases). */
int emd_deconv3x3s2_stats_f32(const float* x, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4], const float* ones,
                              const float* zeros, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int precision, int images,
                              float* mean, float* var, void* workspace, emd_stream_t stream);
/* The three above with the training-mode fold of the norm behind the conv in the statistics' final kernel (emd_bn_train_fold[_images]_f32's
 * step: scale, shift, rstd1, rstd2, moving-average updates; mean / var are written as well): one launch less per layer. */
int emd_conv1x1_stats_fold_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones, const float* zeros, float* y,
                               int ldy, int B, int H, int W, int Cin, int Cout, int stride, int precision, int images, float* mean, float* var,
                               void* workspace, const emd_bn_train_fold_t* fold, emd_stream_t stream);
int emd_conv3x3_stats_fold_f32(const float* x, int ldx, const uint16_t* whi, const uint16_t* wlo, const float* ones, const float* zeros, float* y,
                               int ldy, int B, int H, int W, int Cin, int Cout, int rate, int precision, int images, float* mean, float* var,
                               void* workspace, const emd_bn_train_fold_t* fold, emd_stream_t stream);
int emd_deconv3x3s2_stats_fold_f32(const float* x, int ldx, const uint16_t* const whi[4], const uint16_t* const wlo[4], const float* ones,
                                   const float* zeros, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int precision, int images,
                                   float* mean, float* var, void* workspace, const emd_bn_train_fold_t* fold, emd_stream_t stream);
int emd_affine_act_images_f32(const float* x, int ldx, const float* scale, const float* shift, const float* res, int ldres,
                              float* y, int ldy, int B, long npix_img, int C, int act, emd_stream_t stream);
/* y = act(x*scale + shift) + res_act(res*res_scale + res_shift): the residual operand given BEFORE its own affine + activation (round 4,
 * graph D': the 1x1 residual projection's batch norm + relu6 -- conv_block_not_sep, machine_learning/denoiser.py:356-383 with phase =
 * True -- applied where the block adds it instead of in a pass of its own; bits of the two-pass route).  images = 0: vectors [C], npix =
 * all pixels; images = B > 0: vectors [B][C], npix = pixels per image.  res_act: EMD_ACT_RELU6 or EMD_ACT_RELU. */
int emd_affine_act_res_affine_f32(const float* x, int ldx, const float* scale, const float* shift, const float* res, int ldres,
                                  const float* res_scale, const float* res_shift, int res_act, float* y, int ldy, int images, long npix,
                                  int C, int act, emd_stream_t stream);
size_t emd_bn_stats_workspace_bytes(long npix, int C);
int emd_bn_stats_f32(const float* x, int ldx, long npix, int C, float* mean, float* var, void* workspace,
                     emd_stream_t stream);
int emd_bn_fold_f32(const float* mean, const float* var, const float* gamma, const float* beta, float eps,
                    float* scale, float* shift, int C, emd_stream_t stream);

/* ================================================================================================
 * Training path of graph D' (misc_py/denoiser-multi-gpu.py): tf.gradients of the tower loss (:752-782) and the
 * Nesterov train op (:1011-1077).  Data gradients of the 1x1 / 3x3 / transposed convolutions are the forward
 * entry points above run with weights packed transposed (emd_pack_weights_dev); the rest follows.
 * Convention: PARAMETER gradients are ADDED into their destination (towers / micro-batches accumulate one
 * gradient set, :1040; zero it once per step), activation gradients are written.
 * ================================================================================================ */

/* Weight gradient of any convolution above: dw[t][k][n] += sum_m a[src_t(m)][k] * dy[m][n].
 * replaces: the Conv2DBackpropFilter nodes tf.gradients (:779) creates for tf.layers.conv2d / the pointwise half of
 * slim.separable_convolution2d (:225-276) / tf.layers.conv2d_transpose (:278-289).
 * m runs over the [B,Hg,Wg] grid of dy (pixel stride ldd, N channels); a is [B,Ha,Wa,K] (pixel stride lda) read at
 * (i*sa + tap_dy[t], j*sa + tap_dx[t]), zero outside.  conv (stride s, rate r, SAME pad pt): a = layer input,
 * sa = s, tap = k*r - pt, dw in TF layout [taps][Cin][Cout].  Transposed conv: a = the gradient w.r.t. its OUTPUT,
 * dy := its INPUT, sa = 2, tap = k, dw in TF layout [taps][Cout][Cin].  K, N multiples of 4. */
int emd_conv_wgrad_f32(const float* a, int lda, const float* dy, int ldd, float* dw, int B, int Hg, int Wg, int Ha, int Wa,
                       int K, int N, int ntaps, const int* tap_dy, const int* tap_dx, int sa, emd_stream_t stream);

/* emd_pack_weights_bf16 for weights that live on the DEVICE (re-packed after every optimizer step).
 * w [src_taps][Cin][Cout] (cout_major 0) or [src_taps][Cout][Cin] (cout_major 1); packed tap t is source tap
 * tap_sel[t] (NULL: identity, needs ntaps == src_taps) -- reversed order for the data gradient of a 3x3 conv,
 * emd_deconv_phase_taps subsets for the transposed conv.  hi/lo: emd_packed_weight_elems(ntaps,Cin,Cout) elements. */
int emd_pack_weights_dev(const float* w, int src_taps, int ntaps, const int* tap_sel, int Cin, int Cout, int cout_major,
                         uint16_t* hi, uint16_t* lo, emd_stream_t stream);

/* All of a model's packs in ONE launch (the re-pack after an optimizer step is ~860 packs of a few KB..MB each: launch-bound one
 * by one).  A job = one emd_pack_weights_dev call; emd_pack_job_fill validates the arguments on the host and fills the derived
 * fields; the caller numbers the jobs' blocks consecutively (first_block = sum of the earlier jobs' n_blocks), copies the table
 * to the device once (the pointers in it do not change between steps) and passes the total block count. */
typedef struct emd_pack_job {
    const float* w;
    uint16_t* hi;
    uint16_t* lo;
    unsigned long long tap_sel;   /* 4 bits per packed tap: its source tap */
    long total;                   /* packed elements of one plane */
    long first_block;             /* caller-assigned */
    long n_blocks;                /* workgroups of this job in the batch launch (set by emd_pack_job_fill: ceil(total / 256), or the 16 x 16
                                   * tile count of the transposing form) */
    int ntaps, cin, cout, cout_major, cpad, pad_;
} emd_pack_job_t;
int emd_pack_job_fill(emd_pack_job_t* job, const float* w, int src_taps, int ntaps, const int* tap_sel, int Cin, int Cout,
                      int cout_major, uint16_t* hi, uint16_t* lo);
int emd_pack_weights_batch_dev(const emd_pack_job_t* jobs_dev, int n_jobs, long n_blocks, emd_stream_t stream);

/* Data gradient of the stride-2 1x1 conv (residual branches, :225-238 with strides=2):
 * dx[b,2i,2j,:] = dy[b,i,j,:] * W^T (+ res at the same pixels); other pixels of dx are left as they are.
 * dy [B,ceil(H/2),ceil(W/2),Cout]; dx [B,H,W,Cin]; whi/wlo packed with (Cin:=Cout, Cout:=Cin, cout_major 1). */
int emd_conv1x1_s2_bwd_data_f32(const float* dy, int ldd, const uint16_t* whi, const uint16_t* wlo, const float* scale1,
                                const float* shift1, const float* res, int ldres, float* dx, int ldx, int B, int H, int W,
                                int Cout, int Cin, int precision, emd_stream_t stream);

/* Training-mode batch norm chain  r -> [BN1] -> BN2 -> relu6 [-> clip]  (:210-223; contrib batch_norm, fused,
 * decay 0.999, eps 1e-3), see csrc/bn_train.hip for the algebra.
 * emd_bn_train_fold_f32: batch (mean,var) of r (emd_bn_stats_f32) -> forward affine (scale, shift), rstd1 (and
 *   rstd2 for the double norm: gamma1/beta1 non-NULL), and, if mm2 != NULL, the moving-average updates
 *   (mm1/mv1: BN1's, double norm only; bias: the conv bias that precedes a single BN, may be NULL).
 * emd_bn_bwd_reduce_f32: s1[c] = sum g, s2[c] = sum g*(x-mean)*rstd, g = dy*mask(x*mscale+mshift);
 *   mask 0 none, 1 relu6 (0<z<6), 2 relu6 then clip [0,1] (0<z<=1), 3 leaky_relu 0.2 (graph G), 4 relu (z>0, graph S).
 *   x == NULL: s1 only.
 *   accumulate_s1 != 0: s1 += (bias gradients).  workspace: emd_chan_reduce_workspace_bytes(npix, C) bytes.
 * emd_bn_bwd_prep_f32: (s1, t=s2) -> K, m1, m2 for the apply step; dgamma1, dgamma2, dbeta2 += .
 * emd_bn_bwd_apply_f32: dx = K*(g - m1 - (x-mean)*m2); dx may be dy.  C = 1 is allowed (the final layer). */
int emd_bn_bwd_reduce_prep_f32(const float* dy, int ldd, const float* x, int ldx, const float* mean, const float* rstd, const float* mscale,
                               const float* mshift, int mask, int images, long npix, int C, float* s1, float* s2, void* workspace,
                               const emd_bn_bwd_prep_t* prep, emd_stream_t stream);
/* The reduction (+ per-channel step) and the apply pass for a gradient that is the data gradient of a 3x3 conv to ONE output channel (the
 * network's final conv, :528-532): dy[p][c] = sum_taps g1[p + (1-ky, 1-kx)] * w9[3ky+kx][c] is formed from the 1-channel image g1 [B][H][W]
 * in both passes and never written (emd_conv3x3_cout1_bwd_data_f32's arithmetic).  images != 0: per-image vectors [B][C]. */
int emd_bn_bwd_reduce_prep_cout1_f32(const float* g1, const float* w9, int B, int H, int W, const float* x, int ldx, const float* mean,
                                     const float* rstd, const float* mscale, const float* mshift, int mask, int images, int C, float* s1,
                                     float* s2, void* workspace, const emd_bn_bwd_prep_t* prep, emd_stream_t stream);
int emd_bn_bwd_apply_cout1_f32(const float* g1, const float* w9, int B, int H, int W, const float* x, int ldx, const float* K, const float* m1,
                               const float* mean, const float* m2, const float* mscale, const float* mshift, int mask, int images, float* dx,
                               int ldo, int C, emd_stream_t stream);
size_t emd_chan_reduce_workspace_bytes(long npix, int C);
int emd_bn_train_fold_f32(const float* mean, const float* var, const float* gamma1, const float* beta1, const float* gamma2,
                          const float* beta2, const float* bias, float eps, long npix, int C, float* scale, float* shift,
                          float* rstd1, float* rstd2, float* mm1, float* mv1, float* mm2, float* mv2, double decay,
                          emd_stream_t stream);
int emd_bn_bwd_reduce_f32(const float* dy, int ldd, const float* x, int ldx, const float* mean, const float* rstd,
                          const float* mscale, const float* mshift, int mask, long npix, int C, float* s1, float* s2,
                          int accumulate_s1, void* workspace, emd_stream_t stream);
int emd_bn_bwd_prep_f32(const float* s1, const float* t, const float* gamma1, const float* gamma2, const float* rstd1,
                        const float* rstd2, float eps, long npix, int C, float* K, float* m1, float* m2, float* dgamma1,
                        float* dgamma2, float* dbeta2, emd_stream_t stream);
int emd_bn_bwd_apply_f32(const float* dy, int ldd, const float* x, int ldx, const float* K, const float* m1,
                         const float* mean, const float* m2, const float* mscale, const float* mshift, int mask, float* dx,
                         int ldo, long npix, int C, emd_stream_t stream);
/* Per-image forms of the four (B images of npix pixels each; statistics / coefficient vectors [B][C]; the parameter
 * vectors gamma / beta / bias and their gradients stay [C]; the moving statistics follow image 0, the first tower,
 * misc_py/denoiser-multi-gpu.py:701-707).  Image b is reduced exactly as it would be alone, so the one-image towers of a
 * rank (:763) run as ONE batched pass with per-image statistics from emd_bn_stats_images_f32 / emd_affine_act_images_f32:
 * identical arithmetic per image, B times the GEMM M, B times fewer launches.  Workspace of the reduce: B x
 * emd_chan_reduce_workspace_bytes(npix, C). */
int emd_bn_train_fold_images_f32(const float* mean, const float* var, const float* gamma1, const float* beta1,
                                 const float* gamma2, const float* beta2, const float* bias, float eps, long npix, int B, int C,
                                 float* scale, float* shift, float* rstd1, float* rstd2, float* mm1, float* mv1, float* mm2,
                                 float* mv2, double decay, emd_stream_t stream);
int emd_bn_bwd_reduce_images_f32(const float* dy, int ldd, const float* x, int ldx, const float* mean, const float* rstd,
                                 const float* mscale, const float* mshift, int mask, int B, long npix, int C, float* s1,
                                 float* s2, void* workspace, emd_stream_t stream);
int emd_bn_bwd_prep_images_f32(const float* s1, const float* t, const float* gamma1, const float* gamma2, const float* rstd1,
                               const float* rstd2, float eps, long npix, int B, int C, float* K, float* m1, float* m2,
                               float* dgamma1, float* dgamma2, float* dbeta2, emd_stream_t stream);
int emd_bn_bwd_apply_images_f32(const float* dy, int ldd, const float* x, int ldx, const float* K, const float* m1,
                                const float* mean, const float* m2, const float* mscale, const float* mshift, int mask,
                                float* dx, int ldo, int B, long npix, int C, emd_stream_t stream);

/* The training-mode batch norm of a SMALL map as ONE launch per direction (round 4): per-image statistics (a tower of one image,
 * misc_py/denoiser-multi-gpu.py:763, or B of them as one batched pass; vectors [B][C]), npix <= 4096 pixels per image, C % 4 == 0
 * (emd_bn_train_small_supported; EMD_E_UNSUPPORTED otherwise: use the slab forms above).
 * emd_bn_train_fwd_small_f32 == emd_bn_stats_images_f32 + emd_bn_train_fold_images_f32 + emd_affine_act_images_f32:
 *   out = act(r * scale + shift) [+ res], with scale / shift / rstd1 / rstd2 / mean returned for the reverse pass and the moving
 *   statistics (NULL = leave them) updated from image 0.  gamma1 / beta1 NULL: a single norm (gamma2, beta2) behind conv + bias.
 * emd_bn_train_bwd_small_f32 == emd_bn_bwd_reduce_images_f32 + emd_bn_bwd_prep_images_f32 + emd_bn_bwd_apply_images_f32:
 *   dx = d loss / d r (dx may be dy or x), the norms' parameter gradients ADDED (float atomics) into dgamma1 / dgamma2 / dbeta2.
 * Same formulas as the slab forms; their sums are cut differently, so the two agree to rounding, not bit for bit. */
int emd_bn_train_small_supported(long npix, int C);
int emd_bn_train_fwd_small_f32(const float* r, int ldr, int B, long npix, int C, const float* gamma1, const float* beta1,
                               const float* gamma2, const float* beta2, const float* bias, float eps, float* scale, float* shift,
                               float* rstd1, float* rstd2, float* mean, float* mm1, float* mv1, float* mm2, float* mv2, double decay,
                               const float* res, int ldres, float* out, int ldo, int act, emd_stream_t stream);
int emd_bn_train_bwd_small_f32(const float* dy, int ldd, const float* x, int ldx, int B, long npix, int C, const float* mean,
                               const float* rstd1, const float* rstd2, const float* mscale, const float* mshift, int mask,
                               const float* gamma1, const float* gamma2, float eps, float* dgamma1, float* dgamma2, float* dbeta2,
                               float* dx, int ldo, emd_stream_t stream);

/* Depthwise 3x3 backward (the depthwise half of slim.separable_convolution2d, :253-273); shapes as emd_dw3x3_f32
 * (x, dx [B,H,W,C]; dy [B,ceil(H/s),ceil(W/s),C]); dw [3][3][C] +=. */
int emd_dw3x3_wgrad_f32(const float* x, int ldx, const float* dy, int ldd, float* dw, int B, int H, int W, int C, int stride,
                        int rate, emd_stream_t stream);
int emd_dw3x3_bwd_data_f32(const float* dy, int ldd, const float* w, float* dx, int ldx, int B, int H, int W, int C,
                           int stride, int rate, emd_stream_t stream);
/* Round 4: the data gradient of a stride-1 depthwise 3x3 fused with the batch-norm backward of the layer BEFORE it, for a gradient that
 * has no other contribution (the output of a separable conv consumed by exactly one separable conv): dy = emd_dw3x3_f32(dd, w_flipped)
 * is formed on the fly in both passes and never written.
 *   emd_dw3x3_bn_bwd_reduce_f32 = emd_dw3x3_f32 + emd_bn_bwd_reduce[_images]_f32 (s1 = sum g, s2 = sum g * (r - mean) * rstd,
 *                                 g = dy * mask(r * mscale + mshift)); workspace: emd_dw3x3_bn_bwd_workspace_bytes(B, H, W, C)
 *   emd_dw3x3_bn_bwd_apply_f32  = emd_dw3x3_f32 + emd_bn_bwd_apply[_images]_f32 (dr = K * (g - m1 - (r - mean) * m2); dr may be r)
 * dw_consumer (or NULL; needs mask = relu6): [9][C] += the CONSUMER's depthwise weight gradient = emd_dw3x3_wgrad_pre_f32(r, mscale,
 * mshift, relu6, dd): the reduction pass streams exactly its operands.
 * r, dr [B,H,W,C] (the consumer's INPUT grid); dd [B,ceil(H/stride),ceil(W/stride),C]; stride 1 or 2, rate (dilation, stride 1 only) as
 * emd_dw3x3_f32 (stride 1, rate 1: the rolling-window form; else a gather form = emd_dw3x3_bwd_data_f32's arithmetic);
 * w_flipped [9][C] = the consumer's depthwise taps reversed (tap t = original tap 8 - t); images != 0: every
 * per-channel vector is [B][C] (per-image statistics).  (tf.gradients of machine_learning/denoiser.py:110-136 with phase = True.) */
size_t emd_dw3x3_bn_bwd_workspace_bytes(int B, int H, int W, int C);
int emd_dw3x3_bn_bwd_reduce_f32(const float* dd, int ldd, const float* w_flipped, const float* r, int ldr, const float* mean,
                                const float* rstd, const float* mscale, const float* mshift, int mask, int images, int B, int H, int W,
                                int C, int stride, int rate, float* s1, float* s2, float* dw_consumer, void* workspace,
                                const emd_bn_bwd_prep_t* prep /* or NULL */, emd_stream_t stream);
int emd_dw3x3_bn_bwd_apply_f32(const float* dd, int ldd, const float* w_flipped, const float* r, int ldr, const float* K, const float* m1,
                               const float* mean, const float* m2, const float* mscale, const float* mshift, int mask, int images,
                               float* dr, int ldo, int B, int H, int W, int C, int stride, int rate, emd_stream_t stream);
/* Both gradients of a stride-1 depthwise 3x3 in one pass (round 4): dx = emd_dw3x3_f32(dd, w_flipped) -- the data gradient, its bits -- and
 * dw[9][C] += emd_dw3x3_wgrad_f32(x, dd); dd is read once instead of twice.  x, dx, dd [B,H,W,C]; w_flipped = the taps reversed. */
int emd_dw3x3_bwd_both_f32(const float* dd, int ldd, const float* w_flipped, const float* x, int ldx, float* dx, int ldo, float* dw, int B,
                           int H, int W, int C, emd_stream_t stream);
/* emd_dw3x3_wgrad_f32 with the layer's input given as the pre-activation tensor r of the layer before it (the forward pass ran
 * emd_dw3x3_pre_act_f32 on it and never wrote x = act(r * pre_scale + pre_shift)): x is rebuilt in the loads.  Arguments as there. */
int emd_dw3x3_wgrad_pre_f32(const float* r, int ldx, const float* pre_scale, const float* pre_shift, int pre_images, int act,
                            const float* dy, int ldd, float* dw, int B, int H, int W, int C, int stride, int rate, emd_stream_t stream);

/* Backward of the final 3x3 conv to one channel (:528-532): dy [B,H,W]; dw [3][3][Cin] +=; dx [B,H,W,Cin]. */
int emd_conv3x3_cout1_wgrad_f32(const float* x, int ldx, const float* dy, float* dw, int B, int H, int W, int Cin,
                                emd_stream_t stream);
int emd_conv3x3_cout1_bwd_data_f32(const float* dy, const float* w, float* dx, int ldx, int B, int H, int W, int Cin,
                                   emd_stream_t stream);

/* Gradients of emd_resize_bilinear_f32 (dx [B,Hi,Wi,C] from dy [B,Ho,Wo,C]) and emd_avgpool2x2_f32. */
int emd_resize_bilinear_bwd_f32(const float* dy, int ldd, float* dx, int ldx, int B, int Hi, int Wi, int Ho, int Wo, int C,
                                emd_stream_t stream);
int emd_avgpool2x2_bwd_f32(const float* dy, int ldd, float* dx, int ldx, int B, int H, int W, int C, emd_stream_t stream);

/* y += alpha*x over [npix, C] (gradient fan-in where a tensor feeds several layers). */
int emd_axpy_f32(const float* x, int ldx, float* y, int ldy, long npix, int C, float alpha, emd_stream_t stream);

/* _tower_fn's loss (:768-775): mse = mean((out-truth)^2); loss = 1000*mse if mse < 1e-3 else sqrt(1000*mse)
 * (weight_decay = 0, :117).  result3 (device) = {mse, loss, f}; dout (may be NULL) = grad_scale * dloss/dout.
 * workspace: emd_denoise_loss_workspace_bytes() bytes.  No host synchronisation. */
size_t emd_denoise_loss_workspace_bytes(void);
int emd_denoise_loss_f32(const float* out, const float* truth, long n, float grad_scale, float* result3, float* dout,
                         void* workspace, emd_stream_t stream);

/* tf.train.MomentumOptimizer(lr, momentum, use_nesterov=True) (:1064-1066) on a flat parameter vector:
 * g = grad*grad_scale (1/number of gradient sets, :1040); accum = momentum*accum + g; param -= lr*(g + momentum*accum). */
int emd_nesterov_step_f32(float* param, const float* grad, float* accum, long n, float lr, float momentum, float grad_scale,
                          emd_stream_t stream);

/* ================================================================================================
 * Graph G: the in-filling GAN's generator (misc_py/gan-infilling-100.py:133-374), inference.  Its pointwise halves,
 * SAME-padded separable convs and resizes are the graph-D entry points with act = EMD_ACT_LEAKY; what follows is what
 * only G has.
 * ================================================================================================ */

/* Depthwise 3x3 over the tf.pad(REFLECT, 1) input, VALID, stride 1 or 2 -- the depthwise half of
 * strided_conv_block(pad_size=(1,1)) (:205-243): output (oy,ox) reads input rows oy*s-1..oy*s+1, index -1 -> 1,
 * H -> H-2.  x [B,H,W,C]; y [B,(H-1)/s+1,(W-1)/s+1,C]; w [3][3][C]. */
int emd_dw3x3_reflect_f32(const float* x, int ldx, const float* w, float* y, int ldy, int B, int H, int W, int C, int stride,
                          emd_stream_t stream);

/* The first layer (:343-347): 7x7 separable conv on the 1-channel image, reflect-padded by 3, VALID:
 * y[pix][n] = act(d[pix]*a[n] + shift[n]), d = 7x7 depthwise (w49), a = pointwise weight * folded BN scale;
 * act != 0: leaky_relu(0.2).  x [B,H,W]; y [B,H,W,Cout] pixel stride ldy; Cout/4 must divide 64. */
int emd_cin1_k7_reflect_f32(const float* x, const float* w49, const float* a, const float* shift, float* y, int ldy, int B,
                            int H, int W, int Cout, int act, emd_stream_t stream);

/* The last conv (:362-369): tf.pad(REFLECT,1) + slim.conv2d(1, 3, VALID) + bias, no activation.
 * x [B,H,W,Cin]; w [3][3][Cin]; y [B,H,W]. */
int emd_conv3x3_cout1_reflect_f32(const float* x, int ldx, const float* w, float bias, float* y, int B, int H, int W, int Cin,
                                  emd_stream_t stream);

/* _instance_norm with its fixed unit affine (:140-148) + tf.tanh (:372) on a 1-channel batch:
 * y = tanh((x - mean[b]) * rsqrt(var[b] + eps)); mean/var per image (emd_bn_stats_f32 with C = 1 on each image). */
int emd_instnorm_tanh_f32(const float* x, const float* mean, const float* var, float* y, int B, long npix_img, float eps,
                          emd_stream_t stream);

/* The decoder pair "separable conv + 1x1 residual projection of the SAME input" in one launch
 * (machine_learning/denoiser.py:356-359, :368-371, :380-383: deconv*_a = strided_conv_block(concat) and
 * residual*_d = conv_block_not_sep(concat, kernel_size=1)):
 *   y  = act(pointwise(depthwise3x3(x)) * scale1 + shift1)     as emd_sep3x3_fused_f32 (stride 1, TF SAME)
 *   y2 = relu6((x . W2) * scale_b + shift_b)                    W2 packed as for emd_conv1x1_f32; bias and BN folded into scale_b / shift_b
 * The 384- / 128-channel input -- the largest tensors of the decoder -- is read from HBM once instead of twice.
 * Split-bf16 precision.  Supported (emd_sep3x3_dual_supported): W%16==0, Cin%32==0, both Cout%4==0 and <= 128,
 * H%8==0 (H%4==0 when either output has more than 64 channels).  emd_sep3x3_dual_preferred: 1 where the one-launch form is also the
 * faster route (always up to 64 | 64 channels; wider only for H%8==0, W%32==0) -- what a graph executor should ask. */
int emd_sep3x3_dual_supported(int H, int W, int Cin, int Cout, int Cout2);
int emd_sep3x3_dual_preferred(int H, int W, int Cin, int Cout, int Cout2);
int emd_sep3x3_dual_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                        const float* scale1, const float* shift1, float* y, int ldy, const uint16_t* w2hi,
                        const uint16_t* w2lo, const float* scale_b, const float* shift_b, float* y2, int ldy2, int B, int H,
                        int W, int Cin, int Cout, int Cout2, int act, emd_stream_t stream);

/* The separable conv of the 728-channel flow as ONE kernel (csrc/sep_gemm.hip): the depthwise 3x3 stage (stride 1, TF SAME) is
 * computed per 32-channel K step inside the pointwise GEMM -- no depthwise launch, no intermediate tensor, 128-pixel x
 * 384-channel workgroup tiles (machine_learning/denoiser.py:110-136 as used by :297-302, :312-325).  Arguments as
 * emd_sep3x3_fused_f32 (split-bf16 precision only).  Supported (emd_sep3x3_gemm_supported): H%4==0, W%32==0,
 * 256 <= Cin <= 4096, 384 < Cout <= 768, Cin%4==0, Cout%4==0. */
int emd_sep3x3_gemm_supported(int H, int W, int Cin, int Cout);
int emd_sep3x3_gemm_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                        const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                        const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout, int act,
                        emd_stream_t stream);

/* emd_sep3x3_fused_f32 with the depthwise stage reading the tf.pad(REFLECT, 1) border instead of zeros: the
 * stride-1 strided_conv_block(pad_size=(1,1)) of graph G (:205-243).  Same arguments and support rule. */
int emd_sep3x3_fused_reflect_f32(const float* x, int ldx, const float* dw, const uint16_t* whi, const uint16_t* wlo,
                                 const float* scale1, const float* shift1, const float* scale2, const float* shift2,
                                 const float* res, int ldres, float* y, int ldy, int B, int H, int W, int Cin, int Cout,
                                 int act, int precision, emd_stream_t stream);

/* emd_dw3x3_reflect_f32 on a GENERATED input: the C-channel tensor the depthwise conv reads is act(d[pixel] * gen_a[c] + gen_t[c]),
 * d one value per pixel with pitch ldd floats (channel 0 of a 4-channel emd_cin1_k7_reflect_f32 output with a = (1,0,0,0), no
 * activation); leaky_act != 0: tf.nn.leaky_relu(alpha 0.2).  The generator's first layer feeding its second
 * (misc_py/gan-infilling-100.py:343-349) without the [B,H,W,C] tensor in memory; bit-identical to the two calls it replaces. */
int emd_dw3x3_reflect_gen_f32(const float* d, int ldd, const float* gen_a, const float* gen_t, int leaky_act, const float* w,
                              float* y, int ldy, int B, int H, int W, int C, int stride, emd_stream_t stream);

/* emd_sep3x3_fused_f32 on a GENERATED input: the Cin-channel tensor the depthwise stage reads is
 * act_gen(d[pixel] * gen_a[c] + gen_t[c]) with d a one-value-per-pixel tensor of pitch ldd floats (e.g. channel 0 of a
 * 4-channel emd_cin1_f32 output with a = (1,0,0,0), no activation).  It is the layer after the one fed by the 1-channel
 * micrograph (cnn0 -> cnn0_last, machine_learning/denoiser.py:252-255): cnn0 = relu6(BN(depthwise(img) (x) pointwise)) is
 * rebuilt in registers and never written to memory.  gen_act is an EMD_ACT_* code (0 none, 1 relu6, 2 relu, 4 leaky 0.2);
 * reflect as in emd_sep3x3_fused_reflect_f32.  Bit-identical to emd_cin1_f32 followed by emd_sep3x3_fused_f32. */
int emd_sep3x3_fused_gen_f32(const float* d, int ldd, const float* gen_a, const float* gen_t, int gen_act, const float* dw,
                             const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1,
                             const float* scale2, const float* shift2, const float* res, int ldres, float* y, int ldy, int B,
                             int H, int W, int Cin, int Cout, int act, int precision, int reflect, emd_stream_t stream);

/* The same layer with d formed inside the kernel too: img is the contiguous 1-channel image [B,H,W] and w9 the nine taps of its 3x3
 * depthwise conv (TF SAME), d = what emd_cin1_f32(img, w9, (1,0,0,0), 0, ..., act = 0) writes into channel 0.  The generated input is
 * built in registers from a (8+2) x (16+2) tile of d in LDS; neither d nor the Cin-channel tensor exists in memory.  Covers
 * gen_act == EMD_ACT_RELU6, zero padding (reflect == 0), precision == EMD_PREC_BF16X3 and the shapes
 * emd_sep3x3_fused_gen9_supported(H, W, Cin, Cout) accepts (H % 8 == 0, W % 16 == 0, Cin 32 or 64, Cout % 4 == 0, Cout <= 64);
 * anything else is EMD_E_UNSUPPORTED (use emd_cin1_f32 + emd_sep3x3_fused_gen_f32).  Bit-identical to that pair. */
int emd_sep3x3_fused_gen9_supported(int H, int W, int Cin, int Cout);
int emd_sep3x3_fused_gen9_f32(const float* img, const float* w9, const float* gen_a, const float* gen_t, int gen_act, const float* dw,
                              const uint16_t* whi, const uint16_t* wlo, const float* scale1, const float* shift1,
                              const float* scale2, const float* shift2, const float* res, int ldres, float* y, int ldy, int B,
                              int H, int W, int Cin, int Cout, int act, int precision, int reflect, emd_stream_t stream);

/* Discriminator head (misc_py/gan-infilling-100.py:560-567, :708): a fully connected layer to ONE output per row,
 * y[b] = x[b,:K].w + bias (x row stride ldx), and output = sigmoid(max(small, medium, large)). */
int emd_fc_rows_f32(const float* x, int ldx, const float* w, float bias, float* y, int B, int K, emd_stream_t stream);
int emd_max3_sigmoid_f32(const float* a, const float* b, const float* c, float* y, int n, emd_stream_t stream);

/* ================================================================================================
 * Training side of graph G (misc_py/gan-infilling-100.py:982-1088 towers, :1378-1379 / :1429-1431 optimizers).  The
 * convolution gradients are the graph-D' entry points with mask 3 (leaky_relu) in emd_bn_bwd_{reduce,apply}_f32.
 * ================================================================================================ */

/* Head of one tower (batch_size 1, :74): out = sigmoid(max(logit3)); mode 0: discriminator loss
 * -log(clip(1-|label-out|, 1e-8, 1-1e-8)) (:1080); mode 1: generator loss -log(clip(out, 1e-8, 1)) (:1037).
 * result2 = {out, loss}; dlogit3 = grad_scale * dloss/dlogit (arg-max branch only).  All device pointers. */
int emd_gan_head_f32(const float* logit3, float label, int mode, float grad_scale, float* result2, float* dlogit3,
                     emd_stream_t stream);
/* Backward of emd_fc_rows_f32 for one row: dw[k] += x[k]*g, *db += g, dx[k] = w[k]*g with g = *dlogit (device). */
int emd_fc_row_bwd_f32(const float* x, const float* w, const float* dlogit, float* dw, float* db, float* dx, int K,
                       emd_stream_t stream);
/* Gradient of tf.reduce_mean(x, [1,2]) (:578): y[p][c] = v[c]*alpha for every pixel p of [npix, C]. */
int emd_bcast_rows_f32(const float* v, float* y, int ldy, long npix, int C, float alpha, emd_stream_t stream);
/* out[0] = |scale*x|^2 of a flat vector (double accumulation): the global norm of clip_gradients_by_norm.
 * workspace: emd_sumsq_workspace_bytes() bytes. */
size_t emd_sumsq_workspace_bytes(void);
int emd_sumsq_f32(const float* x, long n, float scale, float* out, void* workspace, emd_stream_t stream);
/* tf.train.AdamOptimizer(lr, beta1 = 0.5) inside tf.contrib.estimator.clip_gradients_by_norm(., clip_norm):
 * g = grad*grad_scale*clip_norm/max(sqrt(*gnorm_sq), clip_norm) (gnorm_sq NULL: no clipping); m, v moment updates;
 * param -= lr_t*m/(sqrt(v)+eps), lr_t = lr*sqrt(1-beta2^t)/(1-beta1^t) computed by the caller. */
int emd_adam_step_f32(float* param, const float* grad, float* m, float* v, long n, float lr_t, float beta1, float beta2,
                      float eps, float grad_scale, const float* gnorm_sq, float clip_norm, emd_stream_t stream);
/* The same with lr_t (which changes every step through the bias correction) read from DEVICE memory, so that the
 * optimizer step can live inside a replayed hipGraph. */
int emd_adam_step_dev_f32(float* param, const float* grad, float* m, float* v, long n, const float* lr_t_dev, float beta1,
                          float beta2, float eps, float grad_scale, const float* gnorm_sq, float clip_norm,
                          emd_stream_t stream);

/* Generator-side training (the generator tower, :982-1046; its batch norms stay on MOVING statistics while the tower
 * gradients are evaluated, :1667).
 * Reflect-padded depthwise 3x3 backward (shapes as emd_dw3x3_reflect_f32; dw += ; dx written) and the same for the last
 * 3x3 conv to one channel (dy [B,H,W]). */
int emd_dw3x3_reflect_wgrad_f32(const float* x, int ldx, const float* dy, int ldd, float* dw, int B, int H, int W, int C,
                                int stride, emd_stream_t stream);
int emd_dw3x3_reflect_bwd_data_f32(const float* dy, int ldd, const float* w, float* dx, int ldx, int B, int H, int W, int C,
                                   int stride, emd_stream_t stream);
int emd_conv3x3_cout1_reflect_wgrad_f32(const float* x, int ldx, const float* dy, float* dw, int B, int H, int W, int Cin,
                                        emd_stream_t stream);
int emd_conv3x3_cout1_reflect_bwd_data_f32(const float* dy, const float* w, float* dx, int ldx, int B, int H, int W, int Cin,
                                           emd_stream_t stream);
/* First layer for training: d4[pix] = (7x7 reflect depthwise of the 1-channel image, 0, 0, 0) -- the pointwise half
 * then runs as a K = 4 GEMM -- and dw49[t] += sum x[reflect(p + t)] * dd4[p][0]. */
int emd_dw7_c1_reflect_f32(const float* x, const float* w49, float* d4, int B, int H, int W, emd_stream_t stream);
int emd_dw7_c1_reflect_wgrad_f32(const float* x, const float* dd4, float* dw49, int B, int H, int W, emd_stream_t stream);
/* g = dy * (1 - y^2): tf.tanh (:372). */
int emd_tanh_bwd_f32(const float* dy, const float* y, float* g, long n, emd_stream_t stream);
/* One feature-matching term (:1027-1035): *loss_acc += weight*mean|a-b|; dy (accumulate ? += : =) weight*sign(a-b)/n. */
int emd_l1_feature_f32(const float* a, const float* b, long n, float weight, float* dy, int accumulate, float* loss_acc,
                       emd_stream_t stream);
/* Gradient of one crop of get_multiscale_crops (:957-980): channel 0 of dcrop [n,n,ldc] is added into dimg [S,S] at
 * the mirror image of padded position (y0+i, x0+j) (padding 3S/4, REFLECT). */
int emd_crop_scatter_f32(const float* dcrop, int ldc, float* dimg, int y0, int x0, int n, int S, emd_stream_t stream);
/* The same with the offset pair (y0, x0) read from DEVICE memory: a captured hipGraph is replayed with new crops. */
int emd_crop_scatter_dev_f32(const float* dcrop, int ldc, float* dimg, const int* yx_dev, int n, int S, emd_stream_t stream);
/* Inference-mode double batch norm of a generator separable conv: (scale, shift) of the forward affine and the vectors
 * its parameter gradients need (see csrc/gan_train.hip); emd_bn_infer_grads_f32 adds them (s1 = sum g,
 * t1 = sum g*(r-mu1)/s1, t2 = sum g*(z1-mu2)/s2 from emd_bn_bwd_reduce_f32). */
int emd_bn_infer_fold2_f32(const float* g1, const float* b1, const float* m1, const float* v1, const float* g2,
                           const float* b2, const float* m2, const float* v2, float eps, int C, float* scale, float* shift,
                           float* mprime, float* rprime, float* rstd1, float* a2, emd_stream_t stream);
int emd_bn_infer_grads_f32(const float* s1, const float* t1, const float* t2, const float* a2, int C, float* dg1, float* db1,
                           float* dg2, float* db2, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Training input functions on the device (csrc/input_ops.hip).  They replace the numpy bodies of
 * misc_py/denoiser-multi-gpu.py:783-870 (get_scale, gen_lq, scale0to1, flip_rotate, preprocess, record_parser), which the
 * reference runs in tf.py_func threads.  Images are dense float32 [B][npix] (or [B][H][W]); all pointers are device
 * pointers.  Random numbers: Philox4x32-10 keyed by `seed`, indexed by (first_image + b, pixel, draw): results do not depend
 * on the launch geometry or on how a data set is cut into batches.  The reference's own stream (numpy Mersenne-Twister
 * re-seeded from itself, :791) is irreproducible by construction; distributions and deterministic formulas are kept. */
/* Raw generator output, for known-answer tests: out[4*i..4*i+3] = Philox4x32-10(counter = (counter0 + i, 0, 0), key = seed). */
int emd_philox4x32_u32(unsigned* out, long n4, unsigned long long seed, unsigned long long counter0, emd_stream_t stream);
/* get_scale (:783-784): scale[b] = 25 + Exp(mean 75). */
int emd_get_scale_f32(float* scale, int B, unsigned long long seed, unsigned long long first_image, emd_stream_t stream);
/* The draw of flip_rotate (:833): choice[b] = int(8 * U[0,1)). */
int emd_d4_choices_i32(int* choice, int B, unsigned long long seed, unsigned long long first_image, emd_stream_t stream);
/* flip_rotate (:830-851) with the element of D4 given per image (choice_dev[b] in 0..7, device memory; NULL = identity):
 * 0 identity, 1-3 np.rot90(img, k), 4 np.flip(img, 0), 5 np.flip(img, 1), 6 / 7 np.flip(np.rot90(img, 1), 0 / 1).
 * Square images only (H == W).  fix_nonfinite != 0 also applies preprocess()'s NaN / Inf -> 0.5 (:855-856).  x != y. */
int emd_flip_rotate_f32(const float* x, float* y, int B, int H, int W, const int* choice_dev, int fix_nonfinite,
                        emd_stream_t stream);
/* Bytes of scratch emd_gen_lq_f32 / emd_minmax_images_f32 need for a batch of B images of npix pixels (16-byte aligned). */
size_t emd_input_workspace_bytes(int B, long npix);
/* Per-image minimum and maximum (the reductions of scale0to1, :817-828); exact. */
int emd_minmax_images_f32(const float* x, int B, long npix, float* mn, float* mx, void* workspace, emd_stream_t stream);
/* scale0to1 (:817-828): y = (x - min) / (max - min) in float32, a constant image becomes 0.5; y may alias x. */
int emd_scale0to1_images_f32(const float* x, float* y, int B, long npix, const float* mn, const float* mx,
                             emd_stream_t stream);
/* gen_lq + the truth rescale of record_parser (:787-799, :861-870): counts = Poisson(img * scale[b]) (exact samplers in
 * double precision: CDF inversion below a rate of 10, Hoermann's PTRS rejection method above), lq = scale0to1(counts)
 * evaluated in float64 and rounded to float32 as numpy does for integer counts, truth = float32(mean(lq) / mean(img)) * img
 * (truth may be NULL).  counts_out (int32 [B][npix]) may be NULL; when given it receives the raw counts. */
int emd_gen_lq_f32(const float* img, const float* scale, float* lq, float* truth, int* counts_out, int B, long npix,
                   unsigned long long seed, unsigned long long first_image, void* workspace, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Graph D as a native executor (csrc/graph_exec.hip, graph_exec_d.hip): architecture() of machine_learning/denoiser.py:58-398 for
 * a host that is not Python.  emd_graph_create takes the weights as HOST float32 arrays keyed by TensorFlow variable name
 * (the names tf.train.Saver stores under scope 'nn', :514: nn/SeparableConv2d[_k]/{depthwise_weights,pointwise_weights},
 * nn/SeparableConv2d[_k]/BatchNorm/{beta,gamma,moving_mean,moving_variance}, nn/BatchNorm[_k]/..., nn/Conv[_k]/{weights,biases},
 * nn/Conv2d_transpose[_k]/{weights,biases}; 658 variables), folds the inference batch norms (float64), packs the matrix-core
 * weights and uploads them into device memory owned by the handle.  emd_graph_run launches the whole forward pass on `stream`:
 * x, y device float32 [B,S,S,1] (S a multiple of 16; no output clip, :396), activations in the caller's `workspace` (device
 * memory, emd_graph_workspace_bytes(g, B, S) bytes).  Same kernels in the same order as emdenoise.denoiser.DenoiserEngine:
 * bit-identical results.  variant: 0 = graph D; 1 = graph D', the inference graph of the training twin
 * misc_py/denoiser-multi-gpu.py:200-540 (phase=False): tf.layers variable names (nn/conv2d[_k]/{kernel,bias}, nn/conv2d_transpose[_k]/...,
 * the ASPP convs nn/{1x1,lowRate,mediumRate,highRate,imageLevel,pellet}), dense dilated 3x3 ASPP branches, a real image-level
 * branch, output clipped to [0,1] (:534-538); 2 = graph X, the Xception autoencoder misc_py/modified_Xception.py:194-654 (variables under
 * scope "pellet": pellet/conv2d[_k]/{kernel,bias}, pellet/SeparableConv2d[_k]/{depthwise_weights,pointwise_weights,BatchNorm/...},
 * pellet/conv2d_transpose[_k]/..., pellet/{1x1,lowRate,mediumRate,highRate,imageLevel}/..., pellet/BatchNorm[_k]/...; S a multiple of 64;
 * the separable convs' norms run on the statistics of the batch handed to emd_graph_run; output clipped to [0,1]), same kernels as
 * emdenoise.xception.XceptionEngine, bit-identical; 3 = graph G's generator misc_py/gan-infilling-100.py:133-374 (variables under
 * "GAN/Gen" and "GAN/Gen/reg"; x = the 1/64-sampled image with missing pixels -1, S a multiple of 16, >= 32; y in (-1,1)), same kernels
 * as emdenoise.gan.GeneratorEngine, bit-identical.
 * A handle is NOT re-entrant: emd_graph_run calls on one handle must be serialised by the caller (one stream, one thread at a
 * time) -- the fork / join events and the side streams of the two-streams form belong to the handle; use one handle per
 * concurrent stream (the weights are ~100 MB).  emd_graph_workspace_bytes returns the larger of the two launch forms' needs, so a
 * size asked for before emd_graph_set_two_streams stays valid after it; the query writes nothing to the handle.  emd_graph_create returns EMD_E_ALLOC when a device
 * allocation or upload fails (EMD_E_INVALID: a missing / mis-sized variable). */
typedef struct emd_graph emd_graph_t;
int emd_graph_create(emd_graph_t** graph, int variant, int n_vars, const char* const* names, const float* const* host_data,
                     const long* counts);
size_t emd_graph_workspace_bytes(emd_graph_t* graph, int B, int S);
int emd_graph_run(emd_graph_t* graph, const float* x, float* y, int B, int S, void* workspace, size_t workspace_bytes,
                  emd_stream_t stream);
void emd_graph_destroy(emd_graph_t* graph);
/* Launch-order option (speed only, same bits): on != 0 runs the 1/16-resolution flow (denoiser.py:312-325) of an even batch as two
 * halves on two internal streams, forked from and joined to `stream` (capturable), as the Python engine does.  If the side
 * streams cannot be created the run falls back to the single-stream sequence (same results).  Default off: measured slower from a host that enqueues as fast as C
 * does. */
int emd_graph_set_two_streams(emd_graph_t* graph, int on);

/* ------------------------------------------------------------------------------------------------
 * Whole-micrograph tiling (csrc/tile_ops.hip): the image preparation, crop stacking, per-crop rescale and
 * overlap-add blending around the networks, so that a whole micrograph is denoised on the device.
 * replaces: the host numpy of Denoiser.denoise / .preprocess (machine_learning/denoiser.py:632-682), of the graph-S
 *           Micrograph_Autoencoder.denoise / .preprocess (misc_py/apply_autoencoders.py:346-534) and of the graph-K
 *           Micrograph_Autoencoder.denoise (misc_py/apply_kernels+MLPs.py:611-703).
 *
 * Images are [N,H,W] float32.  A tile plan is the caller's (emdenoise.tiling computes it), in DEVICE int32 arrays:
 *   ys[ny], xs[nx]      tile start rows / columns in the coordinates of the image reflect-padded by `pad`;
 *                       tile t = (n, i, j) = n*ny*nx + i*nx + j starts at (ys[i], xs[j]) of image n
 *   row_range[2*H]      for each row y of the (un-padded) image, the tiles [first, last) of ys whose kept rows
 *                       [ys[i] + m, ys[i] + cs - m) contain y + pad; col_range[2*W] the same for columns
 * Rows and columns outside the image are read with numpy's mode="reflect" indexing (any distance), so no padded copy
 * exists and no plan content can make a kernel read outside the image.  Nothing uses atomics; every result is deterministic. */
#define EMD_TILE_PREP_S 0 /* autoencoder preprocess (:346-358): NaN/Inf -> 0, scale0to1, divide by the image mean */
#define EMD_TILE_PREP_K 1 /* graph K (:638-660): NaN/Inf -> 0, statistics of the image reflect-padded by param, (x - off) / scale */
#define EMD_TILE_PREP_D 2 /* Denoiser.preprocess (:632-643): cv2-style half-pixel bilinear resize to param x param (edge
                           * clamp), scale0to1, NaN/Inf -> 0.5, scale0to1, with numpy's NaN semantics (a NaN anywhere after
                           * the resize makes the whole image 0.5) */
/* Bytes of scratch emd_tile_prep_f32 needs (same arguments). */
size_t emd_tile_prep_workspace_bytes(int N, int H, int W, int mode, int param);
/* Per-image preparation, x [N,H,W] -> y: [N,H,W] for S and K (y may alias x), [N,param,param] for D (y != x).  Means
 * accumulate in double and round to float32 once.  K: param = pad (0 <= pad < min(H,W)); stats (double [N][3], required)
 * receives (off, scale, flat) per image for emd_tile_affine_f32: off = min, scale = float32(mean of the padded image) - off
 * in double (0 for a flat image, which becomes 1.0).  stats is ignored by S and D. */
int emd_tile_prep_f32(const float* x, float* y, int N, int H, int W, int mode, int param, double* stats, void* workspace,
                      size_t workspace_bytes, emd_stream_t stream);
/* Crop stack: out[c] (c < count, [count][cs][cs]) = tile t0 + c of the plan, src[n, ys[i] - pad + a, xs[j] - pad + b].
 * crop_stats == NULL: a verbatim copy (numpy slicing of the padded image; graph D).  Otherwise (graph S, :304-308) each
 * crop is rescaled: off = min, scale = float32(mean) - off, out = (x - off) / scale, or 1.0 for a flat crop (scale == 0);
 * crop_stats[c] = (off, scale) (float [count][2]).  Needs cs <= H + 2*pad and cs <= W + 2*pad, t0 + count <= N*ny*nx. */
int emd_tile_gather_f32(const float* src, int N, int H, int W, int pad, int cs, const int* ys, int ny, const int* xs, int nx,
                        int t0, int count, float* out, float* crop_stats, emd_stream_t stream);
/* Overlap-add of all N*ny*nx tile predictions preds [N*ny*nx][cs][cs] into out [N,H,W] (the un-padded core): each output
 * pixel sums, in ascending tile order and in double, the tiles whose kept window (margin m, 0 <= m < cs/2) covers it,
 * divides by their count, optionally clips to [0,1] (clip = 1) and rounds once.  crop_stats != NULL (graph S) first maps each
 * prediction back with the crop's (off, scale) from emd_tile_gather_f32: pred * scale + off in float32. */
int emd_tile_blend_f32(const float* preds, const float* crop_stats, int N, int H, int W, int pad, int cs, int m, const int* ys,
                       int ny, const int* xs, int nx, const int* row_range, const int* col_range, int clip, float* out,
                       emd_stream_t stream);
/* Graph K's inverse rescale (:700-701): y = x * scale + off, or x * off for a flat image (scale == 0), per image, with the
 * (off, scale, flat) of emd_tile_prep_f32(EMD_TILE_PREP_K), in double, rounded once; y may alias x. */
int emd_tile_affine_f32(const float* x, float* y, int N, long npix, const double* stats, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Image-quality metrics (csrc/ssim.hip): SSIM, MS-SSIM, PSNR and the SSIM loss term with its gradient.
 * replaces: misc_py/denoiser-multi-gpu.py:124-139 (_tf_fspecial_gauss), :142-167 (tf_ssim), :170-192 (tf_ms_ssim) and the
 *           loss term of _tower_fn, :775 (tower_loss += 1.0 - tf_ssim(out, truth)); the same functions again in
 *           misc_py/modified_Xception.py:123-191, :649.
 *
 * x, y       : [B,H,W] float32 (NHWC with C == 1), contiguous; 0 <= B <= 65535 (B == 0 is a no-op).
 * taps_host  : HOST array of `size` floats, the 1-D window g (the reference's 2-D window is the outer product g x g:
 *              exp(-i^2 / (2 sigma^2)), i = -size/2 .. size/2, divided by its sum); size odd, 3..15, H, W >= size.
 * Maps are VALID correlations, [B, H-size+1, W-size+1]; C1 = 0.01^2, C2 = 0.03^2 (L = 1).
 * Workspaces are the caller's, 16-byte aligned, sized by the emd_*_workspace_bytes of the same arguments (0 for arguments
 * the routine would refuse).  Sums over a map are formed per tile in float32, then in double in a fixed order: no atomics,
 * every result is bitwise reproducible. */
size_t emd_ssim_workspace_bytes(int B, int H, int W, int size);
/* means [B+1][2] = (mean ssim_map, mean cs_map) of each image, row B the mean over the whole batch (the mean of the rows;
 * tf.reduce_mean of :166, :176-177).  ssim_map / cs_map: optional outputs [B, H-size+1, W-size+1] (NULL: no map and no
 * moment is written to memory). */
int emd_ssim_f32(const float* x, const float* y, int B, int H, int W, const float* taps_host, int size, float* means,
                 float* ssim_map, float* cs_map, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_ssim_loss_workspace_bytes(int B, int H, int W, int size);
/* L = 1 - mean(ssim_map) and its gradient with respect to x (none for y).  result [B+1][2] = (mean ssim, L) per image, row B for
 * the batch mean.  dout (optional, [B,H,W], may not alias x or y) is ACCUMULATED: per_image != 0: dout[b] += scale *
 * (scale_dev ? scale_dev[b] : 1) * dL_b/dx[b] with L_b image b's own loss; per_image == 0: the same with L the batch loss
 * (dL/dx[b] = dL_b/dx[b] / B).  loss_acc (optional): loss_acc[b * acc_stride] += acc_weight * L_b (per_image), or
 * loss_acc[0] += acc_weight * L.  scale_dev: optional DEVICE array of B floats.  The taps must be symmetric (the gradient
 * is the full correlation with the same window, gathered per input pixel). */
int emd_ssim_loss_f32(const float* x, const float* y, int B, int H, int W, const float* taps_host, int size, int per_image,
                      float scale, const float* scale_dev, float* dout, float* result, float* loss_acc, int acc_stride,
                      float acc_weight, void* workspace, size_t workspace_bytes, emd_stream_t stream);
/* tf.nn.avg_pool(x, [1,2,2,1], [1,2,2,1], 'SAME') on one channel (:178-179): x [B,H,W] -> y [B,(H+1)/2,(W+1)/2]; for an odd
 * extent the last window holds one row / column and the sum is divided by the number of valid elements.  y != x. */
int emd_avgpool2x2_same_c1_f32(const float* x, float* y, int B, int H, int W, emd_stream_t stream);
size_t emd_ms_ssim_workspace_bytes(int B, int H, int W, int level, int size);
/* tf_ms_ssim (:170-192): `level` (1..5) SSIM passes with the 2x2 SAME average pool between them, weights 0.0448, 0.2856,
 * 0.3001, 0.2363, 0.1333; value [B+1]: value[B] = prod(mcs[0:level-1] ** w[0:level-1]) * mssim[level-1] ** w[level-1] from
 * the batch means (the reference's value), value[b] the same formula on image b's own means.  A negative mean cs under a
 * fractional power gives NaN, as in the reference.  Needs H, W >= size * 2^(level-1).
 * level_means: optional output [level][B+1][2], the emd_ssim_f32 means of every level. */
int emd_ms_ssim_f32(const float* x, const float* y, int B, int H, int W, int level, const float* taps_host, int size, float* value,
                    float* level_means, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_psnr_workspace_bytes(int B, long npix);
/* out [B+1][2] = (mse, 10 log10(data_range^2 / mse)) of each image of npix pixels, row B for the batch mse (the mean of
 * the images'); sums in double; mse == 0 gives +inf. */
int emd_psnr_f32(const float* x, const float* y, int B, long npix, float data_range, float* out, void* workspace,
                 size_t workspace_bytes, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Classical baseline filters (csrc/filters.hip): the methods of the reference's comparison table,
 * misc_py/err_hist_maker.py:26-45 (Gaussian, Bilateral, Median, Wiener, Chambolle; "Wavelet": csrc/wavelet.hip, below), and the ground-truth
 * blur of misc_py/blur_images.py:13 (cv2.GaussianBlur(img, (3,3), 1.5) = the Gaussian with ksize 3, sigma 1.5).
 *
 * x, out : [B,H,W] float32 (NHWC with C == 1), contiguous, finite; 0 <= B <= 65535 (B == 0 is a no-op); every image of the
 *          batch is filtered on its own.  out may NOT alias or overlap x in any of the five filters: a tile reads the pixels
 *          of its neighbours (the total-variation iteration re-reads x with a halo in every launch, the last one included).
 * "Mirror" border: reflect-101, d c b | a b c d | c b a (cv2's default, tf.pad REFLECT, graph K's); needs radius < min(H,W).
 * Workspaces are the caller's, 16-byte aligned, sized by the emd_*_workspace_bytes of the same arguments (0 for arguments the
 * routine would refuse).  No atomics: every result is bitwise reproducible.  All arguments are checked before any launch. */
/* Separable correlation with the 1-D taps taps_host (HOST array of ksize floats; ksize odd, 3..15), mirror border. */
int emd_filter_gaussian_f32(const float* x, float* out, int B, int H, int W, const float* taps_host, int ksize, emd_stream_t stream);
/* Median of the ksize x ksize window, ksize 3 or 5, mirror border: one of the input values, bit for bit. */
int emd_filter_median_f32(const float* x, float* out, int B, int H, int W, int ksize, emd_stream_t stream);
/* out[p] = sum_q w x[q] / sum_q w over the taps q = p + (dx, dy) with dx^2 + dy^2 <= (d/2)^2 (cv2's circular support),
 * w = exp(-(dx^2 + dy^2) / (2 sigma_space^2)) exp(-(x[q] - x[p])^2 / (2 sigma_color^2)); d odd, 3..9; mirror border. */
int emd_filter_bilateral_f32(const float* x, float* out, int B, int H, int W, int d, float sigma_color, float sigma_space,
                             emd_stream_t stream);
size_t emd_filter_wiener_workspace_bytes(int B, int H, int W);
/* scipy.signal.wiener: m, v = mean and variance of the ksize x ksize window of the ZERO-padded image (divided by ksize^2 at the
 * border too); out = m + (x - m) (1 - n / v) where v >= n and v > 0, else m (scipy's 0 / 0 on a constant image: here m).
 * ksize odd, 3..9.  noise >= 0: n = noise, one launch, the workspace is not used (may be NULL).  noise < 0: n of each image
 * = the mean of its own v, two launches.  noise_out (optional, [B]) receives the n used. */
int emd_filter_wiener_f32(const float* x, float* out, int B, int H, int W, int ksize, float noise, float* noise_out, void* workspace,
                          size_t workspace_bytes, emd_stream_t stream);
size_t emd_filter_tv_workspace_bytes(int B, int H, int W);
/* Chambolle's dual projection for total-variation denoising, a FIXED number of iterations (no stopping rule: capturable):
 * p = 0; n_iter times: u = x + div p, div p [i,j] = -p1[i,j] - p2[i,j] + p1[i-1,j] + p2[i,j-1] (0 outside the image);
 * g1 = u[i+1,j] - u[i,j] (0 on the last row), g2 = u[i,j+1] - u[i,j] (0 on the last column);
 * p <- (p - tau g) / (1 + (tau / weight) sqrt(g1^2 + g2^2)), tau = 0.25.  out = the last u (n_iter == 1: x).  weight > 0,
 * n_iter >= 1; one launch per iteration. */
int emd_filter_tv_f32(const float* x, float* out, int B, int H, int W, float weight, int n_iter, void* workspace,
                      size_t workspace_bytes, emd_stream_t stream);
/* out = min(max(x, 0), 1) over n floats (the comparison table's optional clip before scoring).  Element-wise: here, and only
 * here, out may be x itself (in place); a partial overlap is refused. */
int emd_filter_clip01_f32(const float* x, float* out, long n, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 2-D orthogonal wavelet transform and wavelet-shrinkage denoising (csrc/wavelet.hip): the "Wavelet" method of
 * misc_py/err_hist_maker.py:27.  The script that filled the reference's array is not in the reference; what is built is the
 * arithmetic of skimage.restoration.denoise_wavelet at its defaults (BayesShrink, soft threshold, sigma estimated from the image),
 * from the formulas below -- neither skimage nor pywt is a dependency.
 *
 * A wavelet is its reconstruction low-pass taps rec_lo[0..L-1] (HOST array of doubles; L = ntaps even, 2..8; rounded to float32
 * once): dec_lo[k] = rec_lo[L-1-k], dec_hi[k] = (-1)^(k+1) rec_lo[k], rec_hi[k] = dec_hi[L-1-k].
 * Analysis along an axis of length N -> n = (N + L - 1) / 2 coefficients: c[i] = sum_k dec[k] x~[2i + 1 - k] with x~ the
 * half-sample symmetric extension (x~[-1] = x[0], x~[N] = x[N-1], period 2N: pywt's "symmetric"; NOT the reflect-101 of the
 * filters above).  A 2-D step filters along H, then along W: cA (low, low), ad (low along H, high along W), da (high along H, low
 * along W), dd (high, high), each nH x nW; `levels` steps, each on the previous cA.
 * Synthesis along an axis: x[j] = sum_i a[i] rec_lo[j + L - 2 - 2i] + d[i] rec_hi[j + L - 2 - 2i] over 0 <= j + L - 2 - 2i < L,
 * 2n - L + 2 samples, along W first, then along H; a level's result is cropped to the shape of the level below (pywt's waverecn
 * rule: an approximation one sample longer than its detail bands loses its last sample), the last to (H, W).
 * 1 <= levels <= floor(log2(min(H,W) / (L - 1))), which must be >= 1; H, W <= 32768; 0 <= B <= 65535 (B == 0 is a no-op).
 *
 * The pyramid of one image is packed: cA_levels, then ad, da, dd of level `levels`, of level levels - 1, ..., of level 1; the
 * batch is [B][emd_wavelet_pyramid_floats].  Workspaces are the caller's, 16-byte aligned, sized by the *_workspace_bytes of the
 * same arguments (0 for arguments the routine would refuse); no buffer may overlap another.  No float atomics: every result is
 * bitwise reproducible.  All arguments are checked before any launch; one analysis / synthesis launch per level. */
/* Floats of one image's pyramid (0: refused).  bands (optional, HOST, [1 + 3 levels][3]): (offset in floats, rows, columns) of
 * cA_levels, then ad, da, dd from the coarsest level to the finest. */
size_t emd_wavelet_pyramid_floats(int H, int W, int ntaps, int levels, long* bands);
size_t emd_wavelet_workspace_bytes(int B, int H, int W, int ntaps, int levels);
/* x [B,H,W] -> pyramid [B][emd_wavelet_pyramid_floats]. */
int emd_wavelet_forward_f32(const float* x, float* pyramid, int B, int H, int W, const double* rec_lo_host, int ntaps, int levels,
                            void* workspace, size_t workspace_bytes, emd_stream_t stream);
/* pyramid -> out [B,H,W]. */
int emd_wavelet_inverse_f32(const float* pyramid, float* out, int B, int H, int W, const double* rec_lo_host, int ntaps, int levels,
                            void* workspace, size_t workspace_bytes, emd_stream_t stream);
#define EMD_WAVELET_BAYES 0 /* t = var / sqrt(max(mean(d^2) - var, FLT_EPSILON)) for every detail band d of every level */
#define EMD_WAVELET_VISU 1  /* t = sigma sqrt(2 ln(H W)), the same for every band */
size_t emd_filter_wavelet_workspace_bytes(int B, int H, int W, int ntaps, int levels);
/* out = inverse(soft(forward(x))), soft(d) = sign(d) max(|d| - t, 0) on the detail bands only (applied as synthesis loads them: no
 * thresholded coefficient is written to memory; cA is never thresholded); var = sigma^2; mean(d^2) from per-tile double sums added
 * in a fixed order.  sigma >= 0: used for every image.  sigma < 0: per image, median(|dd_1| over the coefficients that are not
 * exactly 0) / 0.6744897501960817 with dd_1 the finest diagonal band (skimage's _sigma_est_dwt); the median is exact (an even
 * count: (a + b) 0.5 of the two middle values, in float32), found by a radix selection on integer histograms, so it is the same
 * bits on every run; no non-zero coefficient: sigma = 0 and every threshold is 0.  sigma_used (optional, [B]) receives the sigma
 * used.  Hard thresholding and skimage's final clip to [0,1] are not built (emd_filter_clip01_f32 is the clip).  Launches only, on
 * `stream`: capturable. */
int emd_filter_wavelet_f32(const float* x, float* out, int B, int H, int W, const double* rec_lo_host, int ntaps, int levels, int method,
                           float sigma, float* sigma_used, void* workspace, size_t workspace_bytes, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Harvesting raw micrographs (csrc/harvest.hip): what the reference's MATLAB harvester does to a raw image before
 * it becomes a training image -- DM3stoTIFs-batch/img_params.m, img_params_lq.m, estimate_noise.m: crop to the smaller dimension,
 * box-resize to 2048 x 2048, a table of statistics, rescale to [0, 1].  MATLAB is not a dependency: the arithmetic is restated
 * from the formulas below.
 *
 * Crop: d = min(H, W), the top-left d x d pixels (imcrop(img, [1, 1, d-1, d-1])).
 *
 * Box resize d -> S (imresize(crop, [S, S], 'method', 'box'), antialiasing on).  For one axis, with 1-based indices, everything in
 * IEEE double, evaluated in exactly this order with no fused multiply-add:
 *     scale = S / d;   kw = scale < 1 ? 1 / scale : 1
 *     for x = 1..S:    u = x / scale + 0.5 * (1 - 1 / scale);   left = floor(u - kw / 2)
 *                      candidates i = left .. left + ceil(kw) + 1
 *                      i is a member iff -0.5 <= t && t < 0.5,  t = scale < 1 ? scale * (u - i) : (u - i)
 * An output sample is the UNWEIGHTED mean of its member pixels (not fractional coverage: this is not cv2.INTER_AREA); S > d is
 * nearest neighbour.  The members of an output are one contiguous run inside 1..d (MATLAB's mirror fold of indices never applies
 * to this kernel), but where a candidate lands on a tie the double arithmetic above decides, not exact rational arithmetic: the
 * table must come from these expressions.  The crop is square, so both axes share one table, and an output pixel is the mean over
 * (its row run) x (its column run), summed in double in a fixed order and rounded to float32 once.
 *
 * Statistics of an H x W image (H, W >= 3; finite values: NaN / Inf are the caller's problem), N = H W, EMD_NSTATS doubles in
 * this order:
 *      0 min                 1 max
 *      2 nonzero             count of x != 0                       3 negative      count of x < 0
 *      4 mean                                                      5 std           N - 1 denominator (MATLAB std2)
 *      6 skewness            m3 / m2^1.5                           7 kurtosis      m4 / m2^2  (population central moments m_k =
 *                                                                                  sum (x - mean)^k / N; not excess)
 *      8 median              even N: the mean of the two middle values, formed in double; -0 and +0 are equal
 *      9 rms                 sqrt(sum x^2 / N)                    10 coeff_variation  100 std / mean
 *     11 noise               sum |conv2_full(x, [1 -2 1; -2 4 -2; 1 -2 1])| sqrt(pi / 2) / (6 (W - 2) (H - 2)), the sum over the
 *                            (H + 2) x (W + 2) full, zero-padded convolution (estimate_noise.m:8; Immerkaer's estimate)
 *     12 sqrt_mean  13 sqrt_std  14 sqrt_skewness  15 sqrt_kurtosis    the same four moments of sqrt(max(x, 0))
 *     16 sqrt_mean_ratio     sqrt_mean / mean
 * Central moments are two-pass (the mean first, then sum (x - mean)^k in double); every sum is in double, per-workgroup partial
 * sums combined in a fixed order; the median is exact, by a four-pass radix selection on integer histograms.  No floating-point
 * atomics: bitwise reproducible, and an image's result does not depend on B.  A constant image has m2 = 0: skewness and kurtosis
 * are NaN, as in MATLAB.
 *
 * Scale to [0, 1]: (x - min) / (max - min) in float32; |max - min| < 1e-6 (a constant image) gives 0.5 -- this library's
 * scale0to1 rule; the MATLAB gives NaN there (a documented deviation).
 *
 * 0 <= B <= 65535 (B == 0 is a no-op); launches only, on `stream`, no host synchronisation: capturable. */
#define EMD_NSTATS 17
/* HOST only: tab[n_out][2] = (first member, 0-based; member count) of every output sample of the box resize n_in -> n_out, from
 * the expressions above.  The one copy of the table arithmetic.  1 <= n_in <= 32768, 1 <= n_out <= 8192. */
int emd_box_resize_table(int n_in, int n_out, int* tab);
/* y[b] ([B,S,S], contiguous) = box resize of the top-left d x d pixels of image b at x + b * image_stride, rows row_stride floats
 * apart (the crop is expressed by row_stride and d).  tab_dev: DEVICE copy of emd_box_resize_table(d, S); runs are clamped to
 * 0..d-1 whatever it holds.  1 <= d <= 32768, 1 <= S <= 8192, row_stride >= d.  y may not overlap x. */
int emd_box_resize_f32(const float* x, long image_stride, int row_stride, int B, int d, float* y, int S, const int* tab_dev,
                       emd_stream_t stream);
size_t emd_image_stats_workspace_bytes(int B, int H, int W);
/* x [B,H,W] -> stats [B][EMD_NSTATS] (DEVICE, doubles).  3 <= H, W <= 32768.  The workspace is the caller's, 16-byte aligned. */
int emd_image_stats_f64(const float* x, int B, int H, int W, double* stats, void* workspace, size_t workspace_bytes,
                        emd_stream_t stream);
/* y [B][n] = scale to [0, 1] of x [B][n] with min, max = stats[b][0], stats[b][1] of emd_image_stats_f64, read on the device.
 * Element-wise: y may be x itself. */
int emd_scale01_f32(const float* x, float* y, int B, long n, const double* stats, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * The 2-D FFT and the radial frequency profile (csrc/fft.hip): img_params.m:53-77, the four *Freq2048 fields.
 * x is [B,S,S] float32, S a power of two, 8 <= S <= 4096 (one line of 4096 complex doubles is 64 KiB of LDS); finite values.
 *
 * Transform: F = fft2(double(x)), forward, unnormalised, in double.  spec is numpy.fft.rfft2's layout, [B][S][S/2 + 1] interleaved
 * (re, im), unshifted: ky = 0..S-1, kx = 0..S/2.
 *
 * Profile: with the signed frequencies ky, kx in [-S/2, S/2 - 1] (fftshift, mid = S/2 + 1), n = ky^2 + kx^2 and
 * R = ceil(sqrt(2 mid^2)) (1450 at 2048), a pixel's 0-based bin is ceil(sqrt(n)): the smallest integer t with t^2 >= n, in integer
 * arithmetic.  radialProfile[t] = the sum of |F| over the bin; radialFreqs[t] = sqrt(n) / R of the bin's member with the largest kx,
 * and among those the largest ky (the last one the reference's loop -- col outer, row inner -- visits; not a bin centre); a bin
 * without a member has profile 0 and frequency 0 and still counts below.
 *     p = radialProfile / sum(radialProfile) * radialFreqs          [R]
 *     freq_stats[b] = { sum(p), std(p) with R - 1, skewness(p), kurtosis(p) }   (EMD_NFREQ doubles; m3 / m2^1.5 and m4 / m2^2 of the
 *                      population central moments about sum(p) / R, two-pass; "mean" is the SUM, as in the reference)
 * An all-zero image has sum(radialProfile) = 0: p and the four are NaN.  A constant non-zero image has all its energy at n = 0, whose
 * frequency is 0: p = 0, mean = 0, std = 0, and skewness and kurtosis are 0/0 = NaN.  Both as in MATLAB.
 * No floating-point atomics and fixed summation orders: bitwise reproducible, and an image's result does not depend on B.
 * 0 <= B <= 65535 (B == 0 is a no-op); the workspace is the caller's, 16-byte aligned, as are spec and freq_stats; the twiddle
 * table is written into it by a kernel on every call; launches only, on `stream`, no host synchronisation: capturable. */
#define EMD_NFREQ 4
int emd_radial_bins(int S); /* R; 0 for an invalid S */
size_t emd_rfft2_workspace_bytes(int B, int S);
int emd_rfft2_f64(const float* x, int B, int S, double* spec, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_freq_stats_workspace_bytes(int B, int S);
/* profile [B][R] = p, may be NULL; freq_stats [B][EMD_NFREQ] (both DEVICE, doubles) */
int emd_freq_stats_f64(const float* x, int B, int S, double* profile, double* freq_stats, void* workspace, size_t workspace_bytes,
                       emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exit-wave reconstruction from a through-focus series (csrc/exitwave.hip): ewrec_class.py:100-110, :272-380.
 * Everything is double precision; complex arrays are interleaved (re, im) doubles.  Square images of side s; the padded side is
 * S = s (1 + pad_periods), a power of two, 8 <= S <= 4096 (pad_periods = 0, 1, 3, ...): the image sits at the top-left of an S x S
 * array of zeros.  `defocus` is always a DEVICE pointer to one double per image: a search loop changes it without an upload inside
 * the call, and a captured graph reads the new values on replay.
 *
 * Transfer function, at the unshifted (FFT-order) indices: j = i for i < S/2, else i - S; q = (double)j / ((double)S * px);
 *     q2 = qy qy + qx qx;   t = lam df q2 + 0.5 lam^3 Cs q2 q2   (left to right, lam^3 = lam lam lam, every operation rounded on
 *     its own);   H = cospi(t) + i sinpi(t).
 * px (the pixel size) replaces the reference's `px_dim = 1 + pad_periods`.  H is [n][S][S].
 *
 * cfft2: numpy.fft.fft2 / ifft2 of x [B][S][S] (inverse != 0: normalised by 1 / S^2).
 * propagate: out[b] = ifft2(fft2(pad(psi[b])) H(defocus[b]))[:s, :s], [B][s][s]; psi is complex, or float32 (the real part) when
 *     psi_is_real_f32 != 0.  Rows and columns of the padding are never read or transformed on the way in, and only the s rows that
 *     are kept are transformed on the way out.
 * reconstruct: images [N][s][s] float32, 1 <= N <= 64; a_k = |image_k| (EMD_EXITWAVE_FROM_INTENSITY: sqrt(max(image_k, 0)));
 *     psi_k starts as image_k + 0i (FROM_INTENSITY: as a_k); `iterations` times:  E = (sum_k P(psi_k, -df_k)) / N in ascending k;  b_k = P(E, +df_k);
 *     psi_k = a_k b_k / |b_k|  (a_k where |b_k| = 0: the reference gives NaN).  E [s][s] is the last iteration's; stack (may be
 *     NULL) [N][s][s] the last psi; losses (may be NULL) [N]: with I = |b_k|^2 of the last iteration and c = mean(image_k) / mean(I),
 *     mean((image_k - c I)^2), two-pass in double.  With pad_periods == 0 the iteration runs in the frequency domain, two launches
 *     per iteration for the whole stack; with pad_periods > 0 it is composed from the launches of emd_propagate_f64.
 *     With Cs != 0, P(psi, -df) multiplies by H(-df), as the reference does, which is not conj H(df): the Cs term keeps its sign.
 * No floating-point atomics, fixed summation orders: bitwise reproducible.  The workspace is the caller's; it, the inputs and the
 * outputs are 16-byte aligned (defocus and losses: 8-byte, checked too) and may not overlap.  Launches only, on `stream`: capturable. */
#define EMD_EXITWAVE_FROM_INTENSITY 1 /* the only bit of `flags` */
int emd_transfer_function_f64(int S, int n, const double* defocus, double wavelength, double px, double cs, double* H,
                              emd_stream_t stream);
size_t emd_cfft2_workspace_bytes(int B, int S);
int emd_cfft2_f64(const double* x, int B, int S, int inverse, double* out, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_propagate_workspace_bytes(int B, int s, int pad_periods);
int emd_propagate_f64(const void* psi, int psi_is_real_f32, int B, int s, int pad_periods, const double* defocus, double wavelength,
                      double px, double cs, double* out, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_exitwave_workspace_bytes(int N, int s, int pad_periods);
int emd_exitwave_reconstruct_f64(const float* images, int N, int s, int pad_periods, const double* defocus, double wavelength, double px,
                                 double cs, int iterations, int flags, double* E, double* stack, double* losses, void* workspace,
                                 size_t workspace_bytes, emd_stream_t stream);

/* Candidates and the defocus search: ewrec_class.py:382-434, `defocus_initial_estimate`, repaired.
 *
 * candidates: one stack images [N][s][s] reconstructed under C defocus tables, defocus_table [C][N] (DEVICE doubles), 1 <= C <= 64,
 *     C N <= 65535, everything else as emd_exitwave_reconstruct_f64.  losses [C][N]; worst [C] = the largest loss over k, taken in
 *     ascending k, NaN if any loss is NaN; E [C][s][s] and stack [C][N][s][s] may be NULL.  For every c, losses[c], E[c] and
 *     stack[c] are bit for bit what emd_exitwave_reconstruct_f64 gives for defocus_table[c] alone: a candidate's bits do not depend
 *     on C or on the other candidates.  With pad_periods == 0 the candidates are a grid dimension (2 iterations + 6 launches, + 1
 *     with E, + 1 with the stack, whatever C is); with pad_periods > 0 they run one after the other inside the call.
 *
 * search, over defocuses = increment * ramp; ramp [N] and seed are DEVICE doubles, every decision is made on the device, nothing
 *     is read back: capturable, and a replay reads new images, ramp and seed.  Every operation below is rounded on its own.
 *   EMD_SEARCH_SECTION, 3 <= C <= 64, `rounds` rounds, seed = (lo, hi).  A round: inc_c = lo + c ((hi - lo) / (C - 1)) for
 *     c < C - 1, inc_{C-1} = hi; table[c][k] = inc_c ramp[k]; one candidates call; i = the first index of the smallest FINITE worst
 *     loss; (best increment, best loss) is replaced by (inc_i, worst_i) only if worst_i is strictly smaller; the next bracket is
 *     (inc[max(i-1, 0)], inc[min(i+1, C-1)]).  No finite candidate: the bracket stays and EMD_SEARCH_NONFINITE is set.  The
 *     result is the best over ALL rounds (NaN, +inf if there never was one); steps = the rounds that had a finite candidate.
 *   EMD_SEARCH_PLATEAU (the reference's loop), C = 1, `rounds` = the largest number of steps, seed = (incr1, incr2, prev).  A step:
 *     inc = 0.5 (incr1 + incr2); one reconstruction; loss < prev: (incr1, incr2, prev) = (incr2, inc, loss); else the search is
 *     done (a non-finite loss: done, with EMD_SEARCH_NONFINITE).  The launches of the later steps still run: they evaluate incr2
 *     and change nothing.  The result is (incr2, prev); steps = the steps taken before done; EMD_SEARCH_UNFINISHED: never done.
 *   result [2] = (increment, loss); history_increments, history_losses [rounds][C]: every candidate and its worst loss; status [2]
 *     (ints) = (status bits, steps); E [s][s] (may be NULL): the exit wave at the result, by one more reconstruction. */
#define EMD_SEARCH_SECTION 0
#define EMD_SEARCH_PLATEAU 1
#define EMD_SEARCH_NONFINITE 1  /* status bit 1 */
#define EMD_SEARCH_UNFINISHED 2 /* status bit 2 */
size_t emd_exitwave_candidates_workspace_bytes(int C, int N, int s, int pad_periods);
int emd_exitwave_candidates_f64(const float* images, int C, int N, int s, int pad_periods, const double* defocus_table, double wavelength,
                                double px, double cs, int iterations, int flags, double* losses, double* worst, double* E, double* stack,
                                void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_exitwave_search_workspace_bytes(int method, int C, int N, int s, int pad_periods);
int emd_exitwave_search_f64(const float* images, int N, int s, int pad_periods, const double* ramp, const double* seed, int method, int C,
                            int rounds, double wavelength, double px, double cs, int iterations, int flags, double* result,
                            double* history_increments, double* history_losses, int* status, double* E, void* workspace,
                            size_t workspace_bytes, emd_stream_t stream);

/* Candidate stacks and the refinement of crop centres and defocuses: ewrec_class.py:436-478, `refine_params` and
 * `reconstruction_loss_arbitrary_params`, which do not run as written; the formulas below are the specification.
 *
 * crop_candidates: images [N][S0][S0] float32, centres_table [C][N][2] (DEVICE doubles), out [C][N][side][side], C N <= 65535: one
 *     launch with the candidate as a grid dimension; out[c] is bit for bit emd_crop_stack_f32 under centres_table[c].
 *
 * candidate_stacks: emd_exitwave_candidates_f64 with images [C][N][s][s]: candidate c has its own N images.  losses[c], worst[c],
 *     E[c] and stack[c] are bit for bit what emd_exitwave_reconstruct_f64 gives for images[c] and defocus_table[c] alone; the same
 *     kernels, launch counts and workspace as emd_exitwave_candidates_f64.  The images are 4-byte aligned (a chunk of the candidates
 *     of a larger array starts at any image); everything else as there.
 *
 * refine: a compass (pattern) search that minimises the largest per-image loss over the crop centres and the defocuses, jointly.
 *     images [N][S0][S0] float32, 2 <= N <= 64, 1 <= S0 <= 4096; the crops are side x side (emd_crop_stack_f32's arithmetic, pad_val
 *     outside the frame), side (1 + pad_periods) a power of two in 8..4096; the optics, iterations, flags and pad_periods are
 *     emd_exitwave_reconstruct_f64's.  centres0 [N][2] = (x, y), defocus0 [N], steps0 [2] = (step_xy, step_df) are DEVICE doubles;
 *     every decision is made on the device, nothing is read back: capturable, and a replay reads new images, seed and steps.  Every
 *     operation below is one rounded double operation.
 *   State: centres [N][2], defocus [N], steps, best.  `anchor` (0 <= anchor < N) is the gauge: that image's three parameters are
 *     never polled (a common shift picks another region; a common defocus offset leaves the loss unchanged at pad_periods = 0).
 *   loss(centres, defocus) = the worst loss (emd_exitwave_candidates_f64's) of the reconstruction of the crops around `centres`.
 *   Before round 0: loss0 = loss(seed); best = loss0, or +inf with EMD_SEARCH_NONFINITE if loss0 is not finite.
 *   Polls: the free images j = 0..N-2 are the k != anchor in ascending k; parameter p = axis (N - 1) + j, axis 0 = x, 1 = y,
 *     2 = defocus; candidate q = 2 p is the state with that one entry + step, q = 2 p + 1 with that entry - step (step_xy for axes
 *     0 and 1, step_df for axis 2); Q = 6 (N - 1).
 *   A round: the Q candidates in ceil(Q / C) chunks of at most C (1 <= C <= 64; a candidate's bits do not depend on C), each chunk a
 *     table kernel, one candidate crop and one candidate-stacks reconstruction; history_losses[r][q] = its worst loss;
 *     history_steps[r] = the steps the round polled with.  i = the first index of the smallest FINITE loss.  loss_i < best strictly:
 *     the state becomes candidate i, best = loss_i, moves += 1, history_choice[r] = i.  Otherwise both steps are multiplied by 0.5
 *     and history_choice[r] = -1.  No finite candidate: nothing changes, history_choice[r] = -2, EMD_SEARCH_NONFINITE is set.
 *   result_centres [N][2], result_defocus [N]; result [2] = (best, loss0); status [2] (ints) = (status bits, moves);
 *     history_losses [rounds][Q], history_choice [rounds] (ints), history_steps [rounds][2]; E [s][s] (may be NULL): the exit wave at
 *     the result, by one more reconstruction.  1 <= rounds <= 1024.
 *   Launches, with I iterations, R rounds, K = ceil(Q / C) and pad_periods == 0:  2 I + 11 + R (K (2 I + 8) + 1), + 2 I + 4 with E
 *     (init; the seed's table, crop and 2 I + 6 of a reconstruction with its losses; seed; per chunk the same 2 I + 8; one decision
 *     a round; finish; for E a table, a crop and 2 I + 2).  With pad_periods > 0 a reconstruction of n candidates is n (8 I + 2) + 2
 *     launches (one candidate without losses: 8 I) in place of 2 I + 6 (2 I + 2).
 *   The workspace is 16-byte aligned, as is E; arrays of doubles and status 8-byte; the images and history_choice 4-byte.  Outputs and
 *     the workspace may overlap neither one another nor the inputs. */
int emd_crop_candidates_f32(const float* images, int N, int S0, const double* centres_table, int C, int side, float pad_val, float* out,
                            emd_stream_t stream);
size_t emd_exitwave_candidate_stacks_workspace_bytes(int C, int N, int s, int pad_periods);
int emd_exitwave_candidate_stacks_f64(const float* images, int C, int N, int s, int pad_periods, const double* defocus_table,
                                      double wavelength, double px, double cs, int iterations, int flags, double* losses, double* worst,
                                      double* E, double* stack, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_exitwave_refine_workspace_bytes(int C, int N, int side, int pad_periods);
int emd_exitwave_refine_f64(const float* images, int N, int S0, int side, int pad_periods, float pad_val, const double* centres0,
                            const double* defocus0, const double* steps0, int anchor, int C, int rounds, double wavelength, double px,
                            double cs, int iterations, int flags, double* result_centres, double* result_defocus, double* result,
                            int* status, double* history_losses, int* history_choice, double* history_steps, double* E, void* workspace,
                            size_t workspace_bytes, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * 2-D FFT of any side (csrc/fft_any.hip): numpy.fft.fft2 / ifft2 / rfft2 and Fresnel propagation of [B][H][W]
 * with H and W independent, in double; complex arrays are interleaved (re, im) doubles.  The functions above keep their limit (a
 * square whose side is a power of two) and their bits; these are separate entry points.
 *
 * A side n is served if it is a power of two, 8 <= n <= 4096, or any n in 2 <= n <= 2048 (2 and 4 included).
 * Line transform of length n, forward, unnormalised: Y[k] = sum_j x[j] exp(-2 pi i j k / n).
 *   n a power of two, 8..4096: the radix-4 Stockham line of emd_cfft2_f64, the same bits.
 *   any other n: Bluestein.  M = max(8, the smallest power of two >= 2 n - 1) (M <= 4096).
 *       chirp   w[k] = exp(-i pi k^2 / n), evaluated as t = k^2 mod 2 n in integers, w = (cospi(t / n), -sinpi(t / n));
 *       a[j] = x[j] w[j] for j < n, 0 up to M;   b[j] = conj w[j] for 0 <= j < n, b[M - j] = conj w[j] for 1 <= j < n, 0 elsewhere;
 *       Bf = FFT_M(b);   Y[k] = w[k] IFFT_M(FFT_M(a) Bf)[k], k < n, with IFFT_M(v) = conj(FFT_M(conj v)) / M (1 / M is exact).
 *   inverse: x = conj(F(conj Y)) / n, one division per component.
 * emd_fft_any_line(n): the length of the line a transform of n occupies: n, M, or 0 for an n that is not served.
 * 2-D: lines along W first, stored transposed, then lines along H, stored transposed again (the order of emd_cfft2_f64); the
 *   inverse divides by W after the rows and by H after the columns.
 * cfft2_any: x [B][H][W] complex, or float32 (the real part) when x_is_real_f32 != 0; out [B][H][W].
 * rfft2_any: spec [B][H][W/2 + 1] = fft2(x)[..., :W/2 + 1], numpy.fft.rfft2's layout.  Every real row is transformed as a complex
 *   line of which W/2 + 1 elements are kept: twice the row work of emd_rfft2_f64's pair packing.
 * propagate_any: out[b] = ifft2(fft2(psi[b]) Hf(defocus[b])), no padding.  Hf at the unshifted indices (iy, ix): j = i for
 *   i < (n + 1) / 2, else i - n (numpy.fft.fftfreq); qy = (double)jy / ((double)H * px), qx = (double)jx / ((double)W * px);
 *   q2 = qy qy + qx qx;  t = lam df q2 + 0.5 lam^3 Cs q2 q2 (left to right, lam^3 = lam lam lam, every operation rounded on its
 *   own);  Hf = cospi(t) + i sinpi(t): emd_transfer_function_f64's expression on a rectangle.  Three launches after the tables':
 *   rows forward; columns forward, times Hf, inverse, in one kernel; rows inverse.  `defocus` is a DEVICE pointer, one per image.
 * The twiddles of M, the chirp and Bf are written into the workspace by kernels on every call, one set per distinct side: nothing
 * persists between calls and nothing is uploaded.  No atomics, fixed orders: bitwise reproducible, and an image's bits depend
 * neither on B nor on the other images.  0 <= B <= 65535 (B == 0 is a no-op).  The workspace is the caller's; it and the complex
 * arrays are 16-byte aligned (float32 images: 4-byte, defocus: 8-byte); outputs and the workspace may overlap neither one another
 * nor the inputs.  Launches only, on `stream`: capturable. */
int emd_fft_any_line(int n);
size_t emd_cfft2_any_workspace_bytes(int B, int H, int W);
int emd_cfft2_any_f64(const void* x, int x_is_real_f32, int B, int H, int W, int inverse, double* out, void* workspace,
                      size_t workspace_bytes, emd_stream_t stream);
size_t emd_rfft2_any_workspace_bytes(int B, int H, int W);
int emd_rfft2_any_f64(const float* x, int B, int H, int W, double* spec, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_propagate_any_workspace_bytes(int B, int H, int W);
int emd_propagate_any_f64(const void* psi, int psi_is_real_f32, int B, int H, int W, const double* defocus, double wavelength, double px,
                          double cs, double* out, void* workspace, size_t workspace_bytes, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Registration of a focal series (csrc/register.hip): what ewrec_class.py:140-177 does before it reconstructs --
 * the drift between consecutive images by phase correlation (:240-269), the chain of the shifts into one cropping centre per image,
 * the sub-pixel crop around each centre (:190-229).  cv2 is not available: the formulas below are the specification.  Every pointer
 * but the workspace sizes' is a DEVICE pointer; launches only, on `stream`, no host synchronisation, no upload: capturable; no
 * floating-point atomics, fixed orders: bitwise reproducible.
 *
 * Phase correlation, cv2.phaseCorrelate(a, b[, window]) restated.  Images float32 [S][S], S a power of two, 8 <= S <= 4096; all
 * arithmetic in double.
 *   window (EMD_PC_WINDOW), cv2.createHanningWindow's: w[i] = 0.5 (1 - cos(2 pi i / (S - 1))), evaluated as numpy's
 *       0.5 * (1 - cos(2 * pi * i / (S - 1))); the image is multiplied by sqrt(w[y] w[x]).  emd_hanning_window_f64 writes the same
 *       bits: w1 [S] and w2 [S][S] = sqrt(w[y] w[x]) (either may be NULL).
 *   P = F(a) conj F(b);  R = P / |P| where |P| > 0, else 0 (OpenCV adds an epsilon to the denominator instead);
 *   c = Re ifft2(R), normalised by 1 / S^2, viewed in fftshift order: c_s[y][x] = c[(y + S/2) mod S][(x + S/2) mod S].
 *   peak: the largest c_s; on a tie the first in row-major order of c_s.
 *   centroid: over rows and columns peak - 2 .. peak + 2 clipped to [0, S - 1] (not wrapped), in row-major order, in double:
 *       sv += v; sx += x v; sy += y v (every operation rounded on its own);  (cx, cy) = (sx / sv, sy / sv).
 *   shift = (S/2 - cx, S/2 - cy): if b is a displaced by +d, the shift is +d.  response = sv.  Where sv = 0 (images of zeros):
 *       shift = (0, 0), response = 0 (cv2: NaN).
 *   shifts [P][3] = (dx, dy, response), 1 <= P <= 64 pairs; surface: NULL, or [P][S][S] = c_s.  Pair p is (a[p], b[p]); with
 *   EMD_PC_CHAIN `a` holds P + 1 images, b is NULL, pair p is (a[p], a[p + 1]) and every image is transformed once.  Chain and pair
 *   mode give the same bits on the same pairs.  Four launches after the tables' (rows; columns with R formed in LDS between the forward
 *   and the inverse transform; rows back with the peak's partials; one wave per pair for the peak and the centroid).
 *   The workspace is 16-byte aligned, doubles 8-byte, images 4-byte.  The outputs and the workspace may overlap neither one another
 *   nor the inputs; a and b are only read and may share bytes (a == b is an autocorrelation).
 *
 * Centres: shifts [N - 1][3] of the pairs (k, k + 1) (the response is not read), 2 <= N <= 65, images of side S (1..4096):
 *   pos_0 = 0; pos_k = pos_{k-1} + shift_{k-1}; m = (sum_k pos_k, ascending from pos_0) / N; centre_k = (S / 2 + pos_k) - m, as
 *   (x, y) in centres [N][2].  (The reference's loop does not run as written, has one entry too few and returns S/2 + m - pos, which
 *   under the sign convention above moves the crop against the drift.)
 *
 * Crop: images [N][S][S] float32 (1 <= N <= 65535, 1 <= S <= 4096), 1 <= side <= S, out [N][side][side] float32.  Per image and axis
 *   x0 = cx - (double)side / 2; ix = floor(x0); fx = x0 - ix; then, every operation rounded on its own in double,
 *   out[r][c] = (float)((1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11)),  p_jk = image[iy + r + j][ix + c + k], or
 *   pad_val where that tap is outside the image.  (The reference weights the left tap with the fraction, which is not bilinear, and
 *   then returns the integer crop.) */
#define EMD_PC_WINDOW 1
#define EMD_PC_CHAIN 2
int emd_hanning_window_f64(int S, double* w1, double* w2, emd_stream_t stream);
size_t emd_phase_correlate_workspace_bytes(int P, int S, int flags);
int emd_phase_correlate_f64(const float* a, const float* b, int P, int S, int flags, double* shifts, double* surface, void* workspace,
                            size_t workspace_bytes, emd_stream_t stream);
int emd_stack_centres_f64(const double* shifts, int N, int S, double* centres, emd_stream_t stream);
int emd_crop_stack_f32(const float* images, int N, int S, const double* centres, int side, float pad_val, float* out,
                       emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Affine registration of a focal series by mutual information, and warping (csrc/affine.hip): what
 * misc_py/evolutionary_align.m (imregtform with imregconfig('multimodal'): Mattes mutual information on random samples under a (1+1)
 * evolutionary optimizer) and misc_py/warp_stack.m (the transforms chained onto the middle image, imwarp, the common rectangle) do.
 * MATLAB is not available: the formulas below are the specification.  Every pointer is a DEVICE pointer; launches only, on `stream`, no
 * host synchronisation, no upload: capturable; no floating-point atomics: two runs give the same bits.  Images are float32 [N][H][W],
 * 8 <= H, W <= 4096, not necessarily equal or powers of two.  All arithmetic is in double, every operation rounded on its own, every
 * expression evaluated left to right as written.
 *
 * Conventions.  Pixel coordinates are zero-based (x, y); c = ((W - 1) / 2, (H - 1) / 2); h = max(H, W) / 2; the normalised
 *   coordinates are u = (x - cx) / h, v = (y - cy) / h.  A transform T is 2 x 3 doubles, row-major, in normalised coordinates, and a PULL
 *   map: it takes a point of the fixed (output) frame to the point of the moving (input) frame that is sampled there,
 *       u' = (T00 u + T01 v) + T02;  v' = (T10 u + T11 v) + T12;  x' = u' h + cx;  y' = v' h + cy.
 *   The optimizer's six parameters are p = T - [I | 0].  In pixel coordinates the same map is the 3 x 3 matrix
 *   [T00 T01 (T02 h + cx - T00 cx - T01 cy); T10 T11 (T12 h + cy - T10 cx - T11 cy); 0 0 1] on column vectors.  MATLAB's tform.T (row
 *   vectors, the forward map from moving to fixed) is the transpose of the inverse of that matrix (one-based coordinates aside).
 *   MATLAB's optimizer scales its parameters internally; here the normalised coordinates do that: all six have the magnitude of a
 *   displacement in units of half the image.
 *
 * Warp: imwarp(img, T, 'OutputView', imref2d(size(img))) with linear interpolation.  T is [N][6], or [6] shared by all images
 *   (shared_T != 0).  ix = floor(x'), fx = x' - ix, likewise y;
 *       out = (float)((1 - fy) ((1 - fx) p00 + fx p01) + fy ((1 - fx) p10 + fx p11)),  p_jk = image[iy + j][ix + k]
 *   (emd_crop_stack_f32's arithmetic); a tap outside the image reads `fill`; where no tap is inside the output is `fill` itself; a
 *   coordinate that is not finite puts every tap outside.
 *
 * Samples: samples[i] = mulhi32(r_i, H W), r_i the word i % 4 of philox4x32_10 with counter (i / 4, 0, 0, 7) and key (seed lo, seed hi):
 *   pixel indices y W + x, drawn with replacement.
 *
 * Metric: Mattes mutual information of P pairs (fixed[p], moving[p]) under one candidate T[p] each.  fmin, fmax are the extrema of the
 *   whole fixed image, mmin, mmax of the whole moving image (exact, found on the device; NaN pixels are passed over).  samples == NULL
 *   and n == 0: every fixed pixel in row-major order; else n indices (an index >= H W is passed over).  Per sample at (x, y): f the
 *   fixed pixel; (x', y') as above; the sample counts iff 0 <= x' <= W - 1 and 0 <= y' <= H - 1 (false for a value that is not
 *   finite); m is the bilinear value of the moving image as in the warp, in double, with outside taps read as 0.  With pad = 2:
 *       bf = (fmax - fmin) / (bins - 2 pad);  tf = (f - fmin) / bf + pad;  jf = clip(floor(tf), pad, bins - pad - 1);  bm, tm, jm likewise from m;
 *       for d = -1, 0, 1, 2:  w = B3((jm + d) - tm);  hist[jf][jm + d] += rint(w 2^32)       (64-bit integers)
 *       B3(u), a = |u|:  a < 1: a2 = a a, a3 = a2 a, ((4 - 6 a2) + 3 a3) / 6;   a < 2: t = 2 - a, ((t t) t) / 6;   else 0.
 *   The histogram is a sum of integers: it does not depend on the order of the samples and is exact.  Value: n = sum hist; pf[j], pm[k]
 *   the row and column sums (integers); P = hist / n, pf / n, pm / n (each integer converted to double, then one division);
 *       MI = sum over the bins in row-major order of P log(P / (pf pm)), an empty bin adding 0, by one accumulator.
 *   MI = 0 and status EMD_MI_EMPTY if n = 0; MI = 0, a histogram of zeros and status EMD_MI_CONSTANT if fmax <= fmin or mmax <= mmin
 *   (or an extremum is infinite).  8 <= bins <= 64; 1 <= P <= 64.  hist (may be NULL) receives [P][bins][bins].
 *   Launches: two for the extrema, one for the histogram (a workgroup owns a run of samples and keeps the histogram in LDS,
 *   bins^2 x 8 bytes, with integer LDS atomics; G = min(ceil(n / 1024), 64) workgroups per pair store their histograms as partials in
 *   the workspace), one that sums the partials and forms the value, one workgroup per pair.
 *
 * Optimizer: the (1+1) evolution strategy of imregconfig('multimodal') on p, all P pairs in the same launches.  The state of a pair is
 *   EMD_AFFINE_STATE_DOUBLES doubles: x[6] at 0, A[6][6] at 6, the normal vector n[6] that made the child at 42, the child at 48, the
 *   parent's value f at 54, the last value at 55, and as 64-bit integers in the same array the number of evaluations done at 56, the
 *   number accepted at 57, the status at 58 (0, EMD_AFFINE_CONVERGED, EMD_AFFINE_DEGENERATE: an image is constant, f = 0;
 *   EMD_AFFINE_EXHAUSTED: the caller's variates have run out), sum hist of the last evaluation at 59; the rest is internal.
 *   flags: EMD_AFFINE_RESET starts from T0 [P][6] (NULL: the identity): x = T0 - [I | 0], A = initial_radius I, the counters at
 *   first_iteration and 0; EMD_AFFINE_NEXT_LEVEL keeps x and the counters and resets A and the status (the next level of a pyramid);
 *   0 continues.  Then `iterations` times two launches: the histogram launch evaluates the child (T = [I | 0] + child), and a step
 *   launch, one workgroup per pair, sums the partials, forms MI, and one thread does the rest.  The first evaluation after a reset is
 *   the parent itself and only sets f.  Otherwise, with t the number of evaluations done before:
 *       accept iff MI > f: then x = child, f = MI;  factor = growth on acceptance, else sqrt(sqrt(1 / growth)) (growth^(-1/4) in
 *       correctly rounded operations);  nn = sum n_j n_j;  d_i = sum_j A_ij n_j;  c = (factor - 1) / nn;  A_ij = A_ij + (c d_i) n_j
 *       (no update if nn = 0);  if sqrt(sum A_ij A_ij, row-major) < epsilon: status = EMD_AFFINE_CONVERGED, stop;
 *   then the next normals: n = variates[t][p][0..5] where variates != NULL ([variates_rows][P][6]; t >= variates_rows: status =
 *   EMD_AFFINE_EXHAUSTED), else by Box-Muller from Philox: for draw = 0, 1, 2 the words r0, r1 of philox4x32_10 with counter
 *   (t, p, draw, 8) and key (seed lo, seed hi); u1 = (r0 + 0.5) 2^-32, u2 = (r1 + 0.5) 2^-32; rad = sqrt(-2 log u1);
 *   n[2 draw] = rad cospi(2 u2), n[2 draw + 1] = rad sinpi(2 u2) (emd_affine_normals_f64 writes the same bits, [iterations][P][6] from
 *   iteration first_iteration on);  child_i = x_i + sum_j A_ij n_j.  Sums run j = 0..5 from the first product.
 *   A pair whose status is not 0 makes both launches return at once by a uniform branch: further iterations leave its state untouched.
 *   The extrema are found again by every call (two launches), so a captured block of iterations may be replayed on other images.
 *   The workspace is emd_mattes_mi_workspace_bytes(P, H, W, n, bins) for both the metric and the optimizer.
 *
 * Chain: T_pairs [N - 1][6], pair k being (fixed k, moving k + 1); M_k its 3 x 3 homogeneous form; C_middle = I;
 *   C_j = M_{j-1} C_{j-1} above the middle, C_j = inv(M_j) C_{j+1} below; (A B)_ik = (A_i0 B_0k + A_i1 B_1k) + A_i2 B_2k; the inverse of
 *   [a b c; d e f; 0 0 1] is, with det = a e - b d, [e/det, -b/det, (b f - c e)/det; -d/det, a/det, (c d - a f)/det; 0 0 1].  A pair
 *   transform that is singular (det = 0) or not finite gives NaNs from there outwards on either side of the middle, so the warp writes `fill`.  C is [N][6]: the pull
 *   map of image j onto the middle image's frame.  1 <= N <= 65.
 * Limits: warp_stack.m:112-150 applied to every image and intersected.  With D = inv(C_j) as above, the corners (0, 0), (W - 1, 0),
 *   (W - 1, H - 1), (0, H - 1) of image j land at  X = (D00 (x - cx) + D01 (y - cy)) + (D02 h + cx),  Y likewise; left = ceil(max(X1, X4)),
 *   right = floor(min(X2, X3)), top = ceil(max(Y1, Y2)), bottom = floor(min(Y3, Y4)); over all images the largest left and top and
 *   the smallest right and bottom, clamped to the image; limits = int32 (x0, y0, w, h) = (left, top, right - left + 1, bottom - top + 1),
 *   w and h not below 0; (0, 0, 0, 0) if a C_j is singular or not finite.  The identity gives (0, 0, W, H).
 *
 * Deviations from the reference: the pull-map convention and the normalised parameters (above); the fixed-point histogram (ITK adds
 *   doubles); warp_stack.m as committed does not run (its loop (mid-2):1 is empty, the right-hand images use left_trans, crop_limits
 *   reads an undefined image), and int32(L/2)+1 is not the middle for odd L: here middle is an argument (Python: N // 2); the corner
 *   box is the reference's heuristic, not the exact inscribed rectangle of a rotated image, and it intersects edges where the reference
 *   compares a width with an edge; imregtform's moment-based initialisation and its pyramid smoothing are not restated. */
#define EMD_MI_CONSTANT 1
#define EMD_MI_EMPTY 2
#define EMD_AFFINE_STATE_DOUBLES 64
#define EMD_AFFINE_CONVERGED 1
#define EMD_AFFINE_DEGENERATE 2
#define EMD_AFFINE_EXHAUSTED 4
#define EMD_AFFINE_RESET 1
#define EMD_AFFINE_NEXT_LEVEL 2
int emd_warp_affine_f32(const float* images, int N, int H, int W, const double* T, int shared_T, float fill, float* out,
                        emd_stream_t stream);
int emd_mi_samples_u32(int n, int H, int W, uint64_t seed, uint32_t* samples, emd_stream_t stream);
size_t emd_mattes_mi_workspace_bytes(int P, int H, int W, int n, int bins);
int emd_mattes_mi_f64(const float* fixed, const float* moving, int P, int H, int W, const double* T, const uint32_t* samples, int n,
                      int bins, double* mi, int* status, uint64_t* hist, void* workspace, size_t workspace_bytes, emd_stream_t stream);
int emd_affine_normals_f64(int iterations, int P, int first_iteration, uint64_t seed, double* normals, emd_stream_t stream);
int emd_affine_register_f64(const float* fixed, const float* moving, int P, int H, int W, const uint32_t* samples, int n, int bins,
                            double initial_radius, double growth, double epsilon, uint64_t seed, const double* variates,
                            int variates_rows, int flags, const double* T0, int first_iteration, int iterations, double* state,
                            void* workspace, size_t workspace_bytes, emd_stream_t stream);
int emd_affine_chain_f64(const double* T_pairs, int N, int middle, double* C, emd_stream_t stream);
int emd_affine_limits_i32(const double* C, int N, int H, int W, int* limits, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Exit wave and aberrations by gradient descent (csrc/psiart.hip): machine_learning/psi-art.py:97-130, :170-223,
 * :293-313, :334-348.  The reference does not run as committed; the formulas below are the specification.  Everything is double
 * precision; complex arrays are interleaved (re, im) doubles.  S a power of two, 8 <= S <= 2048 (4096 is refused: the column kernels
 * would spill registers); 1 <= N <= 64.  Every pointer but the workspace's size is a DEVICE pointer.
 *
 * Grid (spatial_frequencies): f[i] = (i < S/2 ? i : i - S) * (1.0 / (S * sampling)), as numpy.fft.fftfreq; kx[i][j] = f[i] (the row
 *     index), ky[i][j] = f[j];   theta = lam sqrt(kx kx + ky ky);   phi = atan2(ky, kx) (0 at the origin).
 * Parameters: EMD_PSIART_NPARAM = 27 doubles.  0..24, in the reference's all_symbols order: a22 phi22 a20 a33 phi33 a31 phi31 a44 phi44
 *     a42 phi42 a40 a55 phi55 a53 phi53 a51 phi51 a66 phi66 a64 phi64 a62 phi62 a60;  25: focal_spread D;  26: the raw defocus offset u.
 * CTF of image k (get_chi, get_temporal_envelope):  off = scale tanh(u / scale);   a20_k = a20 ramp_k + off;
 *     chi_k = (2 pi / lam) sum_n (1 / n) theta^n sum_m a_nm cos(m (phi - phi_nm)), the terms of get_chi (m = 0: no angle), a20 replaced
 *     by a20_k;   T = exp(-sign(D) (0.5 pi / lam D theta^2)^2);   C_k = exp(-i chi_k) T.  chi is reduced as t = chi / pi, formed
 *     without pi:  t_k = (2 / lam) sum' + a20_k theta^2 / lam  (sum': every term but a20's),  C_k = (cospi(t_k) - i sinpi(t_k)) T.
 * Forward:  psi = A (cos P + i sin P), A and P [S][S];   psi^ = fft2(psi);   b_k = ifft2(C_k psi^);   m_k = |b_k|.
 *     Targets r_k = sqrt(max(image_k, 0)) of the float32 images [N][S][S] (EMD_PSIART_AMPLITUDES: |image_k|).
 *     c_k = mean(r_k) / mean(m_k) with EMD_PSIART_NORMALISE, else 1;   p_k = c_k m_k;   loss_k = mean((p_k - r_k)^2), two-pass, fixed
 *     order;   L = sum_k w_k loss_k in ascending k.  losses [N + 1]: the N per image, then L.  pred (may be NULL) [N][S][S] = p_k.
 *     An all-zero wave with NORMALISE has mean(m_k) = 0: c_k is then inf or NaN and loss_k, L and pred are NaN, while every
 *     gradient is exactly 0 (G_b below is 0 everywhere), so nothing non-finite reaches A, P or the scalars.  It is not refused.
 * Reverse, n = S^2, d = p_k - r_k, M = mean(m_k):   g_m = w_k (2 c_k / n) (d - sum(d m_k) / (n M))  (the second term only with
 *     NORMALISE);   G_b = g_m b_k / |b_k|, 0 where |b_k| = 0;   F_k = fft2(G_b);   G_psi = sum_k ifft2(conj(C_k) F_k);
 *     dL/dA = cos P Re G_psi + sin P Im G_psi;   dL/dP = A (-sin P Re G_psi + cos P Im G_psi).
 *     With z_k = conj(F_k / n) C_k psi^, summed over the frequencies q and the images k:
 *     dL/da_nm = sum Im z_k (2 pi / lam) (1 / n) theta^n cos(m (phi - phi_nm));   dL/dphi_nm = sum Im z_k (2 pi / lam) (1 / n) theta^n
 *     a_nm m sin(m (phi - phi_nm));   dL/da20 = sum ramp_k Im z_k (pi / lam) theta^2;   dL/du = sech^2(u / scale) sum Im z_k (pi / lam)
 *     theta^2;   dL/dD = sum Re z_k (-2 |D| (0.5 pi theta^2 / lam)^2).   g_amp, g_phase [S][S], g_params [27] may be NULL; with none of
 *     them (and no step) the reverse launches are not made.
 * Step: tf.train.AdamOptimizer's form, t = step[0] + 1:  lr_t = rate sqrt(1 - beta2^t) / (1 - beta1^t);  m = beta1 m + (1 - beta1) g;
 *     v = beta2 v + (1 - beta2) g g;  x -= lr_t m / (sqrt(v) + epsilon);  step[0] = t.  rates [29]: A, P, then the 27 scalars; a rate
 *     of 0 leaves the parameter and its moments bitwise unchanged (a field with rate 0 is not written at all).
 * Deviations from the reference: the normalisation uses mean|b_k| against the mean of the root image (the reference: a complex mean
 *     against the mean of the intensity); the loss is on |b_k|; ramp (3 |k - middle| there) and the weights (its bootstrapping window)
 *     are arguments.  Not here: the spatial-coherence and aperture envelopes, the per-image affine transforms (their translation
 *     part: the emd_psiart_shift_* entry points below), padding.
 * No floating-point atomics, fixed summation orders: bitwise reproducible.  The workspace is the caller's and 16-byte aligned, arrays
 * of doubles 8-byte, the images and the step counter 4-byte; outputs and the workspace overlap nothing.  Launches only: capturable. */
#define EMD_PSIART_NPARAM 27
#define EMD_PSIART_NORMALISE 1  /* bits of `flags` */
#define EMD_PSIART_AMPLITUDES 2
int emd_psiart_ctf_f64(int S, int n, const double* params, const double* ramp, double wavelength, double sampling, double offset_scale,
                       double* C, emd_stream_t stream);
size_t emd_psiart_workspace_bytes(int N, int S);
int emd_psiart_loss_grad_f64(const float* images, int N, int S, const double* amp, const double* phase, const double* params,
                             const double* ramp, const double* weights, double wavelength, double sampling, double offset_scale, int flags,
                             double* losses, double* pred, double* g_amp, double* g_phase, double* g_params, void* workspace,
                             size_t workspace_bytes, emd_stream_t stream);
int emd_psiart_step_f64(const float* images, int N, int S, double* amp, double* phase, double* params, const double* ramp,
                        const double* weights, double wavelength, double sampling, double offset_scale, int flags, double* m_amp,
                        double* v_amp, double* m_phase, double* v_phase, double* m_params, double* v_params, int* step, const double* rates,
                        double beta1, double beta2, double epsilon, double* losses, double* pred, double* g_amp, double* g_phase,
                        double* g_params, void* workspace, size_t workspace_bytes, emd_stream_t stream);

/* The same fit with a trainable sub-pixel shift of every image: the translation part of the per-image transforms of
 * psi-art.py:229-266.  shifts [N][2] doubles, in pixels, along the first axis (the row index) then the second.  With the signed indices
 * i' = (i < S/2 ? i : i - S), j' likewise (numpy.fft.fftfreq(S) times S):
 *     t_k = (tbase + a20_k theta^2 / lam) + 2 (i' d0_k + j' d1_k) / S;   C_k = (cospi(t_k) - i sinpi(t_k)) T,
 * that is C_k times exp(-2 pi i (i' d0_k + j' d1_k) / S): prediction k is moved by (d0_k, d1_k) pixels, and a whole-pixel shift
 * (a, b) is numpy.roll(p_k, (a, b), (0, 1)).  The shift is CIRCULAR: what leaves on one side enters on the other, so a residual of
 * up to one pixel after cropping wraps one border line of the image into the loss.  Modulus, c_k, loss and weights are as above.
 * With all shifts 0 the argument of cospi / sinpi, and so every output, has the bits of the entry points without shifts.
 *     dL/dd0_k = sum_{i,j} Im z_k (2 pi i' / S);   dL/dd1_k = sum_{i,j} Im z_k (2 pi j' / S),  z_k formed with the shifted C_k: sums
 *     per image, in a fixed order (lanes, the four waves, the lines ascending).  g_shifts [N][2] may be NULL.
 * Step: Adam on the shifts with the same t and correction; shift_rates [N], one rate per image for both of its axes; a rate of 0 leaves
 *     that image's shift and its moments bitwise unchanged.  A translation of all images at once is a translation of the wave: keep one
 *     image (the middle one) at rate 0 as the gauge.  m_shifts, v_shifts [N][2].
 * emd_psiart_shift_workspace_bytes: the layout of emd_psiart_workspace_bytes, then partial_shift (S N 2 doubles).  The same refusals
 * as above, before any launch; ten launches a step; capturable, shifts and rates are read on the device. */
size_t emd_psiart_shift_workspace_bytes(int N, int S);
int emd_psiart_shift_loss_grad_f64(const float* images, int N, int S, const double* amp, const double* phase, const double* params,
                                   const double* shifts, const double* ramp, const double* weights, double wavelength, double sampling,
                                   double offset_scale, int flags, double* losses, double* pred, double* g_amp, double* g_phase,
                                   double* g_params, double* g_shifts, void* workspace, size_t workspace_bytes, emd_stream_t stream);
int emd_psiart_shift_step_f64(const float* images, int N, int S, double* amp, double* phase, double* params, double* shifts,
                              const double* ramp, const double* weights, double wavelength, double sampling, double offset_scale, int flags,
                              double* m_amp, double* v_amp, double* m_phase, double* v_phase, double* m_params, double* v_params,
                              double* m_shifts, double* v_shifts, int* step, const double* rates, const double* shift_rates, double beta1,
                              double beta2, double epsilon, double* losses, double* pred, double* g_amp, double* g_phase, double* g_params,
                              double* g_shifts, void* workspace, size_t workspace_bytes, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * cv2.resize for one-channel float32 (csrc/resample.hip, csrc/resize_taps.hpp): the reference's
 * load_image(addr, resizeSize), its random crops resized to the network's side (modified_Xception.py:976-982) and
 * EWREC.resize_stack (ewrec_class.py:236-238).  OpenCV is not used: the arithmetic is restated from these rules.
 *
 * interpolation: cv2's codes, EMD_RESIZE_NEAREST 0, EMD_RESIZE_LINEAR 1, EMD_RESIZE_CUBIC 2, EMD_RESIZE_AREA 3.  For one axis with
 * n_in source and n_out destination samples, inv = (double)n_out / n_in and scale = 1.0 / inv (cv2's order; not n_in / n_out).
 * Everything is IEEE double, every operation rounding on its own, except where a rounding to float32 is written out: those are
 * cv2's own and decide which pixels are read.  For destination sample d:
 *   NEAREST   s = min(floor(d * scale), n_in - 1); one tap, weight 1.
 *   LINEAR    f = (float)((d + 0.5) * scale - 0.5);  s = floor(f);  f = (float)(f - s);  s < 0: s = 0, f = 0;  s >= n_in - 1:
 *             s = n_in - 1, f = 0.  Taps s and min(s + 1, n_in - 1), weights 1 - f and f.
 *   CUBIC     f and s as LINEAR without the clamps; taps s - 1 .. s + 2, each index clamped into 0 .. n_in - 1; with A = -0.75:
 *             c0 = ((A (f + 1) - 5 A) (f + 1) + 8 A) (f + 1) - 4 A;   c1 = ((A + 2) f - (A + 3)) f f + 1;
 *             c2 = ((A + 2) (1 - f) - (A + 3)) (1 - f) (1 - f) + 1;   c3 = 1 - c0 - c1 - c2   (in double from the float32 f: cv2 forms
 *             them in float32, a deviation of a few 1e-8).
 *   AREA      scale >= 1 on BOTH axes -- true area:
 *               whole ratios, i = (int)scale with |scale - i| < DBL_EPSILON on both axes: the mean of the i_y x i_x block, the sum
 *               formed in double, divided by the block's pixel count, rounded once;
 *               otherwise, per axis:  f1 = d * scale;  f2 = f1 + scale;  cell = min(scale, n_in - f1);  s1 = ceil(f1);
 *               s2 = min(floor(f2), n_in - 1);  s1 = min(s1, s2);  if s1 - f1 > 1e-3, pixel s1 - 1 has weight (float)((s1 - f1) / cell);
 *               pixels s1 .. s2 - 1 have (float)(1.0 / cell);  if f2 - s2 > 1e-3, pixel s2 has
 *               (float)(min(min(f2 - s2, 1.0), cell) / cell).  The 1e-3 rule drops slivers, so a sample's weights need not sum to 1
 *               (2001 -> 2000: sample 0 sums to 1 / 1.0005): cv2's behaviour, kept.
 *             an axis enlarges -- cv2's emulated area, on both axes:  s = floor(d * scale);  f = (float)((d + 1) - (s + 1) * inv);
 *               f = f <= 0 ? 0 : (float)(f - floor(f));  then LINEAR's two clamps and pair of taps.  A whole-ratio enlargement is
 *               nearest neighbour.
 * y[r][c] = sum_j beta_j sum_i alpha_i x[sy_j][sx_i]: a source row's columns first, rows ascending, in double, rounded to float32
 * once (cv2 accumulates in float32, a horizontal and then a vertical pass: a deviation at float32 rounding level).  Where the columns a
 * tile of 64 output columns reads span more than 264 source columns (ratios above 4), a row's sum is formed per 264-column segment and
 * each part is weighted and added on its own: a fixed order, different in the last bits of the double only.  Equal sizes return the
 * source bit for bit in every mode (the weights are exactly 0 and 1), as does NEAREST always -- but for -0, which comes out as +0.
 * Non-finite input is the caller's problem.
 *
 * No atomics, no workspace, no host synchronisation, one launch: capturable and bitwise reproducible, and an image's result does not
 * depend on B. */
#define EMD_RESIZE_NEAREST 0
#define EMD_RESIZE_LINEAR 1
#define EMD_RESIZE_CUBIC 2
#define EMD_RESIZE_AREA 3
/* HOST only: the tap description of every destination sample along one axis, from the same code the kernel calls (the one copy of
 * the arithmetic).  other_in -> other_out are the sizes of the other axis (the area rule looks at both).  Sample d has count[d] taps;
 * tap k reads source index min(max(first[d] + k, 0), n_in - 1) with weight
 *     k == 0 ? weights[d][0] : k == count[d] - 1 ? weights[d][3] : k == 1 ? weights[d][1] : weights[d][2]
 * (first, count: [n_out]; weights: [n_out][4]).  *block is 0, or i where this axis takes the whole-ratio area form: the weights are
 * then 1 and the 2-D sum is divided by the block's pixel count.  1 <= n_in, other_in <= 32768, 1 <= n_out, other_out <= 8192. */
int emd_resize_taps(int interpolation, int n_in, int n_out, int other_in, int other_out, int* first, int* count, double* weights,
                    int* block);
/* y[b] ([B,h,w], contiguous) = cv2.resize of image b (H x W at x + b * image_stride, rows row_stride floats apart) to h x w.
 * boxes_dev: NULL for the whole image, or DEVICE int32 [B][4] = (x0, y0, bw, bh): image b's source is that rectangle, the sizes and
 * the area rule taken per image on the device; a box is clamped into the image whatever it holds (x0 into 0 .. W - 1, bw into
 * 1 .. W - x0, likewise y), so no address leaves the image.  1 <= H, W <= 32768, 1 <= h, w <= 8192, row_stride >= W,
 * 0 <= B <= 65535 (B == 0 is a no-op).  y may not overlap x. */
int emd_resize_f32(const float* x, long image_stride, int row_stride, int B, int H, int W, const int* boxes_dev, float* y, int h, int w,
                   int interpolation, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Autofocus (csrc/focus.hip): the arithmetic of em_env/fresnel_env.py:163-179 (fresnel_quantifier), :188-208
 * (get_optimal_z) and misc_py/entropy.py:36-53 (image_entropy).  OpenCV is not used: the Laplacian is restated from its rules, not
 * run against OpenCV (its own summation order is not known here).  Images are float32 [B,H,W], contiguous.
 *
 * Laplacian: cv2.Laplacian(x, CV_32F, ksize) with BORDER_REFLECT_101 (index -1 -> 1, n -> n - 2), scale 1, delta 0, in float32, every
 *   operation rounding on its own, in this order (u, d, l, r the four neighbours, ul .. dr the diagonal ones, c the centre):
 *     ksize 1  [0 1 0; 1 -4 1; 0 1 0]:   ((u + d) + (l + r)) - 4 c
 *     ksize 3  [2 0 2; 0 -8 0; 2 0 2]:   2 ((ul + ur) + (dl + dr)) - 8 c
 *   2 <= H, W <= 32768.  One launch; y may not overlap x.
 * Moments: out [B][EMD_NFOCUS] doubles of the Laplacian L above (never written to memory):
 *     0  mean_L = sum L / (H W)            1  n = #S, S = {L : (double)L >= mean_L} with rectify, every L without
 *     2  mean_S = sum S / n                3  m2 = sum (s - mean_S)^2 / n         4  m4 = sum (s - mean_S)^4 / n
 *     5  m4 / (m2 m2) - 3: scipy.stats.kurtosis with its defaults (Fisher, biased), the reference's fresnel_quantifier
 *   Two-pass in double, fixed order: three reads of x with rectify (mean_L; n and mean_S; the moments), two without.  Every term
 *   ((s - mean_S), its square, the square's square) is rounded to double on its own; the four sums are carried as pairs hi + lo of
 *   doubles (two-sum) and rounded once at the end, so each is the exactly rounded sum of its terms (math.fsum's) but for ties within
 *   about n 2^-104, and the cancellation of column 5 amplifies no summation error.  L must be finite.  A constant image has L = 0:
 *   m2 = m4 = 0, column 5 NaN, as scipy.  Deviation: the reference's threshold is numpy's float32 pairwise mean of L; here it is the
 *   double mean.
 * Histogram: numpy.histogram(x, bins, range=(0, 1)) as int64 [B][bins], bins a power of two 2..4096: bin floor(x bins) for
 *   0 <= x < 1, x == 1 in the last bin, everything else (NaN included) dropped; the product is exact, so no rounding case exists.
 *   normalize == 1 bins t = 0.15 (x - mean) / std + 0.5 instead (entropy.py:48-49), mean and the population std the image's own,
 *   two-pass in double; t = ((0.15 (x - mean)) / std) + 0.5 in double, each operation rounding on its own (deviation: the reference
 *   evaluates t in float32).  A constant image has std = 0: nothing is counted.  Integer LDS atomics per workgroup, integer global
 *   adds (exact, so their order does not matter); counts is zeroed by a memset node first.  1 <= H, W <= 32768.  The workspace is
 *   needed with normalize only (emd_histogram01_workspace_bytes is 0 otherwise, and workspace may be NULL).
 * Entropy: scipy.stats.entropy(counts + eps, base=2) per row: p = (c + eps) / sum (c + eps); (sum -p log p) / log 2, fixed order.
 * Spline: z [N] doubles, strictly increasing (not checked: device data), scores [B][N], 4 <= N <= 256, 1 <= interp_factor <= 4096.
 *   The interpolating cubic spline with not-a-knot end conditions (scipy's InterpolatedUnivariateSpline(z, s), k = 3) is evaluated on
 *   numpy.linspace(z[0], z[N-1], G), G = interp_factor N: grid[i] = (i * step) + z[0] with two roundings, step = (z[N-1] - z[0]) /
 *   (G - 1), grid[G-1] = z[N-1] exactly.  index[b] = the first i with the smallest value (numpy.argmin; values must be finite),
 *   zbest[b] = grid[index[b]], curve[b][i] the values; curve and index may be NULL.  One workgroup per series.
 *
 * No floating-point atomics, no host synchronisation, launches (and the histogram's memset) only: capturable, bitwise reproducible, and
 * an image's results do not depend on B.  Workspaces are the caller's and 16-byte aligned; outputs and workspaces overlap nothing.
 * 0 <= B <= 65535 (B == 0 is a no-op). */
#define EMD_NFOCUS 6
int emd_laplacian_f32(const float* x, int B, int H, int W, int ksize, float* y, emd_stream_t stream);
size_t emd_laplacian_moments_workspace_bytes(int B, int H, int W);
int emd_laplacian_moments_f64(const float* x, int B, int H, int W, int ksize, int rectify, double* out, void* workspace,
                              size_t workspace_bytes, emd_stream_t stream);
size_t emd_histogram01_workspace_bytes(int B, int H, int W, int normalize);
int emd_histogram01_i64(const float* x, int B, int H, int W, int bins, int normalize, int64_t* counts, void* workspace,
                        size_t workspace_bytes, emd_stream_t stream);
int emd_hist_entropy_f64(const int64_t* counts, int B, int bins, double eps, double* entropy, emd_stream_t stream);
int emd_spline_argmin_f64(const double* z, const double* scores, int B, int N, int interp_factor, double* zbest, double* curve,
                          int64_t* index, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dose series (csrc/dose.hip): the arithmetic of misc_py/lq_img_gen-backup.py:6-91 (lq_chunks_gen, record_lq,
 * lq_img_gen) -- a micrograph as an unnormalised probability density, a fixed number of electrons thrown at it through its
 * cumulative sum -- in integers, so that every output is exact.  Images are float32 [B,H,W], contiguous; n = H W.
 *
 * Weights: a pixel that is not finite or <= 0 weighs 0; m = the largest remaining pixel;
 *     q[i] = rint(double(x[i]) / double(m) * 2^32)     (IEEE double division and multiply, round half to even; 0 .. 2^32)
 *   status[b] (may be NULL): EMD_DOSE_EMPTY when no pixel is positive (every q is 0 and every count stays 0), EMD_DOSE_SANITIZED when
 *   a pixel was zeroed for being negative, infinite or NaN (-0 is a zero).  |q[i] / 2^32 - x[i] / m| <= 2^-33 + 2^-53: a pixel below
 *   m 2^-33 gets no electrons.  The weights are never stored.
 * CDF: cdf[b][i] = q[0] + ... + q[i] in row-major order, inclusive, int64; T = cdf[b][n-1] <= 2^62.  Separate launches, none waits
 *   for another workgroup: the maximum (one integer atomicMax per workgroup on the float's bits), a sum per tile of EMD_DOSE_TILE
 *   pixels, a scan of those by one workgroup per image, the scan inside the tiles.  Workspace: emd_dose_workspace_bytes.
 * Draws: draw d of image b comes from philox4x32_10({j lo, j hi, first_image + b, 9}, {seed lo, seed hi}) = (x, y, z, w) with
 *   j = d >> 1: r = x 2^32 | y for even d, z 2^32 | w for odd d;  t = (r T) >> 64 (the high half of the 128-bit product, so t < T);
 *   the electron lands in pixel p = #{i : cdf[i] <= t} (numpy.searchsorted(cdf, t, side="right")): a zero-weight pixel is never hit.
 *   bounds: a HOST array of L + 1 draw indices, not descending, bounds[0] >= 0, bounds[L] - bounds[0] < 2^31,
 *   1 <= L <= EMD_DOSE_MAX_LEVELS; draw d in [bounds[k], bounds[k+1]) adds 1 to planes[b][k][p] (int32 [B][L][H][W]).  The entry point
 *   ADDS to what the planes hold: the caller zeroes them (a memset), or extends a series by a later call whose bounds[0] is where
 *   the last one stopped -- the draws [0, D) are the same electrons however they are split into calls or levels.  One launch,
 *   grid-stride over the Philox calls, one no-return integer atomicAdd per electron; no draw, target or index is written to memory.
 *   A table of at most EMD_DOSE_COARSE values of the CDF, one every ceil(n / EMD_DOSE_COARSE) pixels rounded up to a multiple of 16
 *   (the tile ends where the image has EMD_DOSE_COARSE tiles), is staged in LDS once per workgroup and searched there; the pixels
 *   between two entries are searched in global memory.  An image of more than EMD_DOSE_COARSE tiles has several tiles per table entry
 *   and a correspondingly longer second search; it is not refused.
 *   first_image + B <= 2^32.
 * Cumulate: plane k becomes the sum of the planes 0 .. k, in place, so that it holds every draw below bounds[k+1]; minmax[b][k] =
 *   {min, max} of that plane (int32 [B][L][2]; integer atomics on words that a small launch sets first).  Counts must not be negative.  L = 1 leaves the plane as it is.
 * Rescale (record_lq, :30-35), per plane with that min and max: EMD_DOSE_UINT16  out = (int32) trunc(65535.0 * (c - min) / (max - min)),
 *   product and quotient in double as numpy forms them; EMD_DOSE_UNIT  out = (float32)((c - min) / (max - min)), the quotient in
 *   double, rounded once.  Where max == min the reference divides by zero; here the plane is all 0.  out: [B][L][H][W], 4 bytes an
 *   element either way.
 *
 * Deviations from the reference: its walk along the sorted uniforms advances at most one pixel per draw (:21-26), so a draw that skips
 * a whole low-weight pixel is booked to the wrong pixel -- here the lookup is the inverse CDF; it normalises the cumulative sum in
 * floating point -- here the comparison is scaled by T in integers; it reseeds numpy from numpy per chunk -- here one Philox stream per
 * image.
 *
 * No floating-point atomics, no host synchronisation, launches only: capturable on one stream, bitwise reproducible, and an
 * image's result does not depend on B.  Every argument is checked before any launch.  0 <= B <= 65535 (B == 0 is a no-op),
 * 2 <= H, W <= 32768, H W <= 2^30.  The workspace is the caller's, 16-byte aligned; cdf 8-byte; outputs and the workspace overlap nothing. */
#define EMD_DOSE_EMPTY 1
#define EMD_DOSE_SANITIZED 2
#define EMD_DOSE_UNIT 0
#define EMD_DOSE_UINT16 1
#define EMD_DOSE_TILE 2048
#define EMD_DOSE_COARSE 2048
#define EMD_DOSE_MAX_LEVELS 32
size_t emd_dose_workspace_bytes(int B, int H, int W);
int emd_dose_cdf_i64(const float* x, int B, int H, int W, int64_t* cdf, int* status, void* workspace, size_t workspace_bytes,
                     emd_stream_t stream);
int emd_dose_draw_i32(const int64_t* cdf, int B, int H, int W, unsigned long long seed, unsigned long long first_image,
                      const int64_t* bounds_host, int L, int* planes, emd_stream_t stream);
int emd_dose_cumulate_i32(int* planes, int B, int L, int H, int W, int* minmax, emd_stream_t stream);
int emd_dose_rescale(const int* planes, const int* minmax, int B, int L, int H, int W, int mode, void* out, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Dataset diversity (csrc/diversity.hip): the arithmetic of misc_py/img_stats.py -- for every image the matrix of
 * squared Euclidean distances between its rows (the script's `gram`), and for a pair of images the mean squared difference of their
 * two matrices -- restated from the formulas.  Images are float32 [B,H,W], contiguous; rows are the points.
 *
 * Row norms: n[b][i] = sum_k x[b][i][k]^2 in double (every square is exact).  One wave per row: lane l adds the columns l, l + 64, ...
 *   in ascending order, then the 64 lanes are added as an xor butterfly (offsets 32, 16, .., 1).  nonfinite[b] (int32) = the number of
 *   pixels of image b that are NaN or +-inf, from the same read (integer adds onto a word that a small launch zeroes).
 * Products: G[i][j] = sum_k x[i][k] x[j][k] on v_mfma_f32_32x32x2_f32, whose result is bit for bit the float32 fmaf chain over k in
 *   ascending order.  A chain is at most EMD_DIVERSITY_CHAIN = 256 columns long (columns [256 c, 256 c + 256) of x); at its end the
 *   float32 accumulators are added, in float32, to a float32 running total and cleared.  (One unbroken chain over W = 2048 lies
 *   4.2 - 4.6 x further from the float64 product than numpy's float32 dot; chains of 256 lie 0.54 - 0.65 x as far.)  Columns >= W and
 *   rows >= H enter as zeros and are never read.
 * Distances (emd_row_distances_f32): D[b][i][j] = (float)((n_i + n_j) - 2 (double)G[i][j]), float32 [B][H][H].  Only the tiles of
 *   EMD_DIVERSITY_TILE = 128 rows and columns with tj >= ti are computed; D[j][i] is the same float, so D equals its transpose as
 *   bits.  The diagonal is whatever the arithmetic leaves (zero but for rounding).  H <= 4096.
 * Pair statistic (emd_gram_ssd_f64): for the pair (a, b) the chains of the two images run in separate accumulators; at a chain's
 *   end (acc_a - acc_b) is added in float32 to one running total Gd.  E[i][j] = (dn_i + dn_j) - 2 (double)Gd[i][j] with
 *   dn = n_a - n_b in double; ssd = (sum_ij E[i][j]^2) / H^2.  None of the four H x H matrices is written.  The sum: each lane adds
 *   E^2 over its own accumulators in double in a fixed order, then the wave (butterfly), then the four waves in order; a tile with
 *   tj > ti counts twice (E is symmetric); a wave per pair adds the tile sums (lane l the tiles l, l + 64, ..; butterfly) and divides
 *   by (double)H (double)H.  Hence ssd(a, a) == 0.0 exactly, ssd(a, b) and ssd(b, a) are equal as bits, and a pair's value depends
 *   neither on the other pairs nor on B.  H <= 8192.
 * Pair list: pairs is int32 [P][2], DEVICE memory, indices into the one resident stack x [B]; every image is normed once however
 *   many pairs name it.  status[p]: EMD_DIVERSITY_OK; EMD_DIVERSITY_NONFINITE, a named image has a non-finite pixel (the reference
 *   skips it); EMD_DIVERSITY_BAD_INDEX, an index outside [0, B).  For a status != 0 ssd[p] is NaN and nothing is read through a bad
 *   index.  Pairs and images may be replaced between replays of a captured graph.
 *
 * No floating-point atomics, no host synchronisation, launches only: capturable on one stream and bitwise
 * reproducible.  Every argument is checked before any launch: 0 <= B <= 65535, 1 <= W <= 32768, 1 <= H <= the limit
 * above (8192 for the norms), 0 <= P <= 2^20 and P * T (T + 1) / 2 < 2^31 with T = ceil(H / 128); B == 0 or P == 0 is a no-op.  The
 * workspace is the caller's, 16-byte aligned, its size from the _workspace_bytes functions (0 for arguments out of range); outputs and
 * the workspace overlap nothing.  EMD_DIVERSITY_TILE_K = 32 columns are staged in LDS at a time. */
#define EMD_DIVERSITY_TILE 128
#define EMD_DIVERSITY_TILE_K 32
#define EMD_DIVERSITY_CHAIN 256
#define EMD_DIVERSITY_OK 0
#define EMD_DIVERSITY_NONFINITE 1
#define EMD_DIVERSITY_BAD_INDEX 2
int emd_row_sq_norms_f64(const float* x, int B, int H, int W, double* norms, int* nonfinite, emd_stream_t stream);
size_t emd_row_distances_workspace_bytes(int B, int H, int W);
int emd_row_distances_f32(const float* x, int B, int H, int W, float* D, void* workspace, size_t workspace_bytes, emd_stream_t stream);
size_t emd_gram_ssd_workspace_bytes(int B, int H, int W, int P);
int emd_gram_ssd_f64(const float* x, int B, int H, int W, const int* pairs, int P, double* ssd, int* status, void* workspace,
                     size_t workspace_bytes, emd_stream_t stream);

/* ------------------------------------------------------------------------------------------------
 * Host utility (no GPU): CRC-32C (Castagnoli) of a HOST buffer, continuing from `crc` (0 to start).
 * Used by the TFRecord reader (emdenoise.input_pipeline) for the container that
 * misc_py/TFRecord_creator.py:57-85 writes with tf.python_io.TFRecordWriter. */
uint32_t emd_crc32c(const void* data_host, size_t n, uint32_t crc);

#ifdef __cplusplus
}
#endif
#endif /* EMDENOISE_H */
