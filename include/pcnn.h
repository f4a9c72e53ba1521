/* libpcnn - MI355X (gfx950) native kernels for the poisson_CNN hot path.  C-ABI drop-in boundary.
 *
 * The reference (aligirayhanozbay/poisson_CNN) has no FFI boundary of its own: every FLOP of its hot path runs
 * inside TensorFlow ops called from Python.  Each entry point below therefore names the TensorFlow op (and the
 * reference call site, path:line relative to poisson_CNN/) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes stub a maintainer of the reference would add.
 *
 * Conventions
 *  - All tensors are float32, device memory, NHWC ("channels innermost").  A tensor argument is a base pointer
 *    plus an explicit channel stride `ld*` (floats between consecutive pixels), so a kernel can read/write a
 *    channel slice of a wider buffer (this is how tf.concat(axis=1), models/Homogeneous_Poisson_NN_Legacy.py:224,
 *    is realised without a copy).
 *  - The caller owns every tensor and every workspace that appears as an argument.  The handle owns three scratch regions it grows on demand
 *    (hipMalloc on first use, freed by pcnn_destroy): the packed-filter scratch of the direct convolutions (KBs), the x-interpolated rows of the
 *    two-pass resize, and the SPECTRAL WORKSPACE of the tiled spectral convolutions - tables, the filter spectrum and the tile spectra of the
 *    launch in flight, up to ~14 GB for an 8 x 1024^2 x 32-channel layer.  pcnn_set_workspace_limit caps the latter (the route then runs in
 *    smaller tile chunks); growing it synchronises the stream, so a training loop reaches its high-water mark in the first step.
 *  - Every call is asynchronous on the handle's stream and returns 0 on success, non-zero on error
 *    (pcnn_last_error(handle) gives the message).  No exceptions cross the boundary.
 *  - One handle per (thread, device, stream).
 *  - The recurrent layers of models/Dirichlet_BC_RNN.py are the pcnn_rnn_* calls at the end of this header: one launch per layer and direction
 *    for the whole sequence; their time-parallel products are pcnn_wide_conv2d_* calls.
 *  - Environment variables read by the library are DEVELOPER switches for A/B timing and tests, not part of the interface; each is validated
 *    where it is read (an invalid value keeps the default): PCNN_MATH, PCNN_SPECTRAL, PCNN_SPEC_T (same as the pcnn_set_* calls),
 *    PCNN_SPEC_XFORM (transform kernels of the spectral route: "fft" in-register vector-ALU FFT, "mfma" DFT-as-GEMM), PCNN_SPEC_CHUNK (a size),
 *    PCNN_FWD64_RADIX, PCNN_GROUPED_VALU, PCNN_RCCL_LIBRARY / PCNN_ROCFFT_LIBRARY (a path for dlopen).
 */
#ifndef PCNN_H
#define PCNN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct pcnn_handle_s* pcnn_handle;

enum { PCNN_PAD_CONSTANT = 0, PCNN_PAD_SYMMETRIC = 1, PCNN_PAD_REFLECT = 2 };   /* tf.pad modes */
enum { PCNN_ACT_LINEAR = 0, PCNN_ACT_LEAKY_RELU = 1, PCNN_ACT_TANH = 2, PCNN_ACT_RELU = 3 };
enum { PCNN_POOL_AVERAGE = 0, PCNN_POOL_MAX = 1 };
enum { PCNN_RESIZE_NEAREST = 0, PCNN_RESIZE_BILINEAR = 1, PCNN_RESIZE_BICUBIC = 2,
       PCNN_RESIZE_BICUBIC_LEGACY_ALIGN_CORNERS = 3 /* tf.compat.v1 resize_images(align_corners=True), dataset/utils/image_resize.py:20 */ };

int pcnn_create(int device, void* hip_stream, pcnn_handle* out);
int pcnn_destroy(pcnn_handle h);
int pcnn_set_stream(pcnn_handle h, void* hip_stream);
int pcnn_sync(pcnn_handle h);
const char* pcnn_last_error(pcnn_handle h);
int pcnn_version(void);
/* CRC-32C of a host buffer (continue from `crc`, 0 to start): the checksum of TensorFlow TensorBundle checkpoints
 * (train/utils.py:10-29 loads them; poisson_cnn_amd/tf_checkpoint.py reads and writes the format).  Host only. */
uint32_t pcnn_crc32c(const void* data, size_t n, uint32_t crc);

/* Data-parallel collective: what tf.distribute.MirroredStrategy does under `with dist_strategy.scope()`
 * (train/hpnn_legacy_train.py:37) - ONE sum all-reduce of the flat gradient bucket per optimizer step - over RCCL / xGMI, on the handle's
 * stream.  RCCL is loaded at the first call (dlopen); rendezvous is the caller's: rank 0 obtains the 128-byte id and ships it to the
 * other ranks over whatever channel the host program has, then every rank (one process per GPU, one handle) calls pcnn_comm_init.
 * pcnn_allreduce / pcnn_broadcast are in place, asynchronous, fp32. */
#define PCNN_UNIQUE_ID_BYTES 128
/* host-only probe (no handle, no GPU): 0 when RCCL can be bound, else 1 with the loader's message in `why`.  The environment variable
 * PCNN_RCCL_LIBRARY names the one library file to try instead of the default search (librccl.so.1, librccl.so, /opt/rocm/lib). */
int pcnn_collective_available(char* why, size_t why_bytes);
int pcnn_comm_unique_id(pcnn_handle h, void* id_out);
int pcnn_comm_init(pcnn_handle h, const void* id, int rank, int world_size);
int pcnn_comm_destroy(pcnn_handle h);
int pcnn_allreduce(pcnn_handle h, float* buf, size_t count);
int pcnn_broadcast(pcnn_handle h, float* buf, size_t count, int root);

/* Arithmetic of the convolution GEMMs.
 *   PCNN_MATH_FP32      (default): v_mfma_f32_32x32x2_f32, exact fp32 products, fp32 accumulate.
 *   PCNN_MATH_SPLIT_F16 : every fp32 operand is split into two fp16 halves (hi + lo, 22 significant bits, per-tile power-of-two
 *                         scaling) and a*b is accumulated in fp32 as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16: 5.3x fewer
 *                         matrix-pipe cycles at an accuracy that is measured to be BETTER than the fp32 fmaf chain
 *                         (tools/split_f16_test.hip: 5.4e-7 vs 1.5e-6 rel-L2 against fp64 at K = 7200). */
enum { PCNN_MATH_FP32 = 0, PCNN_MATH_SPLIT_F16 = 1 };
int pcnn_set_math_mode(pcnn_handle h, int mode);
int pcnn_get_math_mode(pcnn_handle h);

/* Algorithm of pcnn_conv2d_fwd / pcnn_conv2d_wgrad for wide filters (replaces the same tf.nn.conv2d / backprop-filter calls):
 *   tiled spectral convolution - overlap-save on 32 x 32 tiles (64 x 64 for 11..15 taps: csrc/spectral64.hip), the DFT applied as fp32 MFMA matrix products, per-frequency channel
 *   mixing, inverse transform fused with the conv epilogue (csrc/spectral_conv.hip).  Exact fp32 products and accumulation like the
 *   direct kernel, ~k*k/25 times fewer of them.  PCNN_SPECTRAL_AUTO (default; environment PCNN_SPECTRAL=-1|0|1): a cost model picks the
 *   route per layer and math mode; _OFF: always the direct implicit GEMM; _FORCE: spectral whenever the shape allows
 *   (kh, kw <= 15, Cin <= 64, Cout <= 32).  The handle owns the workspace (tile spectra), grown on demand. */
enum { PCNN_SPECTRAL_AUTO = -1, PCNN_SPECTRAL_OFF = 0, PCNN_SPECTRAL_FORCE = 1 };
int pcnn_set_spectral_mode(pcnn_handle h, int mode);
int pcnn_get_spectral_mode(pcnn_handle h);
/* Tile size of the spectral route: 0 (default; environment PCNN_SPEC_T) = per layer - 64 x 64 tiles for 13..15 taps on images of >= 36 such
 * tiles and for 11..12 taps on images of >= 256 such tiles, 32 x 32 otherwise (decided on ONE image: a sample's arithmetic never depends on
 * its batch neighbours); 32 / 64 = that size wherever the layer allows it (64: 9..15 taps, more than 16 channels on one side). */
int pcnn_set_spectral_tile(pcnn_handle h, int tile);
int pcnn_get_spectral_tile(pcnn_handle h);
/* Transform kernels of the spectral route (same spectrum layout, same arithmetic class - exact fp32 -, results agree to ~1e-7):
 *   PCNN_XFORM_MFMA: the DFT as a GEMM on the matrix cores (v_mfma_f32_32x32x2_f32; csrc/spectral_conv.hip, spectral64.hip);
 *   PCNN_XFORM_FFT:  in-register FFTs on the vector ALUs, lane = channel (csrc/spectral_fft.hip, fft_regs.h): fp32 MFMA has no rate advantage
 *                    over the vector ALUs on gfx950, so the FFT needs ~9x fewer issue cycles, half the registers and twice the waves per CU.
 * Default: PCNN_XFORM_FFT (measured 20-30 % faster per layer at 8 x 1024^2, profiles/r05_probe_xform*.txt); environment PCNN_SPEC_XFORM=fft|mfma sets the
 * default of new handles. */
enum { PCNN_XFORM_MFMA = 0, PCNN_XFORM_FFT = 1 };
int pcnn_set_spectral_transform(pcnn_handle h, int xform);
int pcnn_get_spectral_transform(pcnn_handle h);
/* Filter spectra across calls (round 5).  A filter's spectrum depends on the weights alone; by default (version 0) every spectral convolution call
 * recomputes it into the workspace - correct for any caller, ~10 us + a launch gap per call.  A caller that knows WHEN its weights change tells the
 * handle: pcnn_set_filter_version(h, v) with v != 0 promises that every filter pointer passed to pcnn_conv2d_fwd / pcnn_conv2d_bwd_spectral(_post)
 * while the version is v holds the same values as at the first call under v.  The handle then keeps each filter's spectrum (key: pointer, shape, tile
 * size, transform family) in a buffer of its own; a call under the same version reuses it, and the first call under a NEW version refreshes every
 * filter the handle knows in ONE launch per tile size.  Inference: set a version once - no filter work after the first call.  Training: bump the
 * version after each optimizer step - one or two launches per step instead of one per layer and direction.  The setting is per call sequence: set 0
 * again before passing filters whose contents the version does not describe (poisson_cnn_amd.ops does that for every call without `w_version`).
 * Contract: a cached filter pointer must stay readable until pcnn_filter_cache_clear / pcnn_destroy (the refresh reads every known filter); memory:
 * Cin x ceil(Cout/32) x T^2 x 128 B per filter (4 MB at 32 -> 32 channels and 32-point tiles, 16 MB at 64-point tiles), pcnn_filter_cache_stats.
 * Under stream capture nothing is allocated: a filter first seen there is transformed into the workspace as with version 0.
 * pcnn_filter_cache_stats: entries / bytes describe what the handle holds now; hits / fills / refreshes are cumulative over the handle's life (a clear does not reset them). */
int pcnn_set_filter_version(pcnn_handle h, uint64_t version);
int pcnn_filter_cache_clear(pcnn_handle h);
int pcnn_filter_cache_stats(pcnn_handle h, long long* entries, long long* bytes, long long* hits, long long* fills, long long* refreshes);
/* The one LARGE buffer a handle owns (besides small scratch and, when a filter version is set, the kept filter spectra above): the spectral workspace (tile spectra of the layer in flight, mixing matrices,
 * constant tables).  By default it grows to a whole layer per launch - 8 x 1024^2 x 32 channels at 15 taps: ~11 GB, sized for 288 GB of
 * HBM.  pcnn_set_workspace_limit caps it (bytes; 0 = no cap): the launches then cover fewer tiles each (never fewer than 32; a layer that
 * cannot run inside the cap fails with an ordinary error), so a host program that budgets device memory itself decides what the
 * library may take.  Growth happens inside a convolution call (stream synchronise + free + allocate) until the largest layer shape has
 * been seen: call the largest shape once up front, or set the cap, to keep allocation out of the steady state. */
int pcnn_set_workspace_limit(pcnn_handle h, size_t bytes);
/* hipGraph safety (poisson_cnn_amd/graphs.py; no reference counterpart - TensorFlow's tf.function graphs own their scratch): a graph
 * captured on this handle's stream has the handle-owned buffers' addresses baked in.  retain = 1: a buffer the handle outgrows (or that a
 * lower pcnn_set_workspace_limit releases) is NOT freed but parked until pcnn_destroy, so that earlier captures keep replaying into valid
 * memory; later calls use the new, larger buffer.  retain = 0 (default): outgrown buffers are freed after a stream synchronise. */
int pcnn_set_workspace_retain(pcnn_handle h, int retain);

/* ---- 2-D convolution: tf.pad + tf.nn.conv2d(VALID) + bias + activation (+ BN affine) (+ residual) ----------
 * Replaces pad_and_apply_convolution (utils/apply_advanced_padding_and_call_conv_layer.py:16-20), Keras
 * Conv2D(padding='same') (models/Homogeneous_Poisson_NN_Legacy.py:71,75,95; layers/Scaling.py:28), the fused
 * BatchNormalization that follows it (blocks/resnet.py:31-36) and the residual add of blocks/resnet.py:37.
 *   z[n,y,x,co]   = bias[co] + sum_{i,j,ci} xpad[n, y - pad_top + i, x - pad_left + j, ci] * w[i,j,ci,co]
 *   a             = act(z);   y = a * bn_scale[co] + bn_shift[co] (if bn_scale);   y += residual (if residual)
 * w is Keras HWIO (kh,kw,Cin,Cout), dense.  Out-of-image reads follow pad_mode (CONSTANT uses pad_value).
 * Ho/Wo need not equal H/W (the data-gradient call uses Ho = H + kh - 1).
 * If act_out != NULL the pre-BN activation `a` is also written there (needed by the backward pass). */
typedef struct {
  int N, H, W, Cin, ldx;          /* input  */
  int Ho, Wo, Cout, ldy;          /* output */
  int kh, kw, pad_top, pad_left;
  int pad_mode; float pad_value;
  int act; float act_alpha;
  int ld_res;                     /* channel stride of residual (if given) */
  int ld_act_out;                 /* channel stride of act_out  (if given) */
} pcnn_conv_desc;

int pcnn_conv2d_fwd(pcnn_handle h, const pcnn_conv_desc* d, const float* x, const float* w, const float* bias,
                    const float* bn_scale, const float* bn_shift, const float* residual, float* y, float* act_out);
/* Same, and y_absmax[0] = max|y| over the tensor (device float, NULL = skip): when y is the input of the next convolution, that
 * layer's weight gradient takes it as its x_absmax hint (pcnn_conv2d_wgrad_hint).  The value is overwritten (not accumulated into), is the maximum
 * of the very floats that were stored (after the residual add), ignores NaNs and is clamped to 3.0e38 when the tensor holds an inf.  Every route of
 * this call honours it - the narrow vector-ALU kernels, both direct MFMA kernels, the split forward kernel and all spectral inverse kernels, also
 * when a workspace limit splits the layer into several launches (tests/test_gpu_absmax.py).  Out of scope: the wide-channel kernels of
 * csrc/conv_wide.hip (pcnn_wide_*) are reached through entry points of their own and have no such output. */
int pcnn_conv2d_fwd_absmax(pcnn_handle h, const pcnn_conv_desc* d, const float* x, const float* w, const float* bias,
                           const float* bn_scale, const float* bn_shift, const float* residual, float* y, float* act_out, float* y_absmax);

/* w (kh,kw,Cin,Cout) -> wt (kh,kw,Cout,Cin) with both taps reversed: the filter of the data-gradient convolution. */
int pcnn_conv2d_flip_transpose_weights(pcnn_handle h, const float* w, float* wt, int kh, int kw, int Cin, int Cout);
/* The same for n filters in ONE launch (a model's ~100 flipped filters are all re-formed when the weights change): `table_dev` is an array of n items in
 * DEVICE memory, ordered by `start` = the running sum of the previous items' element counts (start of item 0 = 0), total = the sum over all items. */
typedef struct pcnn_flip_item { const float* w; float* wt; int kh, kw, Cin, Cout; int64_t start; } pcnn_flip_item;
int pcnn_conv2d_flip_transpose_table(pcnn_handle h, const pcnn_flip_item* table_dev, int n, int64_t total);

/* Filter gradient of the convolution above (tf.nn.conv2d backprop-filter):
 *   dw[i,j,ci,co] = sum_{n,y,x} xpad[n, y - pad_top + i, x - pad_left + j, ci] * dz[n,y,x,co]
 * d describes the FORWARD convolution (x is its input, dz the gradient at its pre-activation output, ldy = its
 * channel stride).  workspace must hold pcnn_conv2d_wgrad_workspace(d) bytes.  The result is deterministic. */
size_t pcnn_conv2d_wgrad_workspace(const pcnn_conv_desc* d);
int pcnn_conv2d_wgrad(pcnn_handle h, const pcnn_conv_desc* d, const float* x, const float* dz, float* dw,
                      void* workspace, size_t workspace_bytes);
/* Same with optional hints: x_absmax / dz_absmax point to device floats holding max|x| / max|dz| (exact, or any finite upper bound
 * within a factor 2^10: the scale only has to keep the fp16 halves in range), NULL = compute here.  Ignored in the fp32 math mode.
 * A hint is about the tensor alone: the constant of a CONSTANT-padded layer (d->pad_value) is taken into x's scale by the library itself, so a
 * padding value far above max|x| does not overflow the halves.  An inf / NaN hint is clamped (the scale falls back to 1).
 * tests/test_gpu_absmax.py pins this contract: exact hints give the same bits as no hints; hints 2^5 and 2^10 too large for either tensor or both
 * stay at the unhinted error (measured 2.0e-7 rel-L2 against fp64 for all three factors on 3x3 20 -> 24, bound 5e-6); the hints that layers.py
 * and models.py thread through a training step satisfy max|t| <= hint <= 2^10 max|t| for the tensors they are handed with. */
int pcnn_conv2d_wgrad_hint(pcnn_handle h, const pcnn_conv_desc* d, const float* x, const float* dz, float* dw,
                           void* workspace, size_t workspace_bytes, const float* x_absmax, const float* dz_absmax);

/* Both gradients of a wide-filter layer in one call on the spectral route (csrc/spectral_conv.hip): the spectrum of dz's tile windows is
 * computed once and serves the data gradient (d/dx of the same tf.nn.conv2d) AND the filter gradient, which is formed input-partitioned.
 * d: the FORWARD convolution; dg: its data-gradient convolution (input dz with channel stride dg->ldx, filter w_flipped = the output of
 * pcnn_conv2d_flip_transpose_weights, output dx (N,dg->Ho,dg->Wo,Cin) with stride dg->ldy - for SYMMETRIC / REFLECT layers the gradient on
 * the padded domain, Ho = H + kh - 1; residual (stride dg->ld_res) is added to dx if given).  Eligibility (cost model, Cout <= 32, zero
 * constant padding) must be asked first; an ineligible layer uses pcnn_conv2d_wgrad + pcnn_conv2d_fwd as before. */
/* One narrow resnet stage as ONE launch (csrc/conv_small.hip, round 4): blocks/resnet.py:29-39 with 3 x 3 filters, C = 4 / 8 channels on both
 * sides of all three convolutions, zero CONSTANT padding, no BatchNormalization, activation linear / relu / leaky relu:
 *   o0 = act(conv0(x) + b0);  a1 = act(conv1(o0) + b1);  o1 = x + a1;  y = act(conv2(o1) + b2)
 * x, y and the optional outputs are dense NHWC (N, H, W, C), 16-byte aligned; filters (3, 3, C, C); biases may be NULL.  o0 / a1 / o1 (each may be
 * NULL) receive what the three pcnn_conv2d_fwd calls of the unfused chain leave behind for the backward pass (conv1's input, conv1's act_out,
 * conv2's input): with them the existing backward calls run unchanged.  Same fp32 FMA chain per output value as the narrow forward kernel. */
int pcnn_resnet3_fwd_eligible(pcnn_handle h, int C, int act);
int pcnn_resnet3_fwd(pcnn_handle h, int N, int H, int W, int C, int act, float act_alpha, const float* x, const float* w0, const float* b0,
                     const float* w1, const float* b1, const float* w2, const float* b2, float* o0, float* a1, float* o1, float* y);

int pcnn_conv2d_bwd_spectral_eligible(pcnn_handle h, const pcnn_conv_desc* d, const pcnn_conv_desc* dg);
int pcnn_conv2d_bwd_spectral(pcnn_handle h, const pcnn_conv_desc* d, const pcnn_conv_desc* dg, const float* x, const float* dz, const float* w_flipped,
                             const float* residual, float* dx, float* dw);
/* The same call with the activation backward of the PRODUCING layer fused into the data gradient's epilogue (round 4): in a chain
 * a_prev = act(conv_prev(...)); y = conv(a_prev) the gradient dx that this call produces is at once multiplied by act'(a_prev) - which is what
 * pcnn_conv2d_epilogue_bwd would do in a separate pass over the tensor before conv_prev's own backward (blocks/resnet.py:29-39 chains three
 * such layers; models/Homogeneous_Poisson_NN_Legacy.py:86-96 seven such blocks):
 *   v = dgrad(dz) (+ residual);  raw_out (optional, stride ld_raw) = v;  dx = v * act'(act_out);  dbias (optional, Cin floats) = sum over pixels of dx.
 * act_out (stride ld_act_out) is conv_prev's saved activation output, act / act_alpha its activation.  Available where the data gradient has
 * one channel group (Cin <= 32; both the 32-point and - since the second session of round 4 - the 64-point inverse kernel carry the epilogue; ask
 * _post_eligible); otherwise call pcnn_conv2d_bwd_spectral and pcnn_conv2d_epilogue_bwd. */
typedef struct pcnn_post_desc {
  const float* act_out; int ld_act_out; int act; float act_alpha;
  float* dbias; float* raw_out; int ld_raw;
} pcnn_post_desc;
int pcnn_conv2d_bwd_spectral_post_eligible(pcnn_handle h, const pcnn_conv_desc* d, const pcnn_conv_desc* dg);
int pcnn_conv2d_bwd_spectral_post(pcnn_handle h, const pcnn_conv_desc* d, const pcnn_conv_desc* dg, const float* x, const float* dz, const float* w_flipped,
                                  const float* residual, float* dx, float* dw, const pcnn_post_desc* post);

/* The same fusion for the NARROW layers (<= 16 channels, 3x3 / 5x5: the tail of the final stack, models/Homogeneous_Poisson_NN_Legacy.py:86-96), whose data
 * gradient runs on the vector-ALU kernel (csrc/conv_small.hip) and not through pcnn_conv2d_bwd_spectral: dx = conv(dz; w_flipped) with the data-gradient
 * descriptor dg (as one would pass it to pcnn_conv2d_fwd: zero padding kh - 1 - pad_top / kw - 1 - pad_left, linear epilogue) + residual, then `post` exactly as
 * above - raw_out receives the sum, dx receives it times act'(act_out), dbias the per-channel sums of dx (partial sums per workgroup in the handle's scratch,
 * reduced in a fixed order: deterministic).  dx and raw_out are bit-identical to pcnn_conv2d_fwd followed by pcnn_conv2d_epilogue_bwd; dbias differs from that
 * pair in summation order only.  Replaces the tape's tf.nn.conv2d_backprop_input + the activation gradient of the producing layer (tf.GradientTape,
 * models/Homogeneous_Poisson_NN_Legacy.py:265-270).  Eligible: the narrow route for dg, a channel count of dx that is a multiple of 4, 16-byte aligned
 * tensors with channel strides that are multiples of 4; otherwise call pcnn_conv2d_fwd and pcnn_conv2d_epilogue_bwd. */
int pcnn_conv2d_dgrad_post_eligible(pcnn_handle h, const pcnn_conv_desc* dg, const float* dz, const float* residual, const float* dx, const pcnn_post_desc* post);
int pcnn_conv2d_dgrad_post(pcnn_handle h, const pcnn_conv_desc* dg, const float* dz, const float* w_flipped, const float* residual, float* dx,
                           const pcnn_post_desc* post);

/* Diagnostics (tests / tools only; no reference counterpart): the tile spectra of one image exactly as the forward transform of a spectral
 * convolution writes them, with the transform kernels the handle currently selects - out: [tile groups][channel groups][T*T rows][32] floats
 * (layout: csrc/spectral_common.h).  tests/test_gpu_spectral_fft.py and test_gpu_spectral64.py compare the kernel families row by row. */
int pcnn_debug_forward_spectrum32(pcnn_handle h, int H, int W, int C, const float* x, int Vy, int Vx, int oy, int ox, int pad_mode, float pad_value,
                                  int ylim, int xlim, int pack, float* out, size_t out_floats);
int pcnn_debug_tile_spectrum64(pcnn_handle h, int H, int W, int C, const float* x, int ylim, int xlim, float* out);

/* Backward of the fused epilogue: given dy (gradient at y) and the saved activation a = act(z),
 *   dz = dy * bn_scale[c] * act'(z)      (act' recovered from a: leaky -> a>0 ? 1 : alpha, tanh -> 1-a^2)
 * and the per-channel sums  dbias[c] = sum dz,  dgamma_hat[c] = sum dy*a,  dbeta[c] = sum dy  (the caller turns
 * dgamma_hat/dbeta into BN gamma/beta gradients).  Any of dbias/dsum_dy_a/dsum_dy may be NULL.
 * npix = N*H*W.  workspace: pcnn_colsum_workspace(C) bytes. */
size_t pcnn_colsum_workspace(int C);
int pcnn_conv2d_epilogue_bwd(pcnn_handle h, int64_t npix, int C, const float* dy, int lddy, const float* a, int lda,
                             const float* bn_scale, int act, float act_alpha, float* dz, int lddz,
                             float* dbias, float* dsum_dy_a, float* dsum_dy, void* workspace, size_t workspace_bytes);
/* Same, and additionally dz_absmax[0] = max|dz| over the tensor (device float, NULL = skip): the weight-gradient kernels of the
 * split math mode scale dz by this maximum - computing it here saves them a pass over dz (pcnn_conv2d_wgrad_hint) */
int pcnn_conv2d_epilogue_bwd_absmax(pcnn_handle h, int64_t npix, int C, const float* dy, int lddy, const float* a, int lda,
                                    const float* bn_scale, int act, float act_alpha, float* dz, int lddz, float* dbias,
                                    float* dsum_dy_a, float* dsum_dy, float* dz_absmax, void* workspace, size_t workspace_bytes);

/* Adjoint of tf.pad SYMMETRIC / REFLECT / CONSTANT: folds the gradient on the padded domain
 * gp (N, H+pt+pb, W+pl+pr, C) back onto the un-padded image: gx[n,y,x,c] = sum of gp over all padded positions
 * that read (y,x).  accumulate != 0 adds into gx. */
int pcnn_pad_fold_bwd(pcnn_handle h, int N, int H, int W, int C, int pt, int pb, int pl, int pr, int pad_mode,
                      const float* gp, int ldgp, float* gx, int ldgx, int accumulate);
/* The same fold AND the activation backward of the layer that produced the convolution's input, in one pass (round 5; the counterpart of
 * pcnn_conv2d_bwd_spectral_post for SYMMETRIC / REFLECT-padded layers, whose data gradient arrives on the padded domain): g = fold(gp) [+ add_to],
 * post->raw_out = g (optional), dz = g * bn_scale * act'(post->act_out), post->dbias[c] = sum dz, dsum_dy_a[c] = sum g * act_out, dsum_dy[c] = sum g
 * (each optional; bn_scale NULL = 1: the arguments of pcnn_conv2d_epilogue_bwd, whose arithmetic this is operation for operation; fixed summation
 * order).  dx itself never reaches memory.  Eligibility (channels and every channel stride a multiple of 4, 16-byte aligned tensors, C <= 256) must be asked first; workspace:
 * pcnn_colsum_workspace(C) bytes. */
int pcnn_pad_fold_bwd_post_eligible(int C, int ldgp, int ld_add, const void* gp, const void* add_to, const pcnn_post_desc* post, int lddz, const void* dz);
int pcnn_pad_fold_bwd_post(pcnn_handle h, int N, int H, int W, int C, int pt, int pb, int pl, int pr, int pad_mode, const float* gp, int ldgp,
                           const float* add_to, int ld_add, const pcnn_post_desc* post, const float* bn_scale, float* dsum_dy_a, float* dsum_dy,
                           float* dz, int lddz, void* workspace, size_t workspace_bytes);

/* Inference-mode BatchNormalization(axis=1, epsilon) folded to a per-channel affine (blocks/resnet.py:26-27,
 * models/Homogeneous_Poisson_NN_Legacy.py:55):  scale = gamma / sqrt(var + eps), shift = beta - mean * scale, for n channels
 * (all BN layers of a model are processed in one call).  bwd: given S1 = sum dy*a and S2 = sum dy from
 * pcnn_conv2d_epilogue_bwd:  dgamma = (S1 - mean*S2) / sqrt(var+eps),  dbeta = S2. */
int pcnn_bn_fold(pcnn_handle h, int n, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                 float* scale, float* shift);
int pcnn_bn_fold_bwd(pcnn_handle h, int n, const float* s_dy_a, const float* s_dy, const float* mean, const float* var, float eps,
                     float* dgamma, float* dbeta);

/* Training-mode BatchNormalization (fused semantics; optional - the reference's train_step most likely runs BN in inference
 * mode).  The conv writes the activation a (npix, C; row stride lda); pcnn_bn_train_fwd then
 *   - sums d = a - K_c and d*d per channel, K_c = the average of the channel's first 8 pixels: centred fp32 sums keep the variance
 *     when |mean| >> std, where sum a*a / n - mean^2 cancels,
 *   - forms mean = K + E[d], var = max(E[d*d] - E[d]^2, 0), inv_std = 1/sqrt(var+eps), scale = gamma*inv_std and updates the moving
 *     statistics (momentum; moving_var takes the unbiased variance var*n/(n-1), n > 1),
 *   - writes y = (a - mean)*scale + beta (+ residual; y may alias residual).
 * a is read twice.  mean / inv_std / scale (C floats each) are what pcnn_bn_train_bwd needs:
 *   dgamma = inv_std * sum dy*(a - mean),  dbeta = sum dy,  da = scale * (dy - dbeta/n - xhat * dgamma/n),  xhat = (a - mean)*inv_std.
 * All sums are two-stage in a fixed order (deterministic).  C <= 256.  scratch_2C / scratch_4C: 2*C / 4*C floats; workspace:
 * pcnn_colsum_workspace(C) bytes.  pcnn_channel_affine is the plain y = x*scale + shift (+residual) of the softmax-weighted sums. */
int pcnn_channel_affine(pcnn_handle h, int64_t npix, int C, const float* x, int ldx, const float* scale, const float* shift,
                        const float* residual, int ld_res, float* y, int ldy);
int pcnn_bn_train_fwd(pcnn_handle h, int64_t npix, int C, const float* a, int lda, const float* gamma, const float* beta, float eps,
                      float momentum, float* moving_mean, float* moving_var, float* mean, float* inv_std, float* scale, float* scratch_2C,
                      const float* residual, int ld_res, float* y, int ldy, void* workspace, size_t workspace_bytes);
int pcnn_bn_train_bwd(pcnn_handle h, int64_t npix, int C, const float* dy, int lddy, const float* a, int lda, const float* scale,
                      const float* mean, const float* inv_std, float* dgamma, float* dbeta, float* scratch_4C, float* da, int ldda,
                      void* workspace, size_t workspace_bytes);

/* ---- pooling: tf.keras.layers.{Average,Max}Pooling2D(pool_size=f, strides=f, padding='same') ----------------
 * (utils/get_pooling_method.py:3-6; blocks/bottleneck_block.py:36-37; layers/Scaling.py:29).
 * Ho = ceil(H/f); window origin o*f - (Ho*f-H)/2; the average divides by the number of valid elements. */
int pcnn_pool2d_fwd(pcnn_handle h, int kind, int N, int H, int W, int C, int f, const float* x, int ldx, float* y, int ldy);
int pcnn_pool2d_bwd(pcnn_handle h, int kind, int N, int H, int W, int C, int f, const float* x, int ldx,
                    const float* y, int ldy, const float* dy, int lddy, float* dx, int lddx, int accumulate);

/* ---- transposed convolution with kernel == stride (layers/deconvupscale.py:103-108) ---------------------------
 * tf.nn.conv2d_transpose(x, k, output_shape=(N,Cout,H,W), strides=f, padding='SAME') + bias, k is (f,f,Cout,Cin):
 *   y[n,Y,X,co] = bias[co] + sum_ci x[n,(Y+py)/f,(X+px)/f,ci] * k[(Y+py)%f,(X+px)%f,co,ci],  py=(h*f-H)/2.
 * y = beta*y + alpha*(...) so the 8-way branch merge (models/Homogeneous_Poisson_NN_Legacy.py:222) accumulates in place. */
int pcnn_deconv_fwd(pcnn_handle h, int N, int hc, int wc, int Cin, int H, int W, int Cout, int f, const float* x, int ldx,
                    const float* k, const float* bias, float alpha, float beta, float* y, int ldy);
int pcnn_deconv_bwd_data(pcnn_handle h, int N, int hc, int wc, int Cin, int H, int W, int Cout, int f, const float* dy, int lddy,
                         const float* k, float alpha, float* dx, int lddx);
/* dk (f,f,Cout,Cin) and dbias (Cout) ; workspace: pcnn_deconv_wgrad_workspace bytes */
size_t pcnn_deconv_wgrad_workspace(int N, int hc, int wc, int Cin, int Cout, int f);
int pcnn_deconv_bwd_filter(pcnn_handle h, int N, int hc, int wc, int Cin, int H, int W, int Cout, int f, const float* x, int ldx,
                           const float* dy, int lddy, float alpha, float* dk, float* dbias, void* workspace, size_t workspace_bytes);

/* ---- wide-channel convolutions of the UNet baseline (models/UNet.py; csrc/conv_wide.hip) -----------------------------------------------
 * Any Cin, Cout >= 1 (channel tails masked), NHWC with channel strides, implicit GEMMs on v_mfma_f32_32x32x2_f32.  These kernels compute exact
 * fp32 products with fp32 accumulation in EVERY math mode (pcnn_set_math_mode does not apply to them).
 * One descriptor for every call; it describes the operation in the direction it runs: input (N,H,W,Cin) with channel stride ldx, output
 * (N,Ho,Wo,Cout) with stride ldy.  `k`: the odd filter size of a SAME convolution (Ho = H, Wo = W), or f = kernel = stride of a transposed one.
 * Forward calls: epilogue z = acc + bias[co]; dropout (rate > 0) z = keep ? z / (1 - rate) : 0; y = act(z).
 * Data-gradient calls: dx = acc * act'(act_out) [* dropout mask / (1 - rate)] where act / dropout / act_out (stride ld_act_out) describe the
 * layer that PRODUCED the tensor whose gradient is formed (act' is taken from that layer's output: ReLU' = [a > 0], and with ReLU the mask is
 * implied by a > 0, so it is not recomputed); act_out == NULL: no epilogue.  accumulate = 1: y += result instead of y = result.
 * Dropout mask (stateless; element idx = pixel * C + channel of the dense NHWC tensor of C channels being produced, pixel = (n*H + y)*W + x):
 *   fmix(h) = murmur3 finaliser: h ^= h>>16; h *= 0x85EBCA6B; h ^= h>>13; h *= 0xC2B2AE35; h ^= h>>16  (uint32 arithmetic)
 *   h = fmix(seed ^ (layer * 0x9E3779B9)); h = fmix(h ^ (idx >> 32)); h = fmix(h ^ (idx & 0xFFFFFFFF))
 *   keep iff h >= floor(min((double)rate * 2^32, 2^32 - 1))
 * The Keras inverted dropout of ConvBlock (models/UNet.py:69-75 `layers.Dropout(rate)` under training=True). */
typedef struct {
  int N, H, W, Cin, ldx;          /* input  */
  int Ho, Wo, Cout, ldy;          /* output */
  int k;
  int act; float act_alpha;
  float dropout_rate; uint32_t dropout_seed; uint32_t dropout_layer;
  int ld_act_out;
  int accumulate;
} pcnn_wide_desc;
/* tf.keras.layers.Conv2D(filters, k, padding='same') + Dropout + Activation of ConvBlock (models/UNet.py:46-77) and the 1x1 head (:260-265):
 * w (k,k,Cin,Cout) Keras HWIO, bias (Cout) or NULL. */
int pcnn_wide_conv2d_fwd(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* w, const float* bias, float* y);
/* Its data gradient (tf.nn.conv2d backprop-input under the GradientTape of models/UNet.py:169-177): the same engine on
 * wf = pcnn_conv2d_flip_transpose_weights(w) (k,k,Cout_fwd,Cin_fwd); d: input dz (Cin = the forward Cout), output dx (Cout = the forward Cin). */
int pcnn_wide_conv2d_dgrad(pcnn_handle h, const pcnn_wide_desc* d, const float* dz, const float* wf, const float* act_out, float* dx);
/* Filter gradient dw[i,j,ci,co] = sum_p x[p + (i,j) - k/2, ci] dz[p, co] and dbias[co] = sum_p dz[p, co] (NULL = skip); d = the FORWARD
 * descriptor (dz has stride ldy).  Split-K over the pixels into `workspace` (pcnn_wide_conv2d_wgrad_workspace bytes), reduced in a fixed order:
 * deterministic. */
size_t pcnn_wide_conv2d_wgrad_workspace(const pcnn_wide_desc* d);
int pcnn_wide_conv2d_wgrad(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* dz, float* dw, float* dbias, void* workspace,
                           size_t workspace_bytes);
/* deconvupscale with kernel_size == upsample_ratio = f (layers/deconvupscale.py:100-109, models/UNet.py:246): tf.nn.conv2d_transpose(x, k,
 * (N,Ho,Wo,Cout), strides=f, padding='SAME') + bias + act, k (f,f,Cout,Cin); H = ceil(Ho/f), W = ceil(Wo/f):
 *   y[n,Y,X,co] = act(bias[co] + sum_ci x[n,(Y+py)/f,(X+px)/f,ci] * k[(Y+py)%f,(X+px)%f,co,ci]),  py = (H*f - Ho)/2, px = (W*f - Wo)/2.
 * A per-input-pixel GEMM (Cin x f*f*Cout) followed by depth-to-space in the epilogue.  No dropout, no accumulate. */
int pcnn_wide_deconv_fwd(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* k, const float* bias, float* y);
/* Its data gradient: d: input dz on the fine grid (N,H,W,Cin = the deconvolution's Cout, stride ldx), output dx on the coarse grid
 * (N,Ho,Wo,Cout = the deconvolution's Cin, stride ldy), Ho = ceil(H/f); dz is the gradient AFTER the deconvolution's own activation backward;
 * epilogue as for every data gradient. */
int pcnn_wide_deconv_bwd_data(pcnn_handle h, const pcnn_wide_desc* d, const float* dz, const float* k, const float* act_out, float* dx);
/* Its filter gradient dk (f,f,Cout,Cin); d = the FORWARD descriptor (x coarse stride ldx, dz fine stride ldy).  Deterministic split-K;
 * the bias gradient is the channel sum of dz (pcnn_epilogue_bwd). */
size_t pcnn_wide_deconv_bwd_filter_workspace(const pcnn_wide_desc* d);
int pcnn_wide_deconv_bwd_filter(pcnn_handle h, const pcnn_wide_desc* d, const float* x, const float* dz, float* dk, void* workspace,
                                size_t workspace_bytes);

/* ---- tf.image.resize(antialias=False, half-pixel centres) (layers/Upsample.py:56-59) ------------------------
 * Separable 4-tap gather: idx_y/wt_y are (Ho,4) tables, idx_x/wt_x (Wo,4) (nearest/bilinear use fewer taps with
 * zero weights).  Tables come from pcnn_resize_tables (host, float32 arithmetic of the TF kernels).
 * y = beta*y + alpha*resize(x). */
int pcnn_resize_tables(int method, int n_in, int n_out, int32_t* idx /*n_out*4*/, float* wt /*n_out*4*/);
int pcnn_resize_fwd(pcnn_handle h, int N, int hc, int wc, int C, int Ho, int Wo, const float* x, int ldx,
                    const int32_t* idx_y, const float* wt_y, const int32_t* idx_x, const float* wt_x,
                    float alpha, float beta, float* y, int ldy);
/* The resize branches of a merge in one pass over the destination (round 6; models/Homogeneous_Poisson_NN_Legacy.py:215-224: the three multilinear bottleneck
 * branches are summed into the merge buffer): y = beta*y + alpha*(resize(x_0) + ... + resize(x_{nsrc-1})), nsrc = 2 or 3, accumulated in the order and with the
 * roundings of nsrc consecutive pcnn_resize_fwd calls (beta, then 1, 1): bit-identical to them, with one read-modify-write of y instead of nsrc.  Eligible: C a
 * multiple of 4, 16-byte aligned tensors, channel strides multiples of 4. */
typedef struct pcnn_resize_src {
  const float* x; int hc, wc, ldx;
  const int32_t* idx_y; const float* wt_y; const int32_t* idx_x; const float* wt_x;
} pcnn_resize_src;
int pcnn_resize_fwd_multi_eligible(int N, int C, int Ho, int Wo, int nsrc, const pcnn_resize_src* src, const float* y, int ldy);
int pcnn_resize_fwd_multi(pcnn_handle h, int N, int C, int Ho, int Wo, int nsrc, const pcnn_resize_src* src, float alpha, float beta, float* y, int ldy);
/* dx = alpha * resize^T(dy); tmp must hold N*hc*Wo*C floats */
int pcnn_resize_bwd(pcnn_handle h, int N, int hc, int wc, int C, int Ho, int Wo, const float* dy, int lddy,
                    const int32_t* idx_y, const float* wt_y, const int32_t* idx_x, const float* wt_x,
                    float alpha, float* tmp, float* dx, int lddx);

/* ---- per-sample-filter ("metalearning") convolutions: ONE launch for the whole batch -------------------------------------------
 * Replace the tf.map_fn over samples of layers/metalearning_conv.py:148-169 (tf.pad + tf.nn.conv{1,2}d + bias per sample, filter and bias
 * emitted by the layer's hyper-network) and layers/metalearning_deconvupscale.py:104-137 (conv2d_transpose, kernel = stride).  Sample n
 * uses the filter at w + n * w_sample_stride (HWIO (kh,kw,Cin,Cout); transposed convolution (f,f,Cout,Cin)) and the bias at
 * bias + n * bias_sample_stride.  d->N = batch, <= 32 output channels, <= 31 taps; 1-D layers are kh = 1.
 *   _deconv_*  conv2d_transpose(kernel = stride = f, padding='SAME') exactly as TensorFlow crops it (layers/metalearning_deconvupscale.py:13-16):
 *           the coarse grid must be H = ceil(Ho / f), W = ceil(Wo / f) (TensorFlow raises otherwise, and so do these calls) and output pixel
 *           Y reads coarse row (Y + py) / f through tap (Y + py) % f with py = (H f - Ho) / 2 (likewise in x) - the same offset as
 *           pcnn_deconv_fwd.  _bwd_filter sums strips of coarse rows in a fixed order (deterministic; partials in the handle's scratch).
 *   _fwd    flip_transpose = 0: y = act(conv(pad(x), w_n) + b_n).  flip_transpose = 1: the same kernel as the DATA gradient - x is dz, the
 *           stored filter is the forward filter (kh,kw,Cout_of_this_call,Cin_of_this_call), read flipped and transposed.
 *   _wgrad  dw_n = filter gradient of sample n (not summed over the batch); workspace: pcnn_grouped_conv2d_wgrad_workspace(d) bytes.
 *   Routes: layers of <= 16 output and <= 16 input channels (every layer of the reference's metalearning configurations) run as a GROUPED
 *   IMPLICIT GEMM on the matrix cores (v_mfma_f32_4x4x1_16B_f32: 4 output channels x 64 pixels x one (tap, channel) step per instruction,
 *   exact fp32, the filter of sixteen K steps in one register through the instruction's A-broadcast); wider layers on the vector ALUs.
 *   pcnn_grouped_conv2d_uses_mfma(d, what) reports the route (what = 0: _fwd, 1: _wgrad); environment PCNN_GROUPED_VALU=1 forces the
 *   vector-ALU kernels. */
size_t pcnn_grouped_conv2d_wgrad_workspace(const pcnn_conv_desc* d);
int pcnn_grouped_conv2d_uses_mfma(const pcnn_conv_desc* d, int what);
int pcnn_grouped_conv2d_fwd(pcnn_handle h, const pcnn_conv_desc* d, const float* x, const float* w, long long w_sample_stride, const float* bias,
                            long long bias_sample_stride, int flip_transpose, float* y);
int pcnn_grouped_conv2d_wgrad(pcnn_handle h, const pcnn_conv_desc* d, const float* x, const float* dz, float* dw, long long dw_sample_stride, void* workspace);
int pcnn_grouped_bias_grad(pcnn_handle h, int N, long long HW, int C, const float* dz, int lddz, float* dbias, long long bias_sample_stride);
int pcnn_grouped_deconv_fwd(pcnn_handle h, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int f, const float* x, const float* k,
                            long long k_sample_stride, const float* bias, long long bias_sample_stride, float* y);
int pcnn_grouped_deconv_bwd_data(pcnn_handle h, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int f, const float* dy, const float* k,
                                 long long k_sample_stride, float* dx);
int pcnn_grouped_deconv_bwd_filter(pcnn_handle h, int N, int H, int W, int Cin, int Ho, int Wo, int Cout, int f, const float* x, const float* dy,
                                   float* dk, long long k_sample_stride, float* dbias, long long bias_sample_stride);

/* ---- small dense layers (tf.keras.layers.Dense: models/Homogeneous_Poisson_NN_Legacy.py:99-102, layers/Scaling.py:31-33)
 * y[n,o] = act(b[o] + sum_i x[n,i] w[i,o]);  bwd: given dy and y, dx, dw (+=), db (+=).  b / db may be NULL: a Dense layer without bias
 * (use_bias=False reaches every Dense layer of the metalearning hyper-networks, layers/metalearning_conv.py:113,128) */
int pcnn_dense_fwd(pcnn_handle h, int N, int In, int Out, const float* x, const float* w, const float* b, int act, float alpha, float* y);
int pcnn_dense_bwd(pcnn_handle h, int N, int In, int Out, const float* x, const float* w, const float* y, const float* dy,
                   int act, float alpha, float* dx, float* dw, float* db);

/* ---- elementwise / layout helpers -------------------------------------------------------------------------- */
/* input assembly: out[n,y,x,0]=rhs, [1]=cos(pi*y/(H-1)), [2]=cos(pi*x/(W-1))  (models/..Legacy.py:172-180,198) */
int pcnn_assemble_input(pcnn_handle h, int N, int H, int W, const float* rhs, int use_pos, float* out, int ldo);
/* Strided convolutions (blocks/bottleneck_block.py:28-34, downsampling_method='conv'): the reference pads exactly as for stride 1
 * (utils/apply_advanced_padding_and_call_conv_layer.py:9-11) and lets the VALID convolution stride, i.e. it keeps every stride-th output
 * of the stride-1 result.  adjoint = 0: y (N, ceil(H/s), ceil(W/s), C) = x[:, ::s, ::s, :];  adjoint = 1: x is the coarse gradient, y the
 * full-resolution one (zero except at the kept positions). */
int pcnn_subsample(pcnn_handle h, int N, int H, int W, int C, int stride, const float* x, int ldx, float* y, int ldy, int adjoint);
/* y = alpha*x + beta*y over npix x C with channel strides */
int pcnn_axpby(pcnn_handle h, int64_t npix, int C, float alpha, const float* x, int ldx, float beta, float* y, int ldy);
/* y[n,p,c] = x[n,p,c]*s[n,c]  (tf.einsum('ijkl,ij->ijkl'), models/..Legacy.py:231); bwd gives dx and ds */
int pcnn_channel_scale_fwd(pcnn_handle h, int N, int64_t hw, int C, const float* x, int ldx, const float* s, float* y, int ldy);
int pcnn_channel_scale_bwd(pcnn_handle h, int N, int64_t hw, int C, const float* x, int ldx, const float* s, const float* dy, int lddy,
                           float* dx, int lddx, float* ds, void* workspace, size_t workspace_bytes);
size_t pcnn_channel_scale_workspace(int N, int64_t hw, int C);
/* pcnn_channel_scale_bwd with the activation backward of the layer that produced x fused in (round 6): x is that layer's saved activation output, so
 * dz = dy s act'(x) is written instead of dx - what pcnn_channel_scale_bwd followed by pcnn_conv2d_epilogue_bwd gives, bit for bit - and dbias (may be NULL)
 * receives the per-channel sums of dz in a fixed order.  workspace: 2 * pcnn_channel_scale_workspace(N, hw, C) bytes.  (The einsum of
 * models/Homogeneous_Poisson_NN_Legacy.py:231 follows the leaky-ReLU of post_merge_resnet's last convolution, :227-229.) */
int pcnn_channel_scale_bwd_post(pcnn_handle h, int N, int64_t hw, int C, const float* x, int ldx, const float* s, const float* dy, int lddy,
                                float* dz, int lddz, float* ds, int act, float act_alpha, float* dbias, void* workspace, size_t workspace_bytes);
/* per-sample scalar scale: y[n,..] = x[n,..]*(1+g[n]) (layers/Scaling.py:55); bwd: dx, dg[n] = sum dy*x */
int pcnn_sample_scale_fwd(pcnn_handle h, int N, int64_t per, const float* x, const float* g, float* y);
int pcnn_sample_scale_bwd(pcnn_handle h, int N, int64_t per, const float* x, const float* g, const float* dy, float* dx, float* dg);
/* BC ring (models/..Legacy.py:251): Dirichlet -> ring = 0 ; Neumann -> ring = adjacent interior.  1 channel.  These are pcnn_bc_ring_edges_fwd/bwd
 * with neumann_mask = neumann ? 15 : 0. */
int pcnn_bc_ring_fwd(pcnn_handle h, int N, int H, int W, int neumann, const float* x, float* y);
int pcnn_bc_ring_bwd(pcnn_handle h, int N, int H, int W, int neumann, const float* dy, float* dx);
/* The ring with a boundary type per edge (extension: the reference's bc_type is model-wide).  Edges are named as the dataset names them: on an
 * (N,1,H,W) tensor left is y = 0, right y = H-1, bottom x = 0, top x = W-1.  neumann_mask bit 0/1/2/3 set: the left/right/bottom/top edge is Neumann,
 * clear: Dirichlet (the order of pcnn_fd_poisson_mixed).  y = E_m x: interior points are copied; a ring point on any Dirichlet edge is 0 - at a corner a
 * Dirichlet edge wins - and any other ring point is x[clamp(y,1,H-2), clamp(x,1,W-2)], the first-order mirror u_0 = u_1 of tf.pad SYMMETRIC (a
 * Neumann/Neumann corner takes its diagonal neighbour).  bwd is E_m^T as a gather: no atomics, deterministic.  Mask 0 and mask 15 are
 * pcnn_bc_ring_fwd/bwd with neumann = 0 and 1.  H, W >= 3. */
int pcnn_bc_ring_edges_fwd(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* x, float* y);
int pcnn_bc_ring_edges_bwd(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* dy, float* dx);
/* Spatial pyramid max-pool over channels and spatial bins (layers/SpatialPyramidPool.py:35-66).
 * bins: nb x 4 int32 (y0,y1,x0,x1) on device; out (N, nb); argmax (N, nb) int32 flat index into (H,W,C) for bwd */
int pcnn_spp_max_fwd(pcnn_handle h, int N, int H, int W, int C, int nb, const int32_t* bins, const float* x, float* out, int32_t* argmax);
int pcnn_spp_max_bwd(pcnn_handle h, int N, int H, int W, int C, int nb, const int32_t* argmax, const float* dout, float* dx);
/* Jacobi post-smoother (layers/JacobiIterationLayer.py:43-66), 3x3 second-order stencil, one sweep */
int pcnn_jacobi_sweep(pcnn_handle h, int N, int H, int W, const float* u, const float* rhs, const float* dx /*N x 2*/, float* out);
int pcnn_jacobi_sweep_bwd(pcnn_handle h, int N, int H, int W, const float* dout, const float* dx /*N x 2*/, float* du);
/* The same smoother for any cross-shaped FD stencil (layers/JacobiIterationLayer.py:7-41: odd `stencil_sizes` per axis, any `orders`), n_sweeps sweeps
 * per call (:57-66) with several sweeps fused into one launch by temporal blocking in LDS.  sy taps along H and sx along W, both
 * odd in 3..9.  coef holds one row per sample as the layer composes its kernel (:43-46): the sy H-taps and the sx W-taps of (L+U) - centre entries
 * zero - then 1 / diagonal.  One sweep: out = coef[sy+sx] * (rhs - taps . u) where sy/2 <= y < H - sy/2 and sx/2 <= x < W - sx/2, out = u on the ring
 * (:48-52).  The result does not depend on how the sweeps are split into launches.  out must not alias u or rhs.  A call that needs more than one
 * launch (n_sweeps > pcnn_jacobi_fused_max_sweeps) keeps one intermediate image in the handle's auxiliary scratch. */
int pcnn_jacobi_fused_fwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef /*N x (sy+sx+1)*/, const float* u, const float* rhs,
                          int n_sweeps, float* out);
/* adjoint of those n_sweeps sweeps w.r.t. u (the guess): du = J^T dout.  du must not alias dout. */
int pcnn_jacobi_fused_bwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef /*N x (sy+sx+1)*/, const float* dout, int n_sweeps,
                          float* du);
/* the edge of the square output tile one workgroup owns, and the most sweeps one launch fuses for an sy x sx stencil */
int pcnn_jacobi_fused_tile(void);
int pcnn_jacobi_fused_max_sweeps(int sy, int sx);
/* The fused smoother with the model's boundary types (neumann_mask as for pcnn_bc_ring_edges_fwd).  One sweep is R_m o J: J the sweep above, R_m a
 * refresh of the frozen band.  With ry = sy/2, rx = sx/2 a point is in the left band where y < ry, the right band where y >= H-ry, the bottom band where
 * x < rx and the top band where x >= W-rx.  A point in no band keeps J(u); a point in any band on a Dirichlet edge keeps its value (frozen, as above);
 * any other band point takes J(u) at (my, mx), my = 2 ry - 1 - y in the left band, 2 (H-ry) - 1 - y in the right band, y otherwise, mx likewise: the
 * SYMMETRIC reflection of the updated interior, which for the 3 x 3 stencil is the ring of pcnn_bc_ring_edges_fwd on its Neumann edges.  n sweeps are
 * (R_m J)^n; bwd is du = (J^T R_m^T)^n dout, a gather.  Needs H >= 3 ry where the mask has a left or right bit and W >= 3 rx where it has a bottom or
 * top bit (mirror sources are interior points).  Mask 0 gives the bits of pcnn_jacobi_fused_fwd/bwd; the result does not depend on how the sweeps are
 * split into launches, and pcnn_jacobi_fused_max_sweeps is the fused depth here too.  The same aliasing rules and scratch. */
int pcnn_jacobi_fused_bc_fwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef /*N x (sy+sx+1)*/, const float* u, const float* rhs,
                             int n_sweeps, int neumann_mask, float* out);
int pcnn_jacobi_fused_bc_bwd(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* coef /*N x (sy+sx+1)*/, const float* dout, int n_sweeps,
                             int neumann_mask, float* du);

/* ---- loss (losses/loss_wrapper.py:53-71, losses/integral_loss.py:126-179) --------------------------------------
 * per-sample partial sums: out[n] = {sum|p-t|, sum (p-t)^2, sum G*(p-t)^2, max|t|}; G is the (H,W) quadrature map.
 * bwd: dpred[n,p] = c_mae[n]*sign(p-t) + (c_mse[n] + c_int[n]*G[p]) * 2 (p-t) */
int pcnn_loss_partials(pcnn_handle h, int N, int64_t hw, const float* pred, const float* target, const float* G, float* out /*N x 4*/);
int pcnn_loss_bwd(pcnn_handle h, int N, int64_t hw, const float* pred, const float* target, const float* G,
                  const float* c_mae, const float* c_mse, const float* c_int, float* dpred);
/* loss_wrapper bookkeeping on the N per-sample partials (losses/loss_wrapper.py:45-71): per-sample weights 1/peak^p,
 * division by the GLOBAL batch size, the scalar loss (+ *extra if given), the loss_bwd coefficients and the `mse` metric
 * of train_step (models/Homogeneous_Poisson_NN_Legacy.py:291). */
int pcnn_loss_coefficients(pcnn_handle h, int N, int64_t hw, const float* partials, float w_mae, float w_mse, float w_int,
                           int scale_by_peak, int global_batch_size, const float* extra, float* loss, float* c_mae, float* c_mse,
                           float* c_int, float* mse);
/* The same three with the integral term's exponent explicit (losses/integral_loss.py:88,153 `Lp_norm_power`: sum G (target - pred)^p; the
 * per-sample weight becomes 1 / peak^p, losses/loss_wrapper.py:68).  The entry points above are these with p = 2 (every shipped config). */
int pcnn_loss_partials_p(pcnn_handle h, int N, int64_t hw, const float* pred, const float* target, const float* G, float lp_power, float* partials);
int pcnn_loss_bwd_p(pcnn_handle h, int N, int64_t hw, const float* pred, const float* target, const float* G, const float* c_mae,
                    const float* c_mse, const float* c_int, float lp_power, float* dpred);
int pcnn_loss_coefficients_p(pcnn_handle h, int N, int64_t hw, const float* partials, float w_mae, float w_mse, float w_int, float lp_power,
                             int scale_by_peak, int global_batch_size, const float* extra, float* loss, float* c_mae, float* c_mse,
                             float* c_int, float* mse);
/* FD-Laplacian residual loss (losses/physics_informed_loss.py:35-50): per-sample sum of (rhs - conv(pred,kern_n))^2 over
 * the interior; kern (N, s, s); bwd accumulates into dpred.  */
int pcnn_pi_loss_partials(pcnn_handle h, int N, int H, int W, int s, const float* pred, const float* rhs, const float* kern, float* out /*N*/);
int pcnn_pi_loss_bwd(pcnn_handle h, int N, int H, int W, int s, const float* pred, const float* rhs, const float* kern,
                     const float* coef /*N*/, float* dpred);
/* The same two for a rectangular stencil (losses/physics_informed_loss.py:6-50 takes any `stencil_sizes`): kern (N, sy, sx), the interior is
 * sy/2 <= y < H - sy/2, sx/2 <= x < W - sx/2.  The entry points above are these with sy == sx == s. */
int pcnn_pi_loss_partials_rect(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* pred, const float* rhs, const float* kern,
                               float* out /*N*/);
int pcnn_pi_loss_bwd_rect(pcnn_handle h, int N, int H, int W, int sy, int sx, const float* pred, const float* rhs, const float* kern,
                          const float* coef /*N*/, float* dpred);
/* Error statistics of a prediction in one pass over the three fields (evaluate / predict / validation).  Per sample n, out[8n..8n+7] =
 * {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2}: e = pred - target and t = target over all H W points;
 * r = (p[i-1,j] - 2 p[i,j] + p[i+1,j]) / dx0^2 + (p[i,j-1] - 2 p[i,j] + p[i,j+1]) / dx1^2 - rhs[i,j] and f = rhs[i,j] over the (H-2)(W-2)
 * interior points, dx as for pcnn_jacobi_sweep (column 0: the H axis).  target == NULL: the first five entries are 0; rhs == NULL: the last
 * three are 0 and dx is not read; rhs needs dx and H, W >= 3.  Two launches, no atomics: a fixed number of workgroups per sample write
 * partials into the handle's scratch and a second kernel combines them in a fixed order, so equal inputs give equal bits. */
int pcnn_error_stats(pcnn_handle h, int N, int H, int W, const float* pred, const float* target /* may be NULL */,
                     const float* rhs /* may be NULL */, const float* dx /* N x 2; required with rhs */, float* out /* N x 8 */);

/* ---- optimizer: tf.keras.optimizers.Adam (train/utils.py:3-8), flat parameter bucket ---------------------------- */
int pcnn_adam_step(pcnn_handle h, int64_t n, float* w, const float* g, float* m, float* v, float lr, float beta1, float beta2,
                   float eps, int step, float grad_scale);
/* Adam(amsgrad=True): vhat = max(vhat, v) is the denominator's second moment (vhat == NULL: plain Adam) */
int pcnn_adam_amsgrad_step(pcnn_handle h, int64_t n, float* w, const float* g, float* m, float* v, float* vhat, float lr, float beta1,
                           float beta2, float eps, int step, float grad_scale);
int pcnn_sgd_step(pcnn_handle h, int64_t n, float* w, const float* g, float lr, float grad_scale);
/* tf.keras.optimizers.SGD(momentum, nesterov) (train/utils.py:7-8 hands optimizer_parameters to it): v = momentum v - lr g; w += v
 * (nesterov: w += momentum v - lr g). */
int pcnn_sgd_momentum_step(pcnn_handle h, int64_t n, float* w, const float* g, float* velocity, float lr, float momentum, int nesterov,
                           float grad_scale);

/* ---- gradient clipping on the flat gradient bucket: clipnorm / global_clipnorm / clipvalue of tf.keras OptimizerV2 (TF 2.4) ----------
 * train/utils.py:3-8 hands `optimizer_parameters` to tf.keras.optimizers.Adam / SGD, which accept these.  Restated from TF 2.4
 * (OptimizerV2._clip_gradients, tf.clip_by_norm, tf.clip_by_global_norm, tf.clip_by_value); parity unpinned like the rest of the TF arithmetic.
 * With g = grad_scale * (the bucket's contents) and a VARIABLE = one trainable entry of the bucket (a kernel, a bias, a BN gamma or beta vector):
 *   clipnorm c          g_v <- g_v * c / max(||g_v||_2, c)      per variable; ||g_v|| <= c (0 included): scale exactly 1.0f, the variable keeps its bits
 *   global_clipnorm c   G = sqrt(sum_v ||g_v||^2) over every variable of every participating bucket;  g <- g * c / max(G, c);
 *                       G not finite: every g becomes NaN (tf.clip_by_global_norm)
 *   clipvalue c         g <- min(max(g, -c), c), after either norm clip; a NaN stays a NaN
 * (the fourth option, decay d: the step uses lr / (1 + d t), t = updates already applied - a host scalar, poisson_cnn_amd/train.py).
 *
 * The PLAN (host only, no handle): the bucket's variables, in their physical order and with sizes[v] floats each, are cut into items
 * (item_var, item_start, item_len): item_len <= PCNN_GRAD_CLIP_CHUNK, consecutive items tile each variable once, none crosses a variable
 * boundary; var_first_item[v] .. var_first_item[v+1] are variable v's items (n_vars + 1 entries).  pcnn_grad_clip_plan_items returns the
 * item count (-1: bad argument); pcnn_grad_clip_plan fills the caller's arrays (non-zero: bad argument).  The device entry points take
 * DEVICE copies of these arrays.
 *
 * Sums: one fp32 partial per item in a fixed order (per lane, then a wave butterfly, then four wave sums from LDS), the partials of a variable
 * added in plan order in a double, the variables of a bucket and the buckets added in order in a double.  No float atomics: a result depends
 * on the gradient and the plan only.
 *
 * pcnn_grad_clip_workspace: bytes of `workspace` (8-byte aligned) for a plan.
 * pcnn_grad_clip_norms:  two launches.  sqnorm (n_vars floats, may be NULL) receives ||g_v||^2, *total (one double, may be NULL) the bucket's
 *                        sum of them; the workspace keeps the per-variable sums in double for pcnn_grad_clip_scales.
 * pcnn_grad_clip_scales: one launch.  mode PER_VARIABLE: scale[v], n_vars floats, from this bucket's workspace.  mode GLOBAL: scale[0] from
 *                        totals[0 .. n_totals) - the `total` of every participating bucket, in the caller's fixed order: this is the one extra
 *                        launch that combines several buckets, no host round trip.  global_norm (may be NULL; needs totals): sqrt(sum of totals)
 *                        as one float, in any mode (mode NONE: that only).
 * pcnn_grad_clip_apply:  one launch, in place: g <- clamp((grad_scale * g) * scale, -clipvalue, clipvalue); clipvalue < 0: no clamp; mode NONE:
 *                        scale = 1.  An item whose scale is exactly 1.0f is skipped when there is no clamp and grad_scale == 1.  The optimizer step
 *                        that follows runs with grad_scale = 1.
 * All device entry points are asynchronous on the handle's stream; the caller owns every buffer. */
#define PCNN_GRAD_CLIP_CHUNK 4096          /* floats per item: 4 rounds of 256 lanes x float4 */
#define PCNN_GRAD_CLIP_NONE 0
#define PCNN_GRAD_CLIP_PER_VARIABLE 1
#define PCNN_GRAD_CLIP_GLOBAL 2
int64_t pcnn_grad_clip_plan_items(int n_vars, const int64_t* sizes);
int pcnn_grad_clip_plan(int n_vars, const int64_t* sizes, int32_t* item_var, int64_t* item_start, int32_t* item_len, int32_t* var_first_item);
size_t pcnn_grad_clip_workspace(int64_t n_items, int n_vars);
int pcnn_grad_clip_norms(pcnn_handle h, const float* g, int64_t n_items, const int64_t* item_start, const int32_t* item_len, int n_vars,
                         const int32_t* var_first_item, float grad_scale, void* workspace, float* sqnorm, double* total);
int pcnn_grad_clip_scales(pcnn_handle h, int mode, float c, int64_t n_items, int n_vars, const void* workspace, int n_totals,
                          const double* totals, float* scale, float* global_norm);
int pcnn_grad_clip_apply(pcnn_handle h, float* g, int64_t n_items, const int32_t* item_var, const int64_t* item_start, const int32_t* item_len,
                         int mode, const float* scale, float grad_scale, float clipvalue);

/* ---- dataset: reference-solution generators (poisson_CNN/dataset) ------------------------------------------- */
/* Dirichlet 5-point FD Poisson solve by DST-I diagonalisation, fp64 on the f64 matrix cores; replaces
 * multigrid_poisson_solve + poisson_RHS (dataset/solvers/multigrid.py:98-150, dataset/solvers/cholesky.py:45-119):
 *   A u_int = -dx^2 f_int + (boundary values folded onto the first interior ring),  A = pyamg.gallery.poisson((H-2, W-2)).
 * rhs (N,H,W) fp32; left/right (N,W) are the values on axis -2 index 0 / -1, bottom/top (N,H) those on axis -1 index
 * 0 / -1 (multigrid.py:145-148); dx (N).  S_h ((H-2)^2), lam_h (H-2), S_w, lam_w: device copies of pcnn_dst_setup output.
 * tmp: 2*N*(H-2)*(W-2) doubles.  soln (N,H,W) fp32 (fp64 solve, fp32 I/O like the reference's cast at
 * dataset/generators/numerical.py:131); at a corner it holds the left / right value (the write order of multigrid.py:145-148).
 * This is the neumann_mask = 0 case of pcnn_fd_poisson_mixed's pipeline with S for V, V^-1 and their transposes (S is symmetric and its own
 * inverse): one build kernel, one division, one ring / interior writer (write_soln, csrc/dataset.hip) serve every FD solve of this header. */
int pcnn_dst_setup(int n, double* S /* (n-2)^2, host */, double* lam /* n-2, host */);
int pcnn_fd_poisson_dst(pcnn_handle h, int N, int H, int W, const float* rhs, const float* left, const float* right,
                        const float* bottom, const float* top, const float* dx, const double* S_h, const double* lam_h,
                        const double* S_w, const double* lam_w, double* tmp, float* soln);
/* The same solve with the two DST-I passes done by rocFFT (BASELINE.json north star: "HIP stencil + rocFFT kernel"): odd extension of the
 * right-hand side to 2 (H-1) x 2 (W-1), batched real 2-D FFT, division by the eigenvalues, the same FFT again - O(n^2 log n) against the
 * 8 n^3 FLOP of the GEMM form above, fp64 throughout.  rocFFT is bound at run time (dlopen; PCNN_ROCFFT_LIBRARY overrides the name); plans are
 * kept per (device, shape, batch).  lam_h / lam_w: the eigenvalues pcnn_dst_setup returns; workspace: pcnn_fd_poisson_fft_workspace bytes.
 * Measured per sample (tools/bench_fd_solver.py): 512^2 0.035 (GEMM) vs 0.076 ms, 1024^2 0.25 vs 0.35, 2048^2 1.86 vs 1.66 - the odd extension
 * quadruples the data and its lengths are awkward (2046 = 2 3 11 31), so poisson_cnn_amd.dataset takes this route from 2048 points per axis
 * (solver='auto'); below that the fp64 matrix cores win and the GEMM form is this route's checker in the tests. */
size_t pcnn_fd_poisson_fft_workspace(int N, int H, int W);
int pcnn_fd_poisson_fft(pcnn_handle h, int N, int H, int W, const float* rhs, const float* left, const float* right, const float* bottom,
                        const float* top, const float* dx, const double* lam_h, const double* lam_w, void* workspace, float* soln);
/* Mixed Dirichlet / Neumann 5-point solve on the same vertex-centred grid (the consumer in the reference is the
 * pressure projection of Navier_Stokes_2D/solvers.py:225-335, whose pure-Neumann system carries a zero-integral constraint, :258-259).
 * neumann_mask bit 0/1/2/3: left / right / bottom / top edge is Neumann - its array then holds du/dn (outward normal), its nodes are
 * unknowns closed by the second-order ghost node; otherwise the array holds the Dirichlet values.  All four Neumann: the singular mode
 * is dropped (solution with zero trapezoidal integral; the data need not be compatible).  Per axis the caller passes the eigen-decomposition
 * of the 1-D operator on that axis' mh (mw) unknowns: Vinv_h, V_h (mh x mh, row-major), lam_h; VinvT_w, VT_w (mw x mw, transposed), lam_w.
 * tmp: 2*N*mh*mw doubles. */
int pcnn_fd_poisson_mixed(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rhs, const float* left, const float* right,
                          const float* bottom, const float* top, const float* dx, const double* Vinv_h, const double* V_h,
                          const double* lam_h, const double* VinvT_w, const double* VT_w, const double* lam_w, double* tmp, float* soln);
/* C[b] = A[b] * B[b] in fp64 (row-major, stride 0 broadcasts an operand) on v_mfma_f64_16x16x4_f64 */
int pcnn_batched_gemm_f64(pcnn_handle h, int batch, int M, int Nn, int K, const double* A, int64_t strideA, int lda,
                          const double* B, int64_t strideB, int ldb, double* C, int64_t strideC, int ldc);
/* Separable series synthesis out[n,a,b] (+)= sum_{A<ka,B<kb} c[n,A,B] f((A+1) x_a) f((B+1) y_b), x = linspace(0,pi,H),
 * y = linspace(0,pi,W), f = sin (trig 0) or cos (trig 1) (dataset/utils/generate_smooth_function.py:45-62). */
int pcnn_series_synthesis(pcnn_handle h, int N, int H, int W, int ka, int kb, const float* coef, int trig, int accumulate, float* out);
/* A (solution, right-hand side) pair of one separable series in one launch, on the same grid x = linspace(0,pi,H), y = linspace(0,pi,W):
 *   soln[n,a,b] = sum_{A<ka,B<kb} c[n,A,B] phi_A(x_a) psi_B(y_b)
 *   rhs[n,a,b]  = sum_{A<ka,B<kb} c[n,A,B] (lam_a[n,A] + lam_b[n,B]) phi_A(x_a) psi_B(y_b)
 * coef (N,ka,kb), lam_a (N,ka), lam_b (N,kb), soln and rhs (N,H,W).  basis_a / basis_b choose phi / psi for the mode A = 1..k:
 *   0: sin(A t)   1: cos(A t)   2: sin((A - 1/2) t)   3: cos((A - 1/2) t)
 * - the eigenfunctions of -d2/dt2 on [0,pi] with (Dirichlet, Dirichlet), (Neumann, Neumann), (Dirichlet, Neumann) and (Neumann, Dirichlet)
 * ends.  ka, kb <= 16; any W (the grid is tiled in both directions). */
int pcnn_series_pair_synthesis(pcnn_handle h, int N, int H, int W, int ka, int kb, const float* coef, const float* lam_a, const float* lam_b,
                               int basis_a, int basis_b, float* soln, float* rhs);
/* out[n,a,b] (+)= sum_{r<R} U[n,r,a] V[n,r,b]: the Taylor component X(x)Y(y), X''Y + XY'' (dataset/generators/reverse.py:231-256) */
int pcnn_separable_sum(pcnn_handle h, int N, int H, int W, int R, const float* U, const float* V, int accumulate, float* out);
/* x[n,:] *= target[n] / max|x[n,:]| (dataset/utils/set_max_magnitude.py:14-50); factors (optional) receives the scale */
int pcnn_set_max_magnitude(pcnn_handle h, int N, int64_t per, const float* target, float* x, float* factors);
/* x[n,:] *= s[n] */
int pcnn_scale_samples(pcnn_handle h, int N, int64_t per, const float* s, float* x);

/* ---- dataset: variable-density problem div((1/rho) grad u) = f (csrc/varcoef.hip) ------ */
/* Same vertex-centred grid, one spacing per sample (dy = dx), Dirichlet data on all four edges, rho (N,H,W) fp32 on every node.  Flux form with
 * the face coefficients beta = 2 / (rho_a + rho_b) of the two nodes a face separates (the first matrix of dataset/generators/variable_density):
 *   (A u)[i,j] = sum over the four neighbours of beta_face (u[i,j] - u[neighbour]) / dx^2   on the (H-2) x (W-2) interior nodes,
 * A symmetric positive definite, A u = b with b = -f + (Dirichlet neighbours' values times their face coefficient / dx^2).  fp64 throughout,
 * no atomics, every reduction in a fixed order per sample: a sample's result does not depend on the batch it is solved in.
 * q = A p for p, q (N,H-2,W-2) fp64 with zero Dirichlet data, and pq[n] = p[n].q[n] from the same pass. */
int pcnn_varcoef_apply(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const double* p, double* q, double* pq);
/* Conjugate gradients on A u = b, preconditioned by the constant-coefficient DST solve z = S_h ((S_h r S_w) ./ (lam_h + lam_w)) S_w (S, lam: device
 * copies of pcnn_dst_setup output; four pcnn_batched_gemm_f64 products per iteration).  State lives on the device: `workspace`
 * (pcnn_varcoef_pcg_workspace bytes), scal (N x 8 doubles per sample: b.b, r.r, p.q, r.z (two slots), min rho, 2 that only the
 * *_bc_* entry points below use) and flags (N ints).
 *   setup:   b, x = interior of the initial guess x0 ((N,H,W) fp64, NULL: 0), r = b - A x, first direction; scal[n][5] = min rho[n], a NaN counting as
 *            -inf (the caller refuses anything but a positive minimum); flags[n] = 1 where ||r|| <= tol ||b|| already.  The workspace, scal and
 *            flags need no initialisation: setup writes every value before it is read, whatever the memory held.
 *   iterate: `iterations` iterations numbered from first_iteration (the count of iterations done before), no host round trip in between:
 *            alpha = r.z / p.q and beta = r.z_new / r.z_old are formed inside the update kernels from scal; flags[n] is raised when
 *            ||r|| <= tol ||b||, and a flagged sample's alpha and beta are 0 from then on - its x is frozen bit for bit.
 *   finish:  soln (N,H,W) fp32: interior from x, edges from the boundary arrays, through the one writer of every FD solve here (write_soln in
 *            csrc/dataset.hip: rows 0 / H-1, i.e. left / right, win the corners). */
size_t pcnn_varcoef_pcg_workspace(int N, int H, int W);
int pcnn_varcoef_pcg_setup(pcnn_handle h, int N, int H, int W, const float* rho, const float* rhs, const float* left, const float* right,
                           const float* bottom, const float* top, const float* dx, const double* x0, double tol, const double* S_h,
                           const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal,
                           int* flags);
int pcnn_varcoef_pcg_iterate(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, double tol, int first_iteration, int iterations,
                             const double* S_h, const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                             double* scal, int* flags);
int pcnn_varcoef_pcg_finish(pcnn_handle h, int N, int H, int W, const void* workspace, const float* left, const float* right, const float* bottom,
                            const float* top, float* soln);
/* The same problem with per-edge Dirichlet / Neumann conditions.  neumann_mask, the edge arrays and the unknowns are those of
 * pcnn_fd_poisson_mixed: bit 0/1/2/3 = left / right / bottom / top is Neumann, its array then holds du/dn along the outward normal and its nodes are
 * unknowns - mh x mw of them, rows (bit 0 ? 0 : 1) .. (bit 1 ? H-1 : H-2) and columns likewise with bits 2 / 3; at a corner a Dirichlet edge wins.
 * p, q, x and the workspace are sized by mh x mw.  rho and rhs are read on Neumann edge nodes too.
 *   operator: a Neumann edge node has no outward neighbour; the inward face of that direction counts twice, 2 beta_in (u_c - u_in) / dx^2 (both
 *             directions at a Neumann/Neumann corner).  Faces between two nodes of one Neumann edge are ordinary faces.
 *   b:        -f, plus beta / dx^2 times the value of every Dirichlet neighbour, plus 2 g / (rho_c dx) for every Neumann edge the node lies on: the
 *             coefficient 1 / rho_c of the boundary face of the node's half cell (second order; the mirrored face's beta would be first order).
 *   weights:  w = w_i w_j, 1/2 per Neumann edge the node lies on.  W A is symmetric - positive definite with a Dirichlet edge, semi-definite with the
 *             constants as null space for mask 15 - and the loop is conjugate gradients in the W inner product: pq, b.b, r.r, r.z are sums of w (..),
 *             a sample is flagged when sum w r^2 <= tol^2 sum w b^2.  For mask 0 every w is 1: the bits of the entry points above.
 *   preconditioner: the constant-coefficient operator of the same edge types, z = V_h ((Vinv_h r VinvT_w) ./ (lam_h + lam_w)) VT_w with the six arrays of
 *             pcnn_fd_poisson_mixed (normalised to V^T W V = I per axis, as dataset/_kernels.py axis_decomposition returns them); the lam = 0 mode is dropped.
 *   mask 15:  setup replaces b by b - (sum w b) / (sum w), the compatibility projection, and b.b is the projected b's; scal[n][6] = sum w b and
 *             scal[n][7] = sum w b^2 of the b as given (0 for other masks).  finish subtracts (sum w x) / (sum w) from x in the workspace before it
 *             writes: the solution with zero trapezoidal integral, whatever mean the initial guess had.
 * Otherwise each entry point is its counterpart above, and refuses a mask outside 0..15 as well.  No atomics; fixed-order reductions. */
int pcnn_varcoef_bc_apply(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const double* p, double* q,
                          double* pq);
size_t pcnn_varcoef_bc_pcg_workspace(int N, int H, int W, int neumann_mask);
int pcnn_varcoef_bc_pcg_setup(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* rhs, const float* left,
                              const float* right, const float* bottom, const float* top, const float* dx, const double* x0, double tol,
                              const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w, const double* VT_w,
                              const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags);
int pcnn_varcoef_bc_pcg_iterate(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, double tol,
                                int first_iteration, int iterations, const double* Vinv_h, const double* V_h, const double* lam_h,
                                const double* VinvT_w, const double* VT_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal,
                                int* flags);
int pcnn_varcoef_bc_pcg_finish(pcnn_handle h, int N, int H, int W, int neumann_mask, void* workspace, const float* left, const float* right,
                               const float* bottom, const float* top, float* soln);
/* g[i] = lo + (hi - lo) min(|g[i]|, 1): a density field from a smooth function scaled to max|g| = 1 (the reference takes 1e-7 + |g|) */
int pcnn_varcoef_density(pcnn_handle h, int64_t total, float lo, float hi, float* g);
/* The smooth profile: g (N x per) -> lo + (hi - lo) (g - min g) / (max g - min g), minimum and maximum per sample by a fixed-order block reduction
 * (two launches, no atomics); a constant sample gives lo.  No kink where g changes sign: the densities the scaled preconditioner below is for. */
int pcnn_varcoef_density_smooth(pcnn_handle h, int N, int64_t per, float lo, float hi, float* g);
/* A (solution, right-hand side) pair of the discrete problem without a solve, one launch:
 *   u[n,i,j]  = sum_{A<ka,B<kb} c[n,A,B] phi_A(x_i) psi_B(y_j),  x = linspace(0,pi,H), y = linspace(0,pi,W), formed in fp64,
 *   soln = (float) u on every node (an exact 0 on a node that is not an unknown),
 *   rhs  = (float) (L_h(rho) u) = -(A u) of pcnn_varcoef_bc_apply on the unknowns of neumann_mask - a Neumann edge's nodes with the doubled inward
 *          face - and 0 elsewhere: the pair satisfies the equation the solve, the loss and the metrics use, to fp32 rounding of the two fields.
 * phi / psi are pcnn_series_pair_synthesis' families chosen by the edge types of the axis - (left, right) = bits 0, 1 for axis -2, (bottom, top) =
 * bits 2, 3 for axis -1: (D,D) sin(A t), (N,N) cos(A t), (D,N) sin((A - 1/2) t), (N,D) cos((A - 1/2) t), A = 1..k - so u = 0 on a Dirichlet edge and
 * is even about a Neumann edge.  With mask 15 u has zero trapezoidal sum and rhs is compatible by construction.  coef (N,ka,kb), ka, kb <= 16;
 * rho (N,H,W) must be positive (not checked, as for pcnn_varcoef_apply); dx (N); H, W >= 3.  u is never rounded before it is differenced.
 * No atomics; a sample's result does not depend on its batch. */
int pcnn_varcoef_series_pair(pcnn_handle h, int N, int H, int W, int ka, int kb, const float* coef, int neumann_mask, const float* rho,
                             const float* dx, float* soln, float* rhs);
/* The solves above with the diagonally scaled preconditioner z = s o M^-1 (s o r) (Concus and Golub): M the constant-coefficient
 * operator of the plain entry points, s = d^-1/2 in fp64, d = diag(A) / diag(M) - the mean of the node's four face coefficients, the inward one twice
 * on a Neumann edge node.  For smooth rho the iteration count then depends on the derivatives of log rho, not on max rho / min rho; for a rho with
 * kinks or jumps it is no better than the plain preconditioner and can be worse: opt-in.  rho = constant gives s = constant, the plain iterates.
 * Arguments, scal, flags and every guarantee are those of the entry points without the suffix: fixed-order reductions, no atomics, results
 * independent of the batch, a flagged sample frozen bit for bit, no dependence on what the workspace held, min rho in scal[n][5].  The workspace
 * holds one more field (s, built by setup): size it with the *_workspace_scaled query.  The same launches per iteration: s o r is written by the
 * pass that updates r, s o z formed by the pass that updates p, and r.z still comes from the division pass.  x and the partial sums lie where the
 * plain layout has them: finish with pcnn_varcoef_pcg_finish / pcnn_varcoef_bc_pcg_finish. */
size_t pcnn_varcoef_pcg_workspace_scaled(int N, int H, int W);
int pcnn_varcoef_pcg_setup_scaled(pcnn_handle h, int N, int H, int W, const float* rho, const float* rhs, const float* left, const float* right,
                                  const float* bottom, const float* top, const float* dx, const double* x0, double tol, const double* S_h,
                                  const double* lam_h, const double* S_w, const double* lam_w, void* workspace, size_t workspace_bytes, double* scal,
                                  int* flags);
int pcnn_varcoef_pcg_iterate_scaled(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, double tol, int first_iteration,
                                    int iterations, const double* S_h, const double* lam_h, const double* S_w, const double* lam_w, void* workspace,
                                    size_t workspace_bytes, double* scal, int* flags);
size_t pcnn_varcoef_bc_pcg_workspace_scaled(int N, int H, int W, int neumann_mask);
int pcnn_varcoef_bc_pcg_setup_scaled(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* rhs, const float* left,
                                     const float* right, const float* bottom, const float* top, const float* dx, const double* x0, double tol,
                                     const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w, const double* VT_w,
                                     const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags);
int pcnn_varcoef_bc_pcg_iterate_scaled(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, double tol,
                                       int first_iteration, int iterations, const double* Vinv_h, const double* V_h, const double* lam_h,
                                       const double* VinvT_w, const double* VT_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                                       double* scal, int* flags);
/* The *_bc_* family with a reaction term: div((1/rho) grad u) - c u = f, on the unknowns (A + C) u = b with C = diag(c).
 * A, b, the Neumann closure and the weights are those above; reaction (N,H,W) fp32 is c on every node, read on the unknowns of neumann_mask only
 * and required >= 0 and finite there.  neumann_mask 0 is the all-Dirichlet problem.  W (A + C) is symmetric, and positive definite once an edge is
 * Dirichlet or c > 0 somewhere.  Each entry point takes the arguments of its counterpart without the suffix, then `reaction` (the workspace query
 * needs no pointer and takes none), and keeps every guarantee: fp64, fixed-order reductions, no atomics, results independent of the batch, a
 * flagged sample frozen bit for bit, no dependence on what the workspace held.
 *   operator: c of the thread's own point joins the point's sum, q = (A + C) p: 24 B per point and product against 20.
 *   setup:    r = b - (A + C) x0.  scal is N x 8 doubles with the layout above, FOLLOWED by N x 4 doubles: [n][0] = cbar, the weighted mean
 *             sum w c / sum w over the unknowns, [n][1] = bbar, the weighted mean of 1 / rho there, [n][2] = min c there, a NaN or an infinity
 *             counting as -inf, [n][3] unused: 12 N doubles in all.  The caller refuses a negative [n][2], and for mask 15 a cbar of 0 (that sample
 *             is singular: solve it without the suffix).
 *   preconditioner: the division is by bbar (lam_h + lam_w) / dx^2 + cbar, the eigenvalues of bbar M + cbar I with M the constant-coefficient
 *             operator including its 1 / dx^2 (a positive factor no longer cancels).  The lam = 0 mode of mask 15 is kept when cbar > 0.
 *   mask 15:  no compatibility projection - scal[n][6] and [n][7] stay 0 - and no mean is removed: finish with pcnn_varcoef_bc_pcg_finish_reaction,
 *             which is pcnn_varcoef_bc_pcg_finish without the mean removal (for masks 0..14 either finish does the same).
 * The workspace holds three more partial-sum arrays: size it with the *_workspace_reaction query.  The scaled preconditioner has no such variant. */
int pcnn_varcoef_bc_apply_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const double* p, double* q,
                                   double* pq, const float* reaction);
size_t pcnn_varcoef_bc_pcg_workspace_reaction(int N, int H, int W, int neumann_mask);
int pcnn_varcoef_bc_pcg_setup_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* rhs, const float* left,
                                       const float* right, const float* bottom, const float* top, const float* dx, const double* x0, double tol,
                                       const double* Vinv_h, const double* V_h, const double* lam_h, const double* VinvT_w, const double* VT_w,
                                       const double* lam_w, void* workspace, size_t workspace_bytes, double* scal, int* flags, const float* reaction);
int pcnn_varcoef_bc_pcg_iterate_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, double tol,
                                         int first_iteration, int iterations, const double* Vinv_h, const double* V_h, const double* lam_h,
                                         const double* VinvT_w, const double* VT_w, const double* lam_w, void* workspace, size_t workspace_bytes,
                                         double* scal, int* flags, const float* reaction);
int pcnn_varcoef_bc_pcg_finish_reaction(pcnn_handle h, int N, int H, int W, int neumann_mask, void* workspace, const float* left, const float* right,
                                        const float* bottom, const float* top, float* soln);
/* pcnn_varcoef_density's map g[i] = lo + (hi - lo) min(|g[i]|, 1) (the same kernel) for a reaction field: 0 <= lo <= hi, lo = 0 allowed */
int pcnn_varcoef_reaction_field(pcnn_handle h, int64_t total, float lo, float hi, float* g);

/* ---- training on the variable-density problem (csrc/varcoef_train.hip) ------------------- */
/* fp32 on one-channel (N,H,W) fields, dx (N) one spacing per sample, rho (N,H,W) read on every node; the discretisation above:
 *   (L u)[i,j] = sum over the four faces of beta_face (u[neighbour] - u[i,j]) / dx^2 = -(A u)[i,j]  on the interior nodes,
 * with the ring of u part of the field.  No atomics; a sample's result does not depend on the batch it sits in; equal inputs give equal bits.
 * out[n] = sum over the interior of (L pred - rhs)^2 (per-tile partials in the handle's auxiliary scratch, then one block per sample). */
int pcnn_varcoef_pi_loss_partials(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                  float* out /*N*/);
/* dpred += coef[n] * d(out[n]) / d(pred) on ALL nodes (the ring is read by L and receives gradient); rho and rhs are data.  dpred aliases no input. */
int pcnn_varcoef_pi_loss_bwd(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                             const float* coef /*N*/, float* dpred);
/* n_sweeps Jacobi sweeps of L u = rhs: u'[i,j] = (sum over the four faces of beta_face u[neighbour] - dx^2 rhs[i,j]) / (sum of the four beta_face)
 * on interior nodes, the ring frozen.  Up to pcnn_varcoef_jacobi_max_sweeps sweeps are fused per launch in LDS; more sweeps chain launches
 * (one intermediate image in the handle's auxiliary scratch) and the result does not depend on the split.  out aliases no input. */
int pcnn_varcoef_jacobi_fwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* u, const float* rhs, const float* dx, int n_sweeps,
                            float* out);
/* the adjoint of those sweeps w.r.t. u: du = J^T dout (rho and rhs get no gradient).  du aliases no input. */
int pcnn_varcoef_jacobi_bwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const float* dout, int n_sweeps, float* du);
int pcnn_varcoef_jacobi_max_sweeps(void);
/* The four operators above with a boundary type per edge (neumann_mask as for pcnn_varcoef_bc_apply: bit 0/1/2/3 set = the
 * left / right / bottom / top edge is Neumann with du/dn = 0).  The unknowns are fd_unknowns(H, W, neumann_mask): a Neumann edge's nodes are unknowns, a
 * Dirichlet edge wins a corner and keeps whatever the field holds there.  At an unknown c
 *   (L u)_c = sum_k m_k beta_k (u_k - u_c) / dx^2,  m = 2 on the inward face of a Neumann edge node in that edge's direction (it has no outward
 * neighbour), 1 otherwise - the half-cell closure of the solver.  With w = w_i w_j, w_i = 1/2 on a Neumann edge's row:
 *   partials: out[n] = sum over the unknowns of w (L pred - rhs)^2;   bwd: dpred += coef[n] * d(out[n]) / d(pred) on all nodes, a gather;
 *   jacobi:   u'_c = (sum_k m_k beta_k u_k - dx^2 rhs_c) / (sum_k m_k beta_k) on the unknowns, Dirichlet nodes frozen;  bwd: its adjoint w.r.t. u.
 * neumann_mask 0 runs the kernels of the entry points above: the same bits.  The same aliasing rules, scratch and sweep fusion; refused: a mask
 * outside 0..15, H or W below 3. */
int pcnn_varcoef_bc_pi_loss_partials(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                     float* out /*N*/, int neumann_mask);
int pcnn_varcoef_bc_pi_loss_bwd(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                const float* coef /*N*/, float* dpred, int neumann_mask);
int pcnn_varcoef_bc_jacobi_fwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* u, const float* rhs, const float* dx, int n_sweeps,
                               float* out, int neumann_mask);
int pcnn_varcoef_bc_jacobi_bwd(pcnn_handle h, int N, int H, int W, const float* rho, const float* dx, const float* dout, int n_sweeps, float* du,
                               int neumann_mask);
/* Gradients with respect to the DATA of the problem (csrc/varcoef_grad.hip): gathers, one thread per output, no atomics, one
 * launch each, a spacing per sample; neumann_mask 0..15 as above, H, W >= 3.  With the system (A u - b)_c = sum_k m_k beta_k (u_c - u_k) / dx^2 + f_c
 * - sum_e 2 g_e / (rho_c dx) on the unknowns and lam (N,H,W) its adjoint variable (A^T lam = d loss / d u on the unknowns, 0 on every other node):
 *   coef_grad: drho_p = sum over the faces (c, k) that touch p of 1/2 beta^2 m lam_c (u_c - u_k) / dx^2 - lam_p sum_e 2 g_e / (rho_p^2 dx) on ALL
 *     nodes, written (not accumulated).  u (N,H,W) is the full field, Dirichlet values included; left / right (N,W), bottom / top (N,H) are the
 *     Neumann data (NULL = 0; a Dirichlet edge's array is not read).  fp32 in, differences and sums in fp64, one rounding.  drho aliases no input.
 *   edge_grad: the gradient of each edge array (NULL: not wanted) - an entry of a Dirichlet edge gets du_d + sum over the node's unknown neighbours
 *     c of lam_c m beta / dx^2 (du (N,H,W) the direct term d loss / d u, NULL = 0), an entry the solution writer overwrites at a corner (bottom /
 *     top at a Dirichlet row 0 / H-1) gets 0; an entry of a Neumann edge gets lam_c 2 / (rho_c dx).  The gradient of f is -lam.
 *   pi_loss_bwd_inputs: the same gradients of coef[n] * pcnn_varcoef_bc_pi_loss_partials[n] w.r.t. rhs and rho (either may be NULL), fused: the
 *     residual r (fp32, the loss's own code) and lam = 2 coef w r stay in LDS.  fp32 throughout.  The outputs alias no input. */
int pcnn_varcoef_bc_coef_grad(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const float* u,
                              const float* lam, const float* left, const float* right, const float* bottom, const float* top, float* drho);
int pcnn_varcoef_bc_edge_grad(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* dx, const float* lam,
                              const float* du /* may be NULL */, float* dleft, float* dright, float* dbottom, float* dtop);
int pcnn_varcoef_bc_pi_loss_bwd_inputs(pcnn_handle h, int N, int H, int W, const float* pred, const float* rho, const float* rhs, const float* dx,
                                       const float* coef /*N*/, float* drhs /* may be NULL */, float* drho /* may be NULL */, int neumann_mask);
/* The backward of pcnn_varcoef_bc_jacobi_fwd with respect to ALL its inputs (csrc/varcoef_train.hip): u0 the field the
 * n_sweeps sweeps started from, dout = d loss / d (their result); du, drho, drhs (N,H,W) are written, each may be NULL (not wanted), all NULL does
 * nothing.  neumann_mask 0 is the all-Dirichlet smoother.  Per sweep u -> u', walking backwards, with g' = d loss / d u', D_c = sum_k m_k beta_k and
 * a_c = g'_c / D_c on the unknowns, 0 on every other node:
 *   du_k = sum over the unknown neighbours c of k of m beta a_c (+ g'_k on a frozen node);   drhs_c += -dx^2 a_c;
 *   drho_p += sum over the faces (c, k) that touch p, c an unknown, of -1/2 beta^2 m a_c (u_k - u'_c)      on ALL nodes.
 * du has the bits of pcnn_varcoef_[bc_]jacobi_bwd (which runs when du alone is wanted).  With drho or drhs the n_sweeps iterates are recomputed by
 * the forward's kernel, one sweep per launch, and kept with two gradient fields in the handle's auxiliary scratch -
 * pcnn_varcoef_jacobi_bwd_inputs_workspace bytes, (n_sweeps + 2) N H W floats (0 for arguments the call refuses) -, then one gather launch per
 * sweep: one thread per output, no atomics, equal inputs give equal bits.  fp32 throughout.  No output aliases an input or another output. */
int pcnn_varcoef_bc_jacobi_bwd_inputs(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* rho, const float* u0, const float* rhs,
                                      const float* dx, const float* dout, int n_sweeps, float* du /* may be NULL */, float* drho /* may be NULL */,
                                      float* drhs /* may be NULL */);
size_t pcnn_varcoef_jacobi_bwd_inputs_workspace(int N, int H, int W, int n_sweeps);
/* out[n,y,x,0:2] = {stack[n,0,y,x], stack[n,1,y,x]} of the generator's (N,2,H,W) stack [rhs, rho], followed - use_pos - by the two positional
 * channels of pcnn_assemble_input; ldo >= 2 (4 with use_pos). */
int pcnn_assemble_density_input(pcnn_handle h, int N, int H, int W, const float* stack, int use_pos, float* out, int ldo);
/* Error statistics of a prediction of the variable-density problem in one pass over the four fields (csrc/error_stats.hip: the kernel of
 * pcnn_error_stats with the flux-form residual of csrc/flux_form.h, the one pcnn_varcoef_pi_loss_partials sums).  out[8n..8n+7] has the layout of pcnn_error_stats, {sum|e|, sum e^2, max|e|, sum t^2, max|t|, sum r^2, max|r|, sum f^2}: e = pred - target
 * and t = target over all H W points; f = rhs[i,j] and
 *   r[i,j] = (L pred)[i,j] - rhs[i,j],  L the flux-form operator above with dx[n], pred's own edge values as the Dirichlet neighbours,
 * over the (H-2)(W-2) interior points, in fp32.  With zero edge values - and only then - sum r^2 / sum f^2 is ||b - A x||^2 / ||b||^2 of the
 * conjugate-gradient solve.  target == NULL: the first five entries are 0; rhs == NULL: the last three are 0 and rho, dx are not read; rhs needs
 * rho, dx and H, W >= 3.  Two launches, no atomics, partials in the handle's scratch, a fixed order: equal inputs give equal bits. */
int pcnn_varcoef_error_stats(pcnn_handle h, int N, int H, int W, const float* pred, const float* target /* may be NULL */,
                             const float* rho /* required with rhs */, const float* rhs /* may be NULL */,
                             const float* dx /* N; required with rhs */, float* out /* N x 8 */);
/* pcnn_varcoef_error_stats with per-edge Neumann boundaries (neumann_mask 0..15, bits as above).  Entries 0..4 are the same.
 * The residual's domain is the unknowns of the mask - the interior plus the nodes of every Neumann edge, a Dirichlet edge wins a corner - and r
 * there is the same fp32 flux-form residual with the neighbour beyond a Neumann edge read at its mirrored index, for pred and rho alike (du/dn = 0,
 * the inward face counts twice: the r of pcnn_varcoef_bc_pi_loss_partials); beyond a Dirichlet edge pred's own edge value is the neighbour.
 * out[8n+5] = sum w r^2 and out[8n+7] = sum w f^2 with w = 1/2 per Neumann edge the unknown lies on; out[8n+6] = max|r|, unweighted.  Mask 0
 * gives the bits of pcnn_varcoef_error_stats.  The same NULL rules, launches and fixed orders. */
int pcnn_varcoef_bc_error_stats(pcnn_handle h, int N, int H, int W, int neumann_mask, const float* pred, const float* target /* may be NULL */,
                                const float* rho /* required with rhs */, const float* rhs /* may be NULL */,
                                const float* dx /* N; required with rhs */, float* out /* N x 8 */);

/* tf.keras.layers.LayerNormalization() over the last axis of an (N, F) matrix (epsilon 1e-3 in Keras): the optional final layer of the
 * metalearning hyper-networks (layers/metalearning_conv.py:128-129).  fwd also returns the per-row mean and 1/sqrt(var + eps) in float32: bwd forms dgamma
 * with them, and forms dx from x and the SAME eps with the row statistics in double (dx can be a small remainder of large terms). */
int pcnn_layernorm_fwd(pcnn_handle h, int N, int F, const float* x, const float* gamma, const float* beta, float eps, float* y, float* mean, float* rstd);
int pcnn_layernorm_bwd(pcnn_handle h, int N, int F, const float* x, const float* gamma, const float* mean, const float* rstd, const float* dy,
                       float eps, float* dx, float* dgamma, float* dbeta);

/* Row softmax of an (N, F) matrix - the 'softmax' activation of a tf.keras Dense layer (models/Dirichlet_BC_NN_Metalearning.py:69-76, its
 * __main__ config :236-239) - and its backward dx = y (dy - sum_f dy y).  dx may alias dy. */
int pcnn_softmax_fwd(pcnn_handle h, int N, int F, const float* x, float* y);
int pcnn_softmax_bwd(pcnn_handle h, int N, int F, const float* y, const float* dy, float* dx);

/* ---- Dirichlet_BC_NN_Legacy_2 / Poisson_CNN_Legacy (kernels in csrc/dbcnn.hip) ------------------------------ */
/* out[n,y,0:3] = {bc[n,y], 1, cos(pi y/(L-1))}: the boundary input with its positional embeddings
 * (models/Dirichlet_BC_NN_Legacy.py:113-124,136-139); 1-D tensors are NHWC with H = 1 */
int pcnn_dbc_assemble_input(pcnn_handle h, int N, int L, const float* bc, float* out, int ldo);
/* Spatial pyramid AVERAGE pool over channels and spatial bins (layers/SpatialPyramidPool.py:10-11,35-66); bins as pcnn_spp_max_fwd */
int pcnn_spp_avg_fwd(pcnn_handle h, int N, int H, int W, int C, int ldx, int nb, const int32_t* bins, const float* x, float* out);
int pcnn_spp_avg_bwd(pcnn_handle h, int N, int H, int W, int C, int lddx, int nb, const int32_t* bins, const float* dout, float* dx);
/* tf.einsum('bmy,mx,bm->bmxy', f, sinh_table, d) written as NHWC (N,X,L,M+2) with the two positional-embedding channels
 * cos(pi x/(X-1)), cos(pi y/(L-1)) appended (models/Dirichlet_BC_NN_Legacy.py:150-156).  f: (N,L,M) stride ldf; sinh_table (M,X); d (N,M) */
int pcnn_dbc_expand_fwd(pcnn_handle h, int N, int X, int L, int M, const float* f, int ldf, const float* sinh_table, const float* d, float* out, int ldo);
size_t pcnn_dbc_expand_bwd_workspace(int N, int L, int M);
int pcnn_dbc_expand_bwd(pcnn_handle h, int N, int X, int L, int M, const float* dout, int lddo, const float* f, int ldf, const float* sinh_table,
                        const float* d, float* df, int lddf, float* dd, void* workspace, size_t workspace_bytes);
/* adjoint of pcnn_set_max_magnitude (dataset/utils/set_max_magnitude.py:14-25 inside a GradientTape): x = the UNSCALED input */
int pcnn_set_max_magnitude_bwd(pcnn_handle h, int N, int64_t per, const float* target, const float* x, const float* dy, float* dx);
/* y[n,0,:] = bc[n,:] (bc == NULL: zeros = the adjoint): tf.concat([expand_dims(bc), out[...,1:,:]], 2) (models/Dirichlet_BC_NN_Legacy.py:164) */
int pcnn_set_first_row(pcnn_handle h, int N, int X, int L, const float* bc, float* y);
/* flip_and_rotate_tensor for (N,H,W) fields (dataset/utils/flip_and_rotate_tensor.py:4-47): out = reverse(transpose?(in)) along the flagged
 * axes, scaled per sample by alpha[n] (NULL = 1) and optionally accumulated into out (the five-term sum of models/Poisson_CNN_Legacy.py:48) */
int pcnn_flip_rotate(pcnn_handle h, int N, int Ho, int Wo, int transpose, int flip_y, int flip_x, const float* in, const float* alpha,
                     int accumulate, float* out);

/* ---- recurrent layers of Dirichlet_BC_RNN (models/Dirichlet_BC_RNN.py:24-30,46-48; kernels in csrc/rnn.hip) -------------------------------
 * tf.keras.layers.LSTM / GRU(units, activation, return_sequences=True, time_major=False), zero initial state, TF 2 semantics:
 *   LSTM  z = x W + h U + b, gate blocks i, f, c~, o:  c' = rec(f) c + rec(i) act(c~),  h' = rec(o) act(c')
 *   GRU (reset_after=True), blocks z, r, h~, bias (2, 3u):  mx = x W + b[0], mh = h U + b[1],
 *         z = rec(mx_z + mh_z), r = rec(mx_r + mh_r), h~ = act(mx_h + r mh_h),  h' = z h + (1 - z) h~
 * The time-parallel products (x W + b for all t; dX, dW, dU, db in the backward) are 1x1 convolutions over the N T rows: pcnn_wide_conv2d_*.
 * The two calls below are the dependent chain: ONE kernel launch for the whole sequence, one workgroup per sample (no cooperation between
 * workgroups), U held in registers, exact fp32 FMAs in a fixed order in every math mode, no atomics, no allocation, no synchronisation.
 * Every (N, T, C) tensor is addressed as base + n * sn + t * ld + c (floats).  reverse = go_backwards: step s reads its input at position
 * T - 1 - s; outputs stay in processing order (Keras does not flip them back).  1 <= units <= PCNN_RNN_MAX_UNITS. */
enum { PCNN_RNN_LSTM = 0, PCNN_RNN_GRU = 1 };
enum { PCNN_RNN_ACT_LINEAR = 0, PCNN_RNN_ACT_TANH = 1, PCNN_RNN_ACT_SIGMOID = 2, PCNN_RNN_ACT_RELU = 3 };   /* the layer's `activation` */
enum { PCNN_RNN_SIGMOID = 0, PCNN_RNN_HARD_SIGMOID = 1 };   /* `recurrent_activation`; hard_sigmoid = clip(0.2 x + 0.5, 0, 1) */
enum { PCNN_RNN_MAX_UNITS = 128 };
typedef struct {
  int cell, N, T, units;
  int act, rec_act, reverse;
  int64_t sn_zx; int ld_zx;       /* projected gates x W + b (N, T, G units), G = 4 (LSTM) / 3 (GRU), indexed by INPUT position */
  int64_t sn_h; int ld_h;         /* h (N, T, units), processing order */
  int64_t sn_h2; int ld_h2;       /* optional second copy of h (forward) */
  int64_t sn_dh; int ld_dh;       /* incoming dL/dh_s (N, T, units), processing order (backward) */
  int64_t sn_dzx; int ld_dzx;     /* dL/d(x W + b) (N, T, G units), by INPUT position (backward) */
  int64_t sn_dzh; int ld_dzh;     /* dL/d(h U [+ b1]) (N, T, G units), processing order (backward) */
} pcnn_rnn_desc;
/* floats of `saved` = N T (G + 1) units: per step the activated gates and c' (LSTM) or (h U + b1)_h (GRU), dense */
size_t pcnn_rnn_saved_floats(const pcnn_rnn_desc* d);
/* The recurrence of LSTM.call / GRU.call (models/Dirichlet_BC_RNN.py:46-48).  U (units, G units) Keras recurrent_kernel; rbias: the GRU's
 * b[1] (3 units) or NULL; hout2: NULL or a second destination of h (e.g. the dense image the Upsample layer reads, :50-52). */
int pcnn_rnn_fwd(pcnn_handle h, const pcnn_rnn_desc* d, const float* zx, const float* U, const float* rbias, float* hout, float* hout2,
                 float* saved);
/* Its gradient under the GradientTape of models/Dirichlet_BC_RNN.py:66-70: from dh (the gradient of every h_s) to dzx and dzh; these feed
 * pcnn_wide_conv2d_dgrad (dX) and pcnn_wide_conv2d_wgrad (dW, db from dzx with x; dU, db[1] from dzh with h_{s-1}).  dzh may be the same
 * buffer as dzx for an LSTM with reverse = 0 (the two are then equal). */
int pcnn_rnn_bwd(pcnn_handle h, const pcnn_rnn_desc* d, const float* U, const float* saved, const float* hout, const float* dh, float* dzx,
                 float* dzh);

#ifdef __cplusplus
}
#endif
#endif
