/*
 * percival_hip.h -- C ABI of libpercival_hip.so (gfx950 / MI355X).
 *
 * This is the drop-in boundary "B2" of SURVEY.md section 8(b): the arithmetic that the
 * reference delegates to TensorFlow/Keras on its WGAN-GP training hot path
 * (reference: percivaltts/optimizertts_wgan.py:107-241, networks_critic.py:44-96,
 * modeltts_common.py:65-126, networktts.py:59-134) is provided here as hand-written HIP
 * kernels.  The reference has no FFI of its own (it is pure Python on tf.keras), so each
 * entry point cites the Keras call site it replaces.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no framework types.
 *   - every pointer is a DEVICE pointer unless the name ends in _host.
 *   - every function is asynchronous on `stream` (a hipStream_t passed as void*),
 *     never allocates or frees, never synchronises, and is safe to capture in a hipGraph.
 *   - return value: 0 = ok, negative = PTTS_E* (see ptts_last_error()).
 *   - tensors are fp32, channel-last, C-contiguous:
 *       frames      [B, T, D]
 *       conv2d maps [B, T, F, C]           (Keras channels_last)
 *       conv2d kernels [KT, KF, Cin, Cout] (Keras HWIO)
 *       dense / conv1d kernels [K, N] resp. [KW, Cin, N]  (Keras layout)
 *   - "input transform": the layers of the reference are Linear -> (BatchNorm) -> LeakyReLU
 *     (networktts.py:59-63,116-126).  We keep the PRE-activation tensor z in HBM and apply
 *     a = act(scale*z + shift) while the next linear op loads it, so an activation is never
 *     written and re-read.  PTTS_IN_* selects that transform.
 */
#ifndef PERCIVAL_HIP_H
#define PERCIVAL_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTTS_OK            0
#define PTTS_EINVAL       -1   /* bad argument / unsupported shape */
#define PTTS_ELAUNCH      -2   /* hipLaunch failed */
#define PTTS_EWORKSPACE   -3   /* workspace too small */
#define PTTS_EDEVICE      -4   /* a kernel reported a failed hand-off (sticky device status word, see ptts_device_status) */

/* input transforms (applied on load; x is what lies in HBM) */
#define PTTS_IN_NONE     0   /* a = x                                   */
#define PTTS_IN_LRELU    1   /* p = x*scale[c]+shift[c]; a = p>0?p:alpha*p  (scale/shift may be NULL) */
#define PTTS_IN_MASKMUL  2   /* a = x * (mask_src>0 ? 1 : alpha)        (second-order sweep of the gradient penalty) */

/* conv2d padding modes along time (frequency is always 'same') */
#define PTTS_PAD_SAME    0
#define PTTS_PAD_CAUSAL  1

/* output activations of ptts_affine_act */
#define PTTS_ACT_NONE    0
#define PTTS_ACT_LRELU   1
#define PTTS_ACT_SIGMOID 2
#define PTTS_ACT_TANH    3

const char* ptts_version(void);
const char* ptts_device_arch(void);     /* "gfx950" : the only code object in the library */
const char* ptts_last_error(void);      /* thread-local message of the last failure */
/* Device status.  Kernels whose waves wait for each other with bounded polls (the wave-specialised Conv2D forward's LDS-counter
 * hand-off) do not hang when a count never arrives -- and do not stay silent either: the
 * wave that gave up stores a code into a block of pinned, device-mapped host memory.  The word is STICKY: ptts_device_status()
 * returns PTTS_EDEVICE (message in ptts_last_error(), bit mask in *word_out: 1 = Conv2D hand-off, 2 = reserved, formerly the
 * persistent LSTM's hand-off) from then on, and so does every later ptts_conv2d_mfma_fwd call, until ptts_device_status_clear().  Reading it is a host
 * memory load (no synchronisation): call it at step boundaries.  The reference has no counterpart (TF raises from Session.run,
 * optimizertts.py:254 turns a NaN cost into a ValueError); this is how a corrupted launch becomes an error instead of a bad step.
 * ptts_device_status_word() returns the HOST address of the first word (tests poke it to exercise the host logic without a GPU);
 * ptts_device_status_message() decodes a mask. */
int ptts_device_status(unsigned* word_out);
int ptts_device_status_clear(void);
unsigned* ptts_device_status_word(void);
int ptts_device_status_message(unsigned word, char* buf, size_t n);
/* Deterministic mode: reductions over workgroups in a fixed order only (no fp32 atomics: stream-K GEMM tiles, the
 * thin weight-gradient kernel and the loss scalars take their single-pass forms).  Returns the previous setting. */
int ptts_set_deterministic(int on);
int ptts_get_deterministic(void);
/* bf16 products (BASELINE configs[2]; the reference is fp32, README.md:166): the split GEMM kernels -- ptts_conv1d_bf16x6,
 * ptts_conv1d_wgrad_bf16x6, ptts_dense_bf16x6, ptts_dense_wgrad_bf16x6* -- form ONE product of the operands' bf16 roundings
 * (plane 1 of the split) instead of the six products of the fp32 split; fp32 accumulation, fp32 master weights and
 * gradients.  Returns the previous setting. */
int ptts_set_bf16_products(int on);
int ptts_get_bf16_products(void);

/* ---------------------------------------------------------------------------------------
 * 2D convolution over (time x frequency), NHWC, stride 1.
 * Replaces kl.Conv2D at networks_critic.py:67, networktts.py:123,129-130, modeltts_common.py:100.
 *   y[b,t,f,:] = bias + sum_{kt,kf} a[b, t+kt*dil_t-pad_t, f+kf-pad_f, :] . w[kt,kf,:,:]
 *   a = transform(x) inside the image, 0 outside ('same' zero padding is in the activation domain).
 * ------------------------------------------------------------------------------------- */
int ptts_conv2d_fwd(const float* x, const float* w, const float* bias /*[Cout] or NULL*/,
                    const float* in_scale /*[Cin] or NULL*/, const float* in_shift /*[Cin] or NULL*/,
                    const float* mask_src /*[B,T,F,Cin], PTTS_IN_MASKMUL only*/,
                    float* y,
                    int B, int T, int F, int Cin, int Cout, int KT, int KF,
                    int dil_t, int pad_mode, int in_mode, float alpha, void* stream);

/* Fused backward of the layer above: given dy = dL/dy and the same (x, transform) as the forward,
 *   da = conv^T(dy, w);  dx = da * d(a)/d(x)          -> dx   (skipped when dx == NULL)
 *   dw = corr(a, dy), dbias = sum dy                  -> dw, dbias (skipped when dw == NULL)
 *   dscale[c] = sum da*lrelu'(p)*x ; dshift[c] = sum da*lrelu'(p)   (PTTS_IN_LRELU with scale; skipped when NULL)
 * One pass over HBM: reads dy, x (and mask_src), writes dx.  Weight-shaped results are reduced
 * deterministically through `workspace` (ptts_conv2d_bwd_workspace_bytes) -- no float atomics. */
size_t ptts_conv2d_bwd_workspace_bytes(int B, int T, int F, int Cin, int Cout, int KT, int KF, int dil_t);
int ptts_conv2d_bwd(const float* dy, const float* x, const float* w,
                    const float* in_scale, const float* in_shift, const float* mask_src,
                    float* dx, float* dw, float* dbias, float* dscale, float* dshift,
                    void* workspace, size_t workspace_bytes,
                    int B, int T, int F, int Cin, int Cout, int KT, int KF,
                    int dil_t, int pad_mode, int in_mode, float alpha, void* stream);

/* The same pass with the weight-shaped sums left unreduced: dx as above (NULL to skip), and the per-workgroup partial sums
 * of dw / dbias as rows [nblocks][npart] (npart = KT*KF*Cin*Cout + Cout + 2*Cin) behind a 4096-byte head of the caller's
 * workspace; *nblocks_out receives nblocks.  Only for shapes with a tiled kernel (workspace_bytes > 16) and without a
 * BatchNorm-fused input.  ptts_conv2d_reduce_grouped then adds up to any number of such passes into their gradient
 * buffers (dw[nw], dbias[cout]; fp32 atomics: several passes may share a buffer) in one launch per 16 passes -- the
 * 8 layers x 3 passes of a critic step otherwise pay one 7 us reduction launch each. */
int ptts_conv2d_bwd_partials(const float* dy, const float* x, const float* w, const float* mask_src,
                             float* dx, void* workspace, size_t workspace_bytes, int* nblocks_out,
                             int B, int T, int F, int Cin, int Cout, int KT, int KF,
                             int dil_t, int pad_mode, int in_mode, float alpha, void* stream);
typedef struct ptts_conv2d_reduce_desc {
    const float* partials;      /* workspace + 4096 bytes */
    int nblocks, npart, nw, cout;
    float* dw; float* dbias;    /* accumulated into; either may be NULL */
} ptts_conv2d_reduce_desc;
int ptts_conv2d_reduce_grouped(const ptts_conv2d_reduce_desc* descs, int n, void* stream);

/* ---------------------------------------------------------------------------------------
 * The same convolution for the wide and non-square layers -- Cin and Cout each 1 or a multiple of 4 up to 16, KT and KF each
 * odd in 3 .. 7 and chosen independently, any dilation whose tile fits the LDS -- as implicit GEMMs on the fp32-input matrix
 * instruction (csrc/conv2d_wide.hip; exact fp32, the tolerances of the fp32 stencil).  Same semantics as ptts_conv2d_fwd /
 * ptts_conv2d_bwd.  Shapes the packed-FMA stencil or the 4 -> 4 5x5 matrix-core kernels take are NOT supported here.
 *   ptts_conv2d_wide_supported     1 where the entry points below take the shape; anywhere else they return PTTS_EINVAL and
 *                                  launch nothing.  x, dy, mask_src, in_scale and in_shift must be 16-byte aligned.
 *   ptts_conv2d_wide_fwd           y = bias + conv(transform(x), w)
 *   ptts_conv2d_wide_bwd_partials  dx (NULL to skip; includes lrelu'(p) and scale) and, where want_dw / want_affine, per-workgroup
 *                                  partial sums as rows [*nblocks_out][*npart_out] at the START of the workspace (no head), a row =
 *                                  dw (KT*KF*Cin*Cout) | dbias (Cout) | dscale (Cin) | dshift (Cin); columns not asked for are
 *                                  undefined.  ptts_conv2d_reduce_grouped adds them up.  At most 256 rows in deterministic mode.
 *   ptts_conv2d_wide_bwd_workspace_bytes   bytes of those rows (0 for an unsupported shape)
 * ------------------------------------------------------------------------------------- */
int ptts_conv2d_wide_supported(int F, int Cin, int Cout, int KT, int KF, int dil_t);
int ptts_conv2d_wide_fwd(const float* x, const float* w, const float* bias, const float* in_scale, const float* in_shift,
                         const float* mask_src, float* y, int B, int T, int F, int Cin, int Cout, int KT, int KF,
                         int dil_t, int pad_mode, int in_mode, float alpha, void* stream);
size_t ptts_conv2d_wide_bwd_workspace_bytes(int B, int T, int F, int Cin, int Cout, int KT, int KF, int dil_t);
int ptts_conv2d_wide_bwd_partials(const float* dy, const float* x, const float* w, const float* in_scale, const float* in_shift,
                                  const float* mask_src, float* dx, void* workspace, size_t workspace_bytes,
                                  int* nblocks_out, int* npart_out, int want_dw, int want_affine,
                                  int B, int T, int F, int Cin, int Cout, int KT, int KF,
                                  int dil_t, int pad_mode, int in_mode, float alpha, void* stream);

/* ---------------------------------------------------------------------------------------
 * The same convolution for the 4 -> 4 channel, 5x5 layers (the critic's stack, networks_critic.py:66-68, and the
 * generator's, networktts.py:122-126) on the bf16 matrix cores, in fp32 arithmetic: both operands are split three ways
 * into bf16 (x = x1 + x2 + x3 exactly), the six products of order >= 2^-16 are formed by v_mfma_f32_16x16x32_bf16 and
 * accumulated in fp32 (csrc/conv2d_mfma.hip).  Time dilation 1, 2, 4 or 8; any T, F, B.
 *   ptts_conv2d_mfma_tables   the banded (Toeplitz) operand tables of a kernel w [5,5,4,4], 3 bf16 planes each
 *                             (ptts_conv2d_mfma_table_bytes(5) bytes): table_fwd for the forward, table_bwd (flipped,
 *                             transposed) for the backward-data pass; either may be NULL.  Rebuild when w changes.
 *   ptts_conv2d_mfma_fwd      y = bias + conv(transform(x)) with pad_t rows of zero padding before t = 0; when out_mask
 *                             is given, y *= (out_mask > 0 ? 1 : alpha).  Forward: table_fwd, pad_t = 2 dil ('same') or
 *                             4 dil (causal).  Masked forward of the second-order sweep: in_mode PTTS_IN_MASKMUL.
 *                             Backward data: x = dy, table_bwd, pad_t = 4 dil - pad_t(forward), out_mask = the forward
 *                             layer's pre-activation input (its LeakyReLU mask), in_mode PTTS_IN_NONE.
 *   ptts_conv2d_mfma_wgrad_partials   per-workgroup partial sums of dw / dbias in the row layout of
 *                             ptts_conv2d_bwd_partials (rows of *npart_out floats behind a 4096-byte head), reduced in a
 *                             fixed order inside a workgroup (no atomics); ptts_conv2d_reduce_grouped adds them up.
 *   ptts_conv2d_mfma_debug    measurement hook of tools/conv2d_mfma_probe.py (phase switches, per-workgroup stamps);
 *                             flags 0 = the product path; bit 16 alone keeps the results and launches the four-wave form of
 *                             the dilation-1 fp32 forward kernel instead of the wave-specialised default (A/B in tests).
 * ------------------------------------------------------------------------------------- */
int ptts_conv2d_mfma_supported(int F, int Cin, int Cout, int KT, int KF, int dil_t);
size_t ptts_conv2d_mfma_table_bytes(int KT);
int ptts_conv2d_mfma_tables(const float* w, void* table_fwd, void* table_bwd, int KT, int KF, int Cin, int Cout,
                            int planes /*3: fp32 split, 1: bf16 copy of the kernel*/, void* stream);
/* The same for n kernels (5x5, 4 -> 4) in one launch: w[i] -> table_fwd[i], table_bwd[i] (host arrays of device pointers). */
int ptts_conv2d_mfma_tables_grouped(const float* const* w, void* const* table_fwd, void* const* table_bwd, int n, int planes,
                                    void* stream);
/* planes = 3: fp32 arithmetic (six products), every tensor fp32.  planes = 1: bf16 arithmetic (BASELINE configs[2]; time
 * dilation 1): ONE product per position with the bf16 copy of the kernel, fp32 accumulation; x and mask_src are bf16 in
 * HBM when in_bf16 (else fp32, rounded to bf16 on load), y and out_mask are bf16 when out_bf16 (else fp32). */
int ptts_conv2d_mfma_fwd(const void* x, const void* table, const float* bias, const float* in_scale, const float* in_shift,
                         const void* mask_src, const void* out_mask, void* y,
                         int B, int T, int F, int KT, int dil_t, int pad_t, int in_mode, float alpha,
                         int planes, int in_bf16, int out_bf16, void* stream);
/* The same forward pass (fp32 maps, dilation 1, in_mode NONE / LRELU with or without the BatchNorm affine) that ALSO leaves the
 * per-workgroup sums of the outputs it stores -- stats[*nrows_out][8] doubles: four channel sums, four channel sums of squares -- for
 * the kl.BatchNormalization that follows the kl.Conv2D in pCNN2D (networktts.py:122-126): TF computes the layer's batch moments with a
 * pass of its own over the map (FusedBatchNorm); here they ride on the convolution's stores and ptts_bn_finalize_partials finishes
 * them.  capacity_rows >= 256.  y is bit-identical to ptts_conv2d_mfma_fwd's. */
int ptts_conv2d_mfma_fwd_stats_supported(int F, int dil_t, int in_mode);
int ptts_conv2d_mfma_fwd_stats(const float* x, const void* table, const float* bias, const float* in_scale, const float* in_shift,
                               float* y, int B, int T, int F, int KT, int pad_t, int in_mode, float alpha,
                               double* stats, int capacity_rows, int* nrows_out, void* stream);
size_t ptts_conv2d_mfma_wgrad_workspace_bytes(int B, int T);
/* x (and mask_src) bf16 when x_bf16, dy bf16 when dy_bf16; the partial sums and the reduced gradients are fp32 always. */
int ptts_conv2d_mfma_wgrad_partials(const void* dy, const void* x, const void* mask_src, void* workspace,
                                    size_t workspace_bytes, int* nblocks_out, int* npart_out, int B, int T, int F,
                                    int KT, int dil_t, int pad_t, int in_mode, float alpha,
                                    int planes, int x_bf16, int dy_bf16, void* stream);
/* Fused backward launches (round 4; dilation 1, 'same' padding, fp32 maps): the two passes of a layer that read the same staged tile
 * as ONE launch -- what TF runs as Conv2DBackpropInput + Conv2DBackpropFilter (+ BiasAddGrad) of one kl.Conv2D (networks_critic.py:67),
 * and, for the gradient penalty (optimizertts_wgan.py:53-68), the forward + Conv2DBackpropFilter pair of the backward of
 * Conv2DBackpropInput:
 *   kind 1  p = dy, q = x (the layer's pre-activation input), table = table_bwd:  y = dx = conv^T(dy) . lrelu'(x), and the partial
 *           rows of dw = corr(lrelu(x), dy), dbias = sum dy
 *   kind 2  p = u with mask_src = x, q = dy, table = table_fwd:  y = conv(u . lrelu'(x)), and the partial rows of
 *           dw = corr(u . lrelu'(x), dy) (bias sums zero)
 * pad_t is the forward layer's (2).  y is bit-identical to ptts_conv2d_mfma_fwd's; the partial rows (one per workgroup, behind a
 * 4096-byte head, *npart_out floats each) go to ptts_conv2d_reduce_grouped like ptts_conv2d_mfma_wgrad_partials'. */
size_t ptts_conv2d_mfma_bwd_fused_workspace_bytes(int B, int T);
int ptts_conv2d_mfma_bwd_fused_supported(int F, int dil_t, int planes);
int ptts_conv2d_mfma_bwd_fused(const void* p, const void* q, const void* mask_src, const void* table, void* y,
                               void* workspace, size_t workspace_bytes, int* nblocks_out, int* npart_out,
                               int B, int T, int F, int KT, int pad_t, int kind, float alpha, void* stream);
/* Kind 1 for a layer whose input was lrelu(scale x + shift) -- the kl.BatchNormalization + kl.LeakyReLU in front of the generator's
 * kl.Conv2D layers (networktts.py:122-126): q = the raw map x, y = dx = conv^T(dy) lrelu'(scale x + shift) scale (TF: Conv2DBackpropInput +
 * LeakyReluGrad + the input half of FusedBatchNormGrad's elementwise stage), and every partial row carries, behind the 400 + 4 sums of
 * dw / dbias, the 4 + 4 sums that are the gradients of scale and shift (columns 404 .. 411: a second ptts_conv2d_reduce_desc with
 * partials + 404 floats, nw = 4, cout = 4 reduces them). */
int ptts_conv2d_mfma_bwd_fused_affine(const float* p, const float* q, const void* table, float* y, void* workspace, size_t workspace_bytes,
                                      int* nblocks_out, int* npart_out, int B, int T, int F, int KT, int pad_t, float alpha,
                                      const float* q_scale, const float* q_shift, void* stream);
int ptts_conv2d_mfma_debug(int flags, void* stamp_buf);

/* ---------------------------------------------------------------------------------------
 * The critic's WHOLE Conv2D stack per launch (csrc/conv2d_chain.hip; BASELINE configs[2]: bf16 storage, bf16 products,
 * fp32 accumulation, fp32 master weights and weight gradients).  Replaces the L x (kl.Conv2D 5x5 + kl.LeakyReLU) of
 * networks_critic.py:64-70 -- forward, TF's Conv2DBackpropInput / Conv2DBackpropFilter chains behind it, and the
 * second-order sweep of K.gradients(K.gradients(...)) (optimizertts_wgan.py:53-68) -- with the maps between the layers
 * held in the LDS: a workgroup carries a tile of 32 time rows x up to 68 bins through all L <= 8 layers (two halo rows
 * per layer and side, recomputed).  Spectra wider than 68 bins run in overlapping frequency blocks of one tile each: block
 * origins and the cuts between the bins that blocks own are multiples of 8 bins, a block owns no bin within 2 L bins of a
 * cut (recomputed by its neighbour), and only owned bins are stored or summed (ptts_conv2d_chain_blocks tells the plan).
 * F <= 68 is one block: the kernels without any block state.  Channels: cin0 (1) -> 4 -> ... -> 4.
 *   maps     a_1 .. a_{L-1} = lrelu(z_l), POST-activation, [L-1][B][T][FP][4] bf16, FP = F rounded up to even, pad bin zero
 *            (ptts_conv2d_chain_map_elems(B, T, F) elements each);   a_last = a_L [B][T][F][4] bf16 (what the dense layers read)
 *   tables   ptts_conv2d_chain_tables_bytes() bytes: the banded operand tables of all layers, both directions (bf16 copies
 *            of the kernels) and the biases; rebuild when a kernel changes.  w / b are HOST arrays of L device pointers.
 *   _fwd       x0 [B][T][ldx] fp32 (the first F values of a row are the spectrum) -> maps, a_last
 *   _bwd       d_last = dL/da_L [B][T][F][4] (fp32, or bf16 when d_bf16) -> per-workgroup partial sums of dW_l / db_l as rows
 *              [L][*nblocks_out][*npart_out] (a row of layer l: KT*KF*Cin_l*4 kernel entries, then 4 bias entries) for
 *              ptts_conv2d_reduce_grouped; fixed summation order (no atomics)
 *   _bwd_data  the backward-data chain alone: g0 = d/dx0 [B][T][F] fp32 (may be NULL) and, when gmaps is given, the masked
 *              gradient maps gamma_l = lrelu'(a_l) . dL/da_l, l = 1 .. L, [L][B][T][FP][4] bf16 (operands of _second)
 *   _second    the backward of _bwd_data w.r.t. d_last and the kernels: u0 = d/d(g0) [B][T][F] fp32 -> out = d/d(d_last)
 *              [B][T][F][4] (fp32 / bf16) and the partial sums of dW_l (rows as _bwd, bias entries zero)
 * The per-row form, ptts_conv2d_chain_{fwd,bwd,bwd_data,second}_rows: the same passes over a ZERO-PADDED batch.  The arguments
 * of the plain entry point plus `lengths` (device int32 [B], in front of B; NULL is PTTS_EINVAL): utterance b holds
 * n_b = min(max(lengths[b], 0), T) real rows.  n_b is the row limit of a tile of utterance b wherever the plain kernels test a
 * row against T; T stays the pitch of every address.  The rule:
 *   - every layer sees zeros at t >= n_b: the input, every map a_l, every gradient map d_l / gamma_l and every u_l are zero
 *     there before the next layer reads them (a pad row whose convolution would give lrelu(bias) included);
 *   - the pad rows of x0, d_last, u0, maps and gmaps are never looked at (a loader selects a zero in their place and never
 *     multiplies): they may hold anything, NaN included;
 *   - EVERY row 0 .. T-1 of every output is written -- maps, a_last, gmaps, g0, out: real rows as computed, pad rows as +0.0,
 *     whatever the buffer held (consumers such as ptts_gp_sqnorm and the dense layers' weight gradients read them without lengths);
 *   - the sums of dW_l / db_l run over real rows only.
 * A real row equals, bit for bit, what the plain entry point gives for utterance b alone at T = n_b; with every n_b = T every
 * output, partial rows included, equals the plain entry point's.
 * ------------------------------------------------------------------------------------- */
/* 1 when the stack has a chain kernel: 2 <= F <= 1024 bins (run on the device up to 200), 1 <= L <= 8 layers, 1 <= Cin0 <= 4,
 * C = 4 filters of 5 x 5 */
int ptts_conv2d_chain_supported(int F, int L, int Cin0, int C, int KT, int KF);
/* host only (tests, tools): the frequency blocks of a launch.  Block k computes bins [origin[k], origin[k] + min(68, F - origin[k]))
 * and owns [own_lo[k], own_hi[k]).  Returns the block count (the arrays receive the first `cap` blocks and may be NULL), or 0
 * when ptts_conv2d_chain_supported says no. */
int ptts_conv2d_chain_blocks(int F, int L, int* origin, int* own_lo, int* own_hi, int cap);
int ptts_conv2d_chain_debug(void* stamp_buf);   /* measurement hook of tools/chain_probe.py: 256 x 32 uint64 phase stamps, NULL = off */
size_t ptts_conv2d_chain_tables_bytes(void);
size_t ptts_conv2d_chain_partials_bytes(int L);
long long ptts_conv2d_chain_map_elems(int B, int T, int F);
int ptts_conv2d_chain_tables(const float* const* w, const float* const* b, void* tables, int L, int cin0, void* stream);
int ptts_conv2d_chain_fwd(const float* x0, long long ldx, const void* tables, void* maps, void* a_last,
                          int B, int T, int F, int L, float alpha, void* stream);
int ptts_conv2d_chain_bwd(const void* d_last, int d_bf16, const float* x0, long long ldx, const void* maps, const void* a_last,
                          const void* tables, float* partials, size_t partials_bytes, int* nblocks_out, int* npart_out,
                          int B, int T, int F, int L, int cin0, float alpha, void* stream);
int ptts_conv2d_chain_bwd_data(const void* d_last, int d_bf16, const void* maps, const void* a_last, const void* tables,
                               void* gmaps, float* g0, int B, int T, int F, int L, float alpha, void* stream);
int ptts_conv2d_chain_second(const float* u0, const void* gmaps, const void* maps, const void* a_last, const void* tables,
                             void* out, int out_bf16, float* partials, size_t partials_bytes, int* nblocks_out, int* npart_out,
                             int B, int T, int F, int L, int cin0, float alpha, void* stream);
int ptts_conv2d_chain_fwd_rows(const float* x0, long long ldx, const void* tables, void* maps, void* a_last,
                               const int* lengths, int B, int T, int F, int L, float alpha, void* stream);
int ptts_conv2d_chain_bwd_rows(const void* d_last, int d_bf16, const float* x0, long long ldx, const void* maps, const void* a_last,
                               const void* tables, float* partials, size_t partials_bytes, int* nblocks_out, int* npart_out,
                               const int* lengths, int B, int T, int F, int L, int cin0, float alpha, void* stream);
int ptts_conv2d_chain_bwd_data_rows(const void* d_last, int d_bf16, const void* maps, const void* a_last, const void* tables,
                                    void* gmaps, float* g0, const int* lengths, int B, int T, int F, int L, float alpha, void* stream);
int ptts_conv2d_chain_second_rows(const float* u0, const void* gmaps, const void* maps, const void* a_last, const void* tables,
                                  void* out, int out_bf16, float* partials, size_t partials_bytes, int* nblocks_out, int* npart_out,
                                  const int* lengths, int B, int T, int F, int L, int cin0, float alpha, void* stream);

/* ---------------------------------------------------------------------------------------
 * fp32 GEMM on the MFMA pipe (v_mfma_f32_32x32x2_f32), with implicit-convolution row
 * addressing for the context Conv1D.  Replaces keras Dense (networktts.py:60; heads at
 * modeltts_common.py:84,95,121; networks_critic.py:96) and kl.Conv1D (networktts.py:117).
 *
 *   C[M,N] (+)= opA(A)[M,K] . opB(B)[K,N] (+ bias[N])
 *
 * A element (m,k):   transA==0:  A[(m / rows_per_seg)*seg_stride + (m % rows_per_seg)*lda + k]
 *                    transA==1:  A[(k / rows_per_seg)*seg_stride + (k % rows_per_seg)*lda + m]
 *   (rows_per_seg = T, seg_stride = (T+KW-1)*Cin, lda = Cin, K = KW*Cin walks a zero-padded
 *    [B, T+KW-1, Cin] frame buffer as the im2col matrix of a 'same' Conv1D without building it;
 *    a plain matrix has rows_per_seg = its row count, seg_stride = 0.)
 * B element (k,n):   transB==0: B[k*ldb + n] ;  transB==1: B[n*ldb + k]
 * The input transform acts on the stored A element; its channel index is the stored column.
 * accumulate != 0 adds to C (beta = 1).
 * out_mask (NULL or laid out like C with ldc): the product is multiplied by (out_mask>0 ? 1 : alpha) before it is
 * stored -- the LeakyReLU mask of a dense layer's backward-data pass, fused into the epilogue.
 * colsum_b (NULL or [N], needs transA==1 and transB==0): receives sum_k B[k,n] -- the bias gradient that goes with a
 * weight-gradient product dW = a^T . dy, taken from the B tiles while they are staged (fp32 atomics across workgroups). */
int ptts_gemm(const float* A, const float* Bm, const float* bias, float* C,
              int M, int N, int K,
              int transA, long long lda, long long rows_per_seg, long long seg_stride,
              int transB, long long ldb, long long ldc,
              int in_mode, const float* in_scale, const float* in_shift, const float* mask_src,
              float alpha, int accumulate, const float* out_mask, float* colsum_b, void* stream);

/* Which kernel family a ptts_gemm call with these arguments launches: the choice ptts_gemm itself makes, as a pure host
 * function (no device, no launch; it reads the deterministic setting and the PTTS_GEMM_* / PTTS_TALL_* switches, as ptts_gemm
 * does).  The scalar arguments are ptts_gemm's; has_bias / has_out_mask / has_colsum_b tell whether that pointer is given;
 * aligned16 is non-zero when A, C, mask_src and out_mask (those that are given) all lie at 16-byte boundaries -- it selects
 * only between the vector and the element-wise form of a thin kernel.  Returns a PTTS_GEMM_PATH_* value, or PTTS_EINVAL for
 * arguments ptts_gemm refuses.  The tests assert the path of every case, so a moved threshold shows as a failure there. */
#define PTTS_GEMM_PATH_GEMV          1   /* thin.hip gemv_rows_kernel<NT, false>: N <= 4, K >= 16, M >= 256, transA = 0   */
#define PTTS_GEMM_PATH_GEMV_VEC      2   /* gemv_rows_kernel<NT, true>: also K % 4 == 0, K <= 256, lda % 4 == 0, aligned  */
#define PTTS_GEMM_PATH_THIN_K        3   /* thin_k_kernel<KT, false>: K <= 4, M N >= 65536, transA = 0                    */
#define PTTS_GEMM_PATH_THIN_K_VEC    4   /* thin_k_kernel<KT, true>: also N % 4 == 0, ldc % 4 == 0, aligned               */
#define PTTS_GEMM_PATH_WCOL_PART     5   /* wcol_part_kernel + wcol_reduce_kernel: transA = 1, N <= 2, K >= 1024          */
#define PTTS_GEMM_PATH_WCOL_PART4    6   /* wcol_part4_kernel + wcol_reduce_kernel: also M % 4 == 0, lda % 4 == 0, aligned */
#define PTTS_GEMM_PATH_WCOL_ATOMIC   7   /* wcol_kernel: the partial rows exceed the stream's buffer (or, not told here: the
                                            buffer cannot be allocated because the stream is being captured)             */
#define PTTS_GEMM_PATH_NSPLIT        8   /* 256 < N <= 512, M >= 2048, K <= 2048, transA = 0: two calls, N = 256 and the rest */
#define PTTS_GEMM_PATH_TALL_MT4      12  /* gemm_tall_kc_kernel<.., MT, 16>, 16 MT rows per workgroup: PTTS_GEMM_PATH_TALL_MT4 + MT - 4 */
#define PTTS_GEMM_PATH_TALL_MT5      13
#define PTTS_GEMM_PATH_TALL_MT6      14
#define PTTS_GEMM_PATH_TALL_MT7      15
#define PTTS_GEMM_PATH_TALL_MT8      16
#define PTTS_GEMM_PATH_DMA           20  /* gemm_dma_kernel, one workgroup per 128 x 128 tile (edge tiles: the register-staged body) */
#define PTTS_GEMM_PATH_DMA_STREAMK   21  /* gemm_dma_kernel, stream-K: equal (tile, k-step) ranges, fp32 atomics           */
#define PTTS_GEMM_PATH_TILE          22  /* gemm_f32_mfma_kernel (register-staged), one workgroup per tile                 */
#define PTTS_GEMM_PATH_TILE_STREAMK  23  /* gemm_f32_mfma_kernel, stream-K                                                 */
int ptts_gemm_path(int M, int N, int K, int transA, long long lda, long long rows_per_seg, long long seg_stride,
                   int transB, long long ldb, long long ldc, int in_mode, int accumulate,
                   int has_bias, int has_out_mask, int has_colsum_b, int aligned16);

/* Weight gradients of several layers in ONE launch: for every product  C[M,N] += T(A)[K,M]^T . B[K,N]  and, when
 * colsum_b is given,  colsum_b[N] += sum_k B[k,:]  (the bias gradient).  A is the layer input as stored ([K rows][lda]),
 * B the incoming gradient; T is the same fused transform as in ptts_gemm (in_mode on the stored A element, channel =
 * stored column).  Every C / colsum_b is ACCUMULATED into with fp32 atomics (zero it beforehand for a plain product):
 * the caller's gradient buffers, as keras accumulates the gradients of the layers of one K.gradients call.  One
 * workgroup grid walks the (product, tile, k-step) space, so a 256x256x25600 product no longer pays its own launch,
 * zero-fill and 128-way split. */
typedef struct ptts_wgrad_desc {
    const float* A; const float* B; float* C; float* colsum_b;
    const float* in_scale; const float* in_shift; const float* mask_src;
    int M, N, K;
    long long lda, ldb, ldc;
    int in_mode; float alpha;
} ptts_wgrad_desc;
int ptts_gemm_wgrad_grouped(const ptts_wgrad_desc* descs, int n, void* stream);

/* The Dense products with M >> N (reference networktts.py:59-63 pFC -> kl.Dense, networks_critic.py:86-93, the LSTM input
 * projections of networktts.py:85-96, and TF's MatMul gradients) as fp32 products on the bf16 matrix cores by the three-way
 * operand split of split.hip ("bf16x6": six bf16 MFMA products, fp32 accumulation; dense.hip).  The weight operand B[K][N] is
 * split once per update into fragment-ordered planes (ptts_split3_dense_weight; transposed = 1 reads w as [N][K], which
 * makes dX = dY.W^T read W as it lies); ptts_dense_bf16x6 then has the contract of ptts_gemm with transA = 0:
 * C[M,N] (+)= T(A).B (+ bias), C *= (out_mask > 0 ? 1 : alpha), T = in_mode (PTTS_IN_*) with in_scale/in_shift [K] or
 * mask_src laid out like A.  N, K, lda, ldc multiples of 4, operands 16-byte aligned (ptts_dense_bf16x6_supported). */
size_t ptts_dense_planes_bytes(int N, int K);
int ptts_split3_dense_weight(const float* w, long long ldw, int K, int N, int transposed, void* planes, void* stream);
/* The same for n weights in ONE launch: after an optimiser update every Dense kernel of a network needs its planes again (forward and
 * transposed), 18 launches of 4 us per critic step otherwise. */
typedef struct ptts_dense_split_desc {
    const float* w; void* planes;
    long long ldw;
    int K, N, transposed, reserved;
} ptts_dense_split_desc;
int ptts_split3_dense_weight_grouped(const ptts_dense_split_desc* descs, int n, void* stream);
/* Planes of windows of frame sequences x [B][T][C] (the segments of the overlap-save form of the frequency-domain Conv1D): matrix
 * z = b*NS + s = the P rows x[b][row_off + s*S + k][:], k < P; rows outside [0, T) and k >= kvalid are zero (never read). */
int ptts_split3_frame_windows(const float* x, int B, int T, int C, int NS, int S, int row_off, int P, int kvalid,
                              void* planes, long long stride_planes_bytes, void* stream);
/* n weights of ONE shape at regular strides: w + i*stride_w (floats) -> planes + i*stride_planes_bytes. */
int ptts_split3_dense_weight_strided(const float* w, long long stride_w, void* planes, long long stride_planes_bytes, int n,
                                     long long ldw, int K, int N, int transposed, void* stream);
int ptts_dense_bf16x6_supported(int M, int N, int K, long long lda, long long ldc);
/* One weight-gradient product of ptts_gemm_wgrad_grouped (TF's MatMul gradient w.r.t. the kernel of a kl.Dense / LSTM
 * projection, plus the bias gradient) as a bf16x6 split product, in two stages without atomics between workgroups:
 * ptts_dense_wgrad_bf16x6_partials writes every workgroup's partial tile of dW[Kin,N] = T(A)[M,Kin]^T . dY[M,N] (and of the
 * column sums of dY) as a row of `workspace` (both operands split on their way into the LDS and read transposed);
 * ptts_dense_wgrad_reduce_grouped sums the rows of up to 16 products per launch in a fixed order and ADDS them into the
 * caller's gradient buffers (one fp32 atomic per element: products of one backward pass may share a buffer).
 * ptts_dense_wgrad_bf16x6 runs both stages for one product. */
typedef struct ptts_dense_wgrad_reduce_desc {
    const float* partials;                   /* the workspace of ptts_dense_wgrad_bf16x6_partials */
    int split, Kin, N;                       /* *split_out of that call; the product's dims */
    long long ldc;
    float* C; float* colsum_b;               /* C[Kin][ldc] += dW ; colsum_b[N] += column sums of dY (or NULL) */
} ptts_dense_wgrad_reduce_desc;
int ptts_dense_wgrad_bf16x6_supported(int Kin, int N, int M, long long lda, long long ldb);
size_t ptts_dense_wgrad_workspace_bytes(int Kin, int N, int M);
int ptts_dense_wgrad_bf16x6_partials(const float* A, const float* dY, const float* mask_src, const float* in_scale,
                                     const float* in_shift, void* workspace, size_t workspace_bytes, int* split_out,
                                     int Kin, int N, int M, long long lda, long long ldb, int in_mode, float alpha,
                                     void* stream);
int ptts_dense_wgrad_reduce_grouped(const ptts_dense_wgrad_reduce_desc* descs, int n, void* stream);
int ptts_dense_wgrad_bf16x6(const float* A, const float* dY, const float* mask_src, const float* in_scale,
                            const float* in_shift, float* C, float* colsum_b, void* workspace, size_t workspace_bytes,
                            int Kin, int N, int M, long long lda, long long ldb, long long ldc, int in_mode, float alpha,
                            void* stream);
int ptts_dense_bf16x6(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                      long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                      const float* mask_src, float alpha, int accumulate, const float* out_mask, void* stream);
/* ... + res[m % res_rows][n] (row stride ldr floats) added in the store, res_rows <= M <= 8 res_rows: the product of a concatenation part
 * shared by k stacked evaluations (the critic's context branch, networks_critic.py:78-86, computed once at B rows) joins each of the k
 * row blocks without an add pass.  res == C with res_rows >= M is ptts_dense_bf16x6's accumulate. */
int ptts_dense_bf16x6_res(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                          long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                          const float* mask_src, float alpha, const float* res, int res_rows, long long ldr,
                          const float* out_mask, void* stream);
/* The product of a kl.Dense that feeds a kl.BatchNormalization (pFC, networktts.py:59-63) also leaves, per row tile, the column sums and
 * the column sums of squares of what it stores: stats[*nrows_out][2 N] doubles, finished by ptts_bn_finalize_partials -- TF's batch
 * moments are a pass of their own over the activation.  capacity_rows >= ptts_dense_bf16x6_stats_rows(M, N); N % 4 == 0. */
int ptts_dense_bf16x6_stats_rows(int M, int N);
int ptts_dense_bf16x6_stats(const float* A, const void* planes, const float* bias, float* C, int M, int N, int K,
                            long long lda, long long ldc, int in_mode, const float* in_scale, const float* in_shift,
                            float alpha, double* stats, int capacity_rows, int* nrows_out, void* stream);
/* Backward-data product of a kl.Dense whose input was the kl.BatchNormalization + kl.LeakyReLU of pFC (networktts.py:59-63), i.e.
 * lrelu(scale z + shift):  C = dz = (A . B) lrelu'(scale z + shift) scale  with A = dy [M, K], B = W^T (planes of the transposed kernel,
 * [K, N]), z [M, N]; and per row tile the column sums of (A . B) lrelu'(.) z and of (A . B) lrelu'(.) -- the gradients of scale and
 * shift -- as stats[*nrows_out][2 N] doubles, which ptts_partial_rows_sum adds.  What TF runs as MatMul + LeakyReluGrad + the reductions of
 * FusedBatchNormGrad's first stage; replaces ptts_dense_bf16x6 + ptts_affine_act_bwd (a pass over da and z). */
int ptts_dense_bf16x6_bwd_affine(const float* A, const void* planes, float* C, int M, int N, int K, long long lda, long long ldc,
                                 const float* z, const float* scale, const float* shift, float alpha,
                                 double* stats, int capacity_rows, int* nrows_out, void* stream);
/* out[j] = sum_r partials[r][j] (doubles), rows added in index order. */
int ptts_partial_rows_sum(const double* partials, int nrows, int ncols, double* out, void* stream);
/* Frequency-domain context Conv1D, helper: Ap [NB][2][B][2*Kh] floats with [Xr | .] in part 0 and [Xi | .] in part 1 (columns < Cin)
 * -> columns Kh .. Kh+Cin-1 get -Xi (part 0) and Xr (part 1): the rows [Xr | -Xi], [Xi | Xr] of the real form of a complex product. */
int ptts_dft_mirror(float* Ap, int NB, int B, int Cin, int Kh, void* stream);

/* Frequency-domain context Conv1D, the kernel's side: planes (ptts_dense_bf16x6_batched layout, ptts_dense_planes_bytes(N, 2*Kh) per
 * frequency) of [Wr_f ; Wi_f] [2*Kh][N], W^_f = sum_k w[k] tw[(f,.)][k], for f < NB, from w [KW][Cin][N] (KW in 3, 5, 7, 9, 11, 21) and
 * the twiddle rows tw [2*NB][KW] (row 2f: cos, row 2f+1: -sin of 2 pi f (pl - k) / P).  Once per weight update. */
int ptts_conv1d_freq_kernel_planes(const float* w, const float* tw, void* planes, int NB, int KW, int Cin, int N, int Kh, void* stream);

/* dst[z][c][r] = src[z][r][c], nb matrices of rows x cols floats. */
int ptts_transpose_batched(const float* src, float* dst, int nb, int rows, int cols, void* stream);
/* Frequency-domain context Conv1D, weight gradient, last step: dW[k][c][n] = out2[k][n*2Kh + c] + out2[KW+k][n*2Kh + Kh + c], out2
 * [2*KW][N*2*Kh] = the product of the inverse twiddles with the per-frequency correlations (TF's Conv1D kernel backprop). */
int ptts_conv1d_freq_wgrad_combine(const float* out2, float* dW, int KW, int Cin, int N, int Kh, void* stream);

/* ... or both steps in one pass over the correlations Gt [NB][N][2*Kh] (KW in 3, 5, 7, 9, 11, 21; t2 [NB][NBp], NBp >= 2*KW: row f =
 * the KW cosine then the KW sine coefficients of frequency f): dW[k][c][n] = sum_f t2[f][k] Gt[f][n][c] + t2[f][KW+k] Gt[f][n][Kh+c]; the frequencies are shared out over four groups of workgroups
 * whose partial sums (workspace) are added in a fixed order: no atomics. */
size_t ptts_conv1d_freq_wgrad_inverse_workspace_bytes(int KW, int Cin, int N);
int ptts_conv1d_freq_wgrad_inverse(const float* Gt, const float* t2, float* dW, void* workspace, size_t workspace_bytes,
                                   int NB, int NBp, int KW, int Cin, int N, int Kh, void* stream);

/* nbatch products of one shape in one launch: C_z[M,N] = A_z[M,K] . B_z (+ bias), A_z = A + z*strideA and C_z = C + z*strideC (floats;
 * strideA = 0 shares the left operand), B_z = the planes at planes + z*stride_planes_bytes (ptts_split3_dense_weight[_grouped] layout).
 * planes_count 3 = fp32 arithmetic (six bf16 products), 1 = one bf16 product.  The building block of the frequency-domain context
 * Conv1D (kl.Conv1D of networktts.py:116-120 as DFT -> per-frequency products -> inverse DFT).
 *
 * The fp32-rows form of the right operand: planes_count = 3 | PTTS_PLANES_ROWS or 1 | PTTS_PLANES_ROWS.  `planes` is then a HOST pointer
 * to one ptts_dense_rows_desc, read during the call, and stride_planes_bytes is ignored: the kernel reads B_z [K][N] as fp32 where it
 * lies and splits it in front of each k-step's matrix instructions, so a right operand that is used once needs no split pass.
 *   windows == 0: row k of member z is B + z*strideB + k*ldb.
 *   windows == 1: z = b*NS + s (nbatch = nB*NS) is the window of ptts_split3_frame_windows: row k = row row_off + s*S + k of
 *                 utterance b of B [nB][T][ldb]; rows outside [0, T) are zero.
 *   Rows k >= kvalid (kvalid <= K) are zero in both forms.  A row that counts as zero is never read.
 *   mirror_cols = Kh > 0 (a multiple of 4, N <= Kh, Kh + N <= ldc, M even): the lane that stores C_z[m][n] also stores C_z[m ^ 1][Kh + n],
 *                 the value itself for even m and the negated value for odd m -- what ptts_dft_mirror writes, bit for bit.
 * The results are those of the planes form on the planes of the same rows, bit for bit.  The form exists on the resident-left kernel
 * only: where ptts_dense_batched_resident_eligible says 0 or the switch is off the call returns PTTS_EINVAL and launches nothing.  The
 * source may span at most 2^30 floats (offsets are 32-bit byte offsets). */
#define PTTS_PLANES_ROWS 0x100
typedef struct ptts_dense_rows_desc {
    const float* B;
    long long strideB, ldb;
    int windows, nB, T, NS, S, row_off;
    int kvalid, mirror_cols;
} ptts_dense_rows_desc;
int ptts_dense_bf16x6_batched(const float* A, long long strideA, const void* planes, long long stride_planes_bytes,
                              const float* bias, float* C, long long strideC, int nbatch, int M, int N, int K,
                              long long lda, long long ldc, int planes_count, void* stream);
/* The resident-left form of ptts_dense_bf16x6_batched: members that share a left operand (strideA == 0) of M <= 128 rows and K <= 128
 * columns run on a kernel that splits A once per workgroup into the LDS and lets its waves walk (member, 32-column slice) work items,
 * with no barrier after the prologue; the results are those of the general kernel bit for bit.  On by default; the environment variable
 * PTTS_DENSE_BATCHED_RESIDENT=0 (read once) or ptts_set_dense_batched_resident(0) sends every batched product to the general kernel.
 * ptts_set_dense_batched_resident returns the previous setting; ptts_dense_batched_resident_eligible returns 1 when a call of that
 * shape takes the resident-left kernel while the switch is on, 0 otherwise, and launches nothing; ptts_dense_batched_resident_enabled
 * returns the switch. */
int ptts_set_dense_batched_resident(int on);
int ptts_dense_batched_resident_enabled(void);
int ptts_dense_batched_resident_eligible(long long strideA, int M, int N, int K, int planes_count);
/* nbatch transposed-reduction products of one shape in one launch: C_z[k][n] = sum_{m<M} A_z[m][k] B_z[m][n], k < Kin, n < N.  Both
 * operands are fp32, row-major (lda, ldb) and are split inside the kernel, so a right operand that is used once needs no planes; A_z =
 * A + z*strideA (0 shares it), B_z = B + z*strideB, C_z = C + z*strideC (floats), C row-major with ldc.  Only cells k < Kin, n < N of C
 * are written.  The operands are read in quads: lda >= Kin and ldb >= N rounded up to 4.  Pointers, leading dimensions and strides keep
 * 16-byte alignment.  planes_count as above.  The per-frequency correlations of the frequency-domain context Conv1D's weight
 * gradient are one of these. */
int ptts_dense_tn_bf16x6_batched(const float* A, long long strideA, const float* B, long long strideB, float* C, long long strideC,
                                 int nbatch, int M, int Kin, int N, long long lda, long long ldb, long long ldc, int planes_count,
                                 void* stream);

/* The context Conv1D forward (reference networktts.py:116-120: kl.Conv1D(width, winlen, padding='same')) as an fp32
 * product on the bf16 matrix cores by a three-way operand split ("bf16x6"; split.hip): x = x1 + x2 + x3 in bf16 (round
 * to nearest), six bf16 products per operand pair, fp32 accumulation -- fp32-level accuracy at 2.7x less matrix-pipe time.
 *   ptts_split3_frames   x [B][T][C] fp32 -> three bf16 planes [Cp/32][B*(pad_left+T+pad_right)][32]: 32-channel blocks
 *                        of the time-padded frames, zero padded in time and in the channels C..Cp-1 (Cp % 32 == 0);
 *   ptts_split3_weight_t w [KW][C][N] fp32 -> three bf16 planes [Cp/32][N][KW][32] (transposed, zero channels C..Cp-1);
 *   ptts_conv1d_bf16x6   y[b][t][n] = bias[n] + sum_{j,c} x[b][t + j - pad_left][c] w[j][c][n] from those planes, with
 *                        pad_left + pad_right = KW - 1.  N % 128 == 0, Cp % 32 == 0, T >= 128 (or B == 1), KW <= 24. */
int ptts_split3_frames(const float* x, void* p1, void* p2, void* p3, int B, int T, int C, int pad_left, int pad_right,
                       int Cp, void* stream);
int ptts_split3_weight_t(const float* w, void* p1, void* p2, void* p3, int KW, int C, int N, int Cp, void* stream);
int ptts_conv1d_bf16x6(const void* a1, const void* a2, const void* a3, const void* bt1, const void* bt2, const void* bt3,
                       const float* bias, float* y, int B, int T, int KW, int Cp, int N, void* stream);

/* The context Conv1D weight gradient (TF's Conv1D kernel backprop of networktts.py:116-120) as a bf16x6 split product:
 *   dw[j][c][n] = sum_{b,t} xp[b][t + j][c] dy[b][t][n]   (xp: the frames zero-padded in time to T + KW - 1).
 *   ptts_split3_frames_t  x [B][T][C] fp32 -> three FRAME-MAJOR bf16 planes [Crows][Pp], element (c, b Tp + pad_left + t),
 *                         zero elsewhere (Crows % 32 == 0, >= C; Pp % 64 == 0, >= B Tp).  Used for the padded frames
 *                         (B, T + KW - 1, pad_left 0, Tp = T + KW - 1) and for dy (B, T, pad_left 0, Tp = T + KW - 1);
 *   ptts_conv1d_wgrad_bf16x6  dw (overwritten) from those planes; KW in {3, 5, 21}, N % 32 == 0, Crows % 64 == 0,
 *                         Pp >= 32 ceil(B (T + KW - 1) / 32) + 64. */
int ptts_split3_frames_t(const float* x, void* p1, void* p2, void* p3, int B, int T, int C, int pad_left, int Tp, int Crows,
                         long long Pp, void* stream);
int ptts_conv1d_wgrad_bf16x6(const void* xt1, const void* xt2, const void* xt3, const void* yt1, const void* yt2,
                             const void* yt3, float* dw, int B, int T, int KW, int C, int N, int Crows, long long Pp,
                             void* stream);

/* The same weight gradient in exact fp32 (v_mfma_f32_16x16x4_f32) over frame-major fp32 operands (conv1d_wgrad.hip):
 *   ptts_transpose_frames  x [B][T][C] -> out [Crows][Pp], element (c, b Tp + pad_left + t), zero elsewhere;
 *   ptts_conv1d_wgrad_t    dw (overwritten; and db[n] = sum_{b,t} dy[b][t][n] when db != NULL) from xt = the transposed
 *                          padded frames and yt = the transposed gradient (Tp = T + KW - 1 for both).  KW in {3, 5, 21},
 *                          N % 32 == 0, Crows % 64 == 0, Pp % 64 == 0, Pp >= 32 ceil(B (T + KW - 1) / 32) + 64. */
int ptts_transpose_frames(const float* x, float* out, int B, int T, int C, int pad_left, int Tp, int Crows, long long Pp,
                          void* stream);
int ptts_conv1d_wgrad_t(const float* xt, const float* yt, float* dw, float* db, int B, int T, int KW, int C, int N, int Crows,
                        long long Pp, void* stream);

/* ---------------------------------------------------------------------------------------
 * channel-last reductions and elementwise passes
 * ------------------------------------------------------------------------------------- */
/* sums[0:C] = sum_r a[r,c], sums[C:2C] = sum_r a[r,c]^2 in fp64, a = transform(x); deterministic two-stage. */
size_t ptts_colstats_workspace_bytes(long long rows, int C);
int ptts_colstats(const float* x, long long rows, int C,
                  int in_mode, const float* in_scale, const float* in_shift, const float* mask_src, float alpha,
                  double* sums /*[2C]*/, void* workspace, size_t workspace_bytes, void* stream);

/* Keras BatchNormalization (axis=-1, eps, momentum) statistics -> per-channel affine.
 * Replaces kl.BatchNormalization at networktts.py:61,118,124,132.
 *   training: mean,var from sums (biased var); scale = gamma*rsqrt(var+eps); shift = beta-mean*scale;
 *             moving stats updated in place with `momentum` (moving_var uses var*count/(count-1) when unbiased_moving!=0)
 *             when update_moving != 0.   inference: same from moving stats. */
int ptts_bn_finalize(const double* sums, long long count, const float* gamma, const float* beta,
                     float* moving_mean, float* moving_var, float eps, float momentum,
                     int training, int update_moving, int unbiased_moving, int C,
                     float* scale, float* shift, float* mean /*[C] out*/, float* rstd /*[C] out*/, void* stream);

/* Training-mode statistics AND the affine of a few-channel map (C = 4, 8, 16: the conv stacks' BatchNormalization, networktts.py:124)
 * in one launch: ptts_colstats + ptts_bn_finalize(training = 1) fused (the workgroup that finishes last adds the partial rows in a
 * fixed order: bit-reproducible).  workspace: ptts_colstats_workspace_bytes(rows, C); counter: one int, zero before the first call,
 * left zero by every call, not shared between streams. */
int ptts_bn_batch_stats_supported(long long rows, int C);
int ptts_bn_batch_stats(const float* x, long long rows, int C, const float* gamma, const float* beta,
                        float* moving_mean, float* moving_var, float eps, float momentum, int update_moving, int unbiased_moving,
                        float* scale, float* shift, float* mean /*[C] out*/, float* rstd /*[C] out*/,
                        void* workspace, size_t workspace_bytes, int* counter, void* stream);

/* ptts_bn_finalize(training = 1) for sums that lie as nrows partial rows [2 C] doubles (C sums, C sums of squares), added in
 * index order: the finish of ptts_conv2d_mfma_fwd_stats and of ptts_dense_bf16x6_stats.  rows = the number of values per channel the sums cover. */
int ptts_bn_finalize_partials(const double* partials, int nrows, long long rows, int C, const float* gamma, const float* beta,
                              float* moving_mean, float* moving_var, float eps, float momentum, int update_moving, int unbiased_moving,
                              float* scale, float* shift, float* mean /*[C] out*/, float* rstd /*[C] out*/, void* stream);

/* BatchNorm backward through the batch statistics.  Given dscale/dshift (gradients w.r.t. the affine that
 * ptts_bn_finalize produced in training mode):  dgamma = (dscale - dshift*mean)*rstd ;  dbeta = dshift ;
 *   dmean = -dshift*gamma*rstd ;  dvar = -0.5*(dscale - dshift*mean)*gamma*rstd^3 ;
 *   c2 = 2*dvar/count ;  c0 = dmean/count - c2*mean      so that   dz[r,c] += c0[c] + c2[c]*z[r,c]. */
int ptts_bn_bwd_coefs(const float* dscale, const float* dshift, const float* mean, const float* rstd,
                      const float* gamma /*NULL = 1*/, long long count, int C,
                      float* dgamma, float* dbeta, float* c0, float* c2, void* stream);
/* ... with dgamma / dbeta ADDED into the buffers given (the parameters' gradient buffers: no separate accumulation launch per parameter) */
int ptts_bn_bwd_coefs_acc(const float* dscale, const float* dshift, const float* mean, const float* rstd,
                      const float* gamma /*NULL = 1*/, long long count, int C,
                      float* dgamma, float* dbeta, float* c0, float* c2, void* stream);

/* y = act(x*scale[c]+shift[c]) materialised (used where no consumer can fuse it: LSTM input, final outputs). */
int ptts_affine_act(const float* x, const float* scale, const float* shift, float* y,
                    long long rows, int C, int act, float alpha, void* stream);
/* The same over a zero-padded batch x [B,T,inner] with a length per row (ragged inference): frames t >= lens[b] give 0.
 * y[b,t,i] = t < lens[b] ? act(x*scale[c]+shift[c]) : 0, c = i % C; inner = elements per frame, a multiple of C (C for
 * [B,T,C], F*C for a Conv2D map).  lens: device int [B].  scale/shift NULL together = identity.  y == x is allowed. */
int ptts_affine_act_rows(const float* x, const float* scale, const float* shift, float* y, const int* lens,
                         int B, int T, int inner, int C, int act, float alpha, void* stream);
/* Its backward with respect to x (evaluation with an input gradient: no parameter gradients):
 * dx[b,t,i] = t < lens[b] ? dy * act'(x*scale[c]+shift[c]) * scale[c] : +0.  act: PTTS_ACT_NONE or PTTS_ACT_LRELU (x may be
 * NULL for NONE).  The same indexing; a float4 path where C % 4 == 0 and the pointers are 16-byte aligned.  dx == dy is allowed. */
int ptts_affine_act_rows_bwd(const float* dy, const float* x, const float* scale, const float* shift, float* dx,
                             const int* lens, int B, int T, int inner, int C, int act, float alpha, void* stream);
/* Masked training: BatchNormalization over a zero-padded batch [B,T,inner] with a length per row (lens: device int [B],
 * 1 <= lens[b] <= T; c = i % C, inner a multiple of C).  Pad frames are never read; all sums are fp64, two-stage, in a fixed
 * order (bit-reproducible), with the float4 path of their dense siblings where C % 4 == 0 and the pointers are 16-byte aligned.
 * workspace for the two reductions: ptts_colstats_rows_workspace_bytes (0 for dimensions the calls refuse).
 *   ptts_colstats_rows: sums[0:C] = sum x, sums[C:2C] = sum x^2 over the real frames (ptts_colstats in identity input mode,
 *     masked); finished by ptts_bn_finalize with count = N * inner / C, N = sum_b lens[b], which the host knows.
 *   ptts_affine_act_rows_bwd_params: dx as ptts_affine_act_rows_bwd, and dsums [2C] = (dscale, dshift) over the real frames in
 *     the same pass (ptts_affine_act_bwd, masked); act PTTS_ACT_NONE or PTTS_ACT_LRELU; dx == dy is allowed.
 *   ptts_axpby_cols_rows: out[b,t,i] = t < lens[b] ? a + x*c2[c] + c0[c] : +0, the statistics' share of the BatchNorm
 *     backward (c0, c2 of ptts_bn_bwd_coefs with the masked count); out == a is allowed. */
size_t ptts_colstats_rows_workspace_bytes(int B, int T, int inner, int C);
int ptts_colstats_rows(const float* x, const int* lens, int B, int T, int inner, int C, double* sums /*[2C]*/,
                       void* workspace, size_t workspace_bytes, void* stream);
int ptts_affine_act_rows_bwd_params(const float* dy, const float* x, const float* scale, const float* shift, float* dx,
                                    double* dsums /*[2C]: dscale, dshift*/, const int* lens, void* workspace,
                                    size_t workspace_bytes, int B, int T, int inner, int C, int act, float alpha, void* stream);
int ptts_axpby_cols_rows(const float* a, const float* x, const float* c2, const float* c0, float* out, const int* lens,
                         int B, int T, int inner, int C, void* stream);
/* dx = dy * act'(.) * scale ; dscale/dshift reductions (NULL to skip).  `y` is the forward output (sigmoid/tanh use it). */
int ptts_affine_act_bwd(const float* dy, const float* x, const float* y, const float* scale, const float* shift,
                        float* dx, double* dsums /*[2C]: dscale, dshift; or NULL*/,
                        void* workspace, size_t workspace_bytes,
                        long long rows, int C, int act, float alpha, void* stream);
/* The gated product of a gated convolution (networktts.py:128-134, pGCNN2D): y = a * sigmoid(b) over the two Conv2D
 * pre-activations, and its backward da = dy*s, db = dy*a*s*(1-s), s = sigmoid(b).  One pass each; n = element count. */
int ptts_gated_mul_fwd(const float* a, const float* b, float* y, long long n, void* stream);
int ptts_gated_mul_bwd(const float* dy, const float* a, const float* b, float* da, float* db, long long n, void* stream);

/* out[r,c] = (acc? out : 0) + a[r,c]*c1[c] + x[r,c]*c2[c] + c0[c]   (BatchNorm backward fix-up: dz += dmean/N + dvar*2(z-mean)/N) */
int ptts_axpby_cols(const float* a, const float* c1, const float* x, const float* c2, const float* c0,
                    float* out, long long rows, int C, void* stream);

/* ---------------------------------------------------------------------------------------
 * WGAN-GP pieces (optimizertts_wgan.py:44-79)
 * ------------------------------------------------------------------------------------- */
/* RandomWeightedAverage (:44-51): out = alpha_b*real + (1-alpha_b)*fake, alpha per sample */
int ptts_gp_interpolate(const float* real, const float* fake, const float* alpha_b /*[B]*/, float* out,
                        int B, long long TD, void* stream);
/* per-sample squared L2 norm over (T, D) (:58-62), wavefront-reduced; out[B] */
int ptts_gp_sqnorm(const float* g, float* out, int B, long long TD, void* stream);
/* penalty = mean_b (1 - sqrt(sq_b))^2 (:64-68);  coef[b] = dPenalty/dg scale = 2*(n_b-1)/(n_b*B)  (inf/nan at n_b=0 as in the reference) */
int ptts_gp_penalty(const float* sq /*[B]*/, float* penalty /*[1]*/, float* coef /*[B]*/, int B, void* stream);
/* dg = upstream[0] * coef[b] * g */
int ptts_gp_scale_rows(const float* g, const float* coef, const float* upstream /*[1] or NULL(=1)*/, float* dg,
                       int B, long long TD, void* stream);

/* Per-row costs of a ragged batch [B,T,...] with a length per row (lens: device int [B], 1 <= lens[b] <= T): one workgroup per
 * row, fp64 partials summed in a fixed order, no atomics -- a row's result depends on nothing but that row. */
/* out[b] = sign * mean over t < lens[b] and all `inner` elements of v [B,T,inner] */
int ptts_rows_mean(const float* v, const int* lens, int B, int T, int inner, float sign, float* out /*[B]*/, void* stream);
/* out_ls[b] = mean_{t<lens[b],d} (y-yhat)^2 * w[d] (specweighted_lse_loss of that row alone; w NULL = 1) and the unweighted
 * out_sq[b] = sum_{t<lens[b],d} (y-yhat)^2 in one pass; either output may be NULL */
int ptts_wlse_rows(const float* y, const float* yhat, const float* w /*[D] or NULL*/, const int* lens, int B, int T, int D,
                   float* out_ls /*[B] or NULL*/, double* out_sq /*[B] or NULL*/, void* stream);
/* Masked training: the costs of the whole batch, means over its N = sum_b lens[b] real frames (N from the host, which made
 * the lengths: 1 <= N <= B*T), and their backward.  Pad frames of the gradients are +0.
 *   ptts_rows_combine:  out[0] = sum_b rows[b] * lens[b] / N in fp64, in index order: the batch mean out of the per-row means
 *                       of ptts_rows_mean / ptts_wlse_rows (lengths read as those kernels read them, clamped to [0, T]).
 *   ptts_rows_mean_bwd: dv[b,t,:] = t < lens[b] ? upstream * sign / (N * inner) : 0   (sign / N for a critic's [B,T,1])
 *   ptts_wlse_rows_bwd: dyhat[b,t,d] = t < lens[b] ? upstream * 2 (yhat - y) w[d] / (N * D) : 0
 * upstream: device float [1], or NULL for 1. */
int ptts_rows_combine(const float* rows /*[B]*/, const int* lens, int B, int T, long long N, float* out /*[1]*/, void* stream);
int ptts_rows_mean_bwd(const float* upstream, const int* lens, int B, int T, int inner, float sign, long long N,
                       float* dv, void* stream);
int ptts_wlse_rows_bwd(const float* y, const float* yhat, const float* w /*[D] or NULL*/, const float* upstream,
                       const int* lens, int B, int T, int D, long long N, float* dyhat, void* stream);
/* out[b] = (1 - sqrt(sq[b]))^2: the gradient penalty per sample, from ptts_gp_sqnorm's sq */
int ptts_gp_penalty_rows(const float* sq /*[B]*/, float* out /*[B]*/, int B, void* stream);

/* One batch cut out of a corpus resident on the device (data.DeviceCorpus, csrc/batchgather.hip).  Up to three streams
 * (nstreams = 1..3: inputs, outputs, time weights; the unused ones NULL / 0) are packed row-wise, src_k [N_total][D_k] fp32,
 * and share row_off [U+1] (device long long, in rows): utterance u is rows row_off[u] .. row_off[u+1]-1.  Row b of the batch is
 * described by the device int arrays utt, shift, n [B]:
 *   dst_k[b][t][:] = src_k[row_off[utt[b]] + shift[b] + t][:]  for t < n[b],   exactly 0 for n[b] <= t < T.
 * Every element of every dst_k [B][T][D_k] is written once (no memset needed), all streams in ONE launch.  Source indices are
 * 64-bit, so N_total * D_k is not limited; T * D_k has to fit an int and B <= 65535.  The caller guarantees 0 <= utt[b] < U,
 * 0 <= shift[b], 0 <= n[b] <= T and shift[b] + n[b] <= the utterance's length (ops.batch_windows checks them on the host); a
 * row that breaks this is not read at all and comes out as zeros.  Pointers need 4-byte alignment only: the destination is
 * written in 16-byte aligned float4 groups with a scalar head and tail per batch row, the source read at 4-byte boundaries. */
int ptts_batch_windows(const float* src0, const float* src1, const float* src2, float* dst0, float* dst1, float* dst2,
                       int D0, int D1, int D2, int nstreams, const long long* row_off /*[U+1]*/, int U, const int* utt /*[B]*/,
                       const int* shift /*[B]*/, const int* n /*[B]*/, int B, int T, void* stream);

/* wasserstein_loss (:70-71): out[0] = sign * mean(v) ; specweighted_lse_loss (:73-79): out[0] = mean((y-yhat)^2 * w[d]) */
int ptts_mean_scaled(const float* v, long long n, float sign, float* out, void* stream);
int ptts_wlse_fwd(const float* y, const float* yhat, const float* w /*[D] or NULL*/, float* out,
                  long long rows, int D, void* stream);
/* dyhat = upstream[0] * 2*(yhat-y)*w[d]/(rows*D) */
int ptts_wlse_bwd(const float* y, const float* yhat, const float* w, const float* upstream, float* dyhat,
                  long long rows, int D, void* stream);

/* weight clipping (north_star extra; the reference has no counterpart): p = clamp(p, lo, hi) */
int ptts_weight_clip(float* p, long long n, float lo, float hi, void* stream);

/* Keras-2.2 Adam (keras.optimizers.Adam, optimizertts_wgan.py:145,172):
 *   t = ++(*step);  lr_t = lr*sqrt(1-b2^t)/(1-b1^t);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2;
 *   p -= lr_t * m / (sqrt(v) + eps).   `step` lives on the device so the launch is graph-replayable;
 *   gscale multiplies g first (1/world_size after an all-reduce(sum)). */
int ptts_adam_keras_step(float* p, const float* g, float* m, float* v, long long n,
                         float lr, float b1, float b2, float eps, float gscale,
                         int* step /*device int, incremented by the kernel*/, void* stream);

/* ---------------------------------------------------------------------------------------
 * Keras LSTM (gates i,f,c,o; activation tanh, recurrent_activation sigmoid; networktts.py:72-96).
 * ndir = 1: one direction (reverse != 0 walks time backwards); ndir = 2: kl.Bidirectional(concat),
 * direction 0 forwards and direction 1 backwards in the SAME launches (networktts.py:85-96).
 *   xproj [B,T,ndir*4H] = x.[W_d0 | W_d1] + b (one ptts_gemm);  U [ndir,H,4H]
 *   h_out [B,T,ndir*H] (the Bidirectional concat layout), gates (post-nonlinearity) [B,T,ndir*4H]
 *   and cell states c_out [B,T,ndir*H] are kept for the backward.
 * ------------------------------------------------------------------------------------- */
size_t ptts_lstm_fwd_workspace_bytes(int B, int T, int H, int ndir);   /* packed recurrent kernel */
int ptts_lstm_fwd(const float* xproj, const float* U, float* h_out, float* gates, float* c_out,
                  void* workspace, size_t workspace_bytes,
                  int B, int T, int H, int ndir, int reverse, void* stream);
/* Forward for inference over a zero-padded batch with a length per row: lens is a device int [B], 1 <= lens[b] <= T.
 * Row b is active for its first lens[b] steps; a backward direction (direction 1, or reverse) starts at the row's own
 * last frame t = lens[b]-1 with zero state.  On t < lens[b] h_out holds what ptts_lstm_fwd gives for that row alone
 * (B = 1, T = lens[b]), bit for bit; on t >= lens[b] it is 0.0f.  gates and c_out may be NULL (they are stored on real
 * frames where given).  workspace: the cell-state carry, ndir*B*H floats rounded up to 256 bytes, followed by
 * ptts_lstm_fwd_workspace_bytes for the packed recurrent kernel (without the latter, as ptts_lstm_fwd without one). */
int ptts_lstm_fwd_ragged(const float* xproj, const float* U, float* h_out, float* gates /*or NULL*/,
                         float* c_out /*or NULL*/, const int* lens, void* workspace, size_t workspace_bytes,
                         int B, int T, int H, int ndir, int reverse, void* stream);
/* dgates [B,T,ndir*4H] out: gradients w.r.t. the gate PRE-activations; dW, dU, db and dx follow from
 * them as ptts_gemm products.  workspace: ptts_lstm_bwd_workspace_bytes */
size_t ptts_lstm_bwd_workspace_bytes(int B, int T, int H, int ndir);
int ptts_lstm_bwd(const float* dh_out /*[B,T,ndir*H]*/, const float* U, const float* gates, const float* c_out,
                  float* dgates, void* workspace, size_t workspace_bytes,
                  int B, int T, int H, int ndir, int reverse, void* stream);
/* ptts_lstm_bwd over a zero-padded batch with a length per row (masked training; lens as in ptts_lstm_fwd_ragged, gates and
 * c_out as that call stored them): on t < lens[b] dgates holds what ptts_lstm_bwd gives for that row alone (B = 1,
 * T = lens[b]), on t >= lens[b] +0.0f, whatever the pad frames of gates, c_out and dh_out hold -- they are not read.  The
 * same step-kernel paths, chosen the same way; the same workspace. */
int ptts_lstm_bwd_ragged(const float* dh_out, const float* U, const float* gates, const float* c_out, float* dgates,
                         const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir, int reverse,
                         void* stream);
/* Kept for bench.py, which reports these counters.  The replay of a recurrence's step launches as one hipGraph was removed
 * (HISTORY.md), so it writes 0 to each non-null output and returns PTTS_OK. */
int ptts_lstm_graph_stats(unsigned long long* hits, unsigned long long* captures, unsigned long long* direct);

/* ---------------------------------------------------------------------------------------
 * Keras GRU, reset_after = False (gates z, r, h; activation tanh, recurrent_activation
 * hard_sigmoid hs(a) = clip(0.2a + 0.5, 0, 1), the TF 1.x default; networktts.py:101-114).
 * ndir = 1: one direction, forwards; ndir = 2: kl.Bidirectional(concat), direction 0 forwards and
 * direction 1 backwards in the SAME launches.  Any H >= 1 (padded tail tiles).
 *   xproj [B,T,ndir*3H] = x.W_d + b_d per direction (ptts_gemm products);  U [ndir,H,3H]
 *   h_out [B,T,ndir*H] (the Bidirectional concat layout), gates (post-nonlinearity z, r, hh)
 *   [B,T,ndir*3H] and rh = r * h_{t-1} [B,T,ndir*H] are kept for the backward (rh is the
 *   operand of the candidate's recurrent-weight gradient).
 * Two launches per time step (r completes before (r*h).U_h starts); exact fp32 MFMA products
 * against the recurrent kernel packed into the workspace; no device memory is allocated.
 * ------------------------------------------------------------------------------------- */
size_t ptts_gru_fwd_workspace_bytes(int B, int T, int H, int ndir);    /* packed recurrent kernel */
int ptts_gru_fwd(const float* xproj, const float* U, float* h_out, float* gates, float* rh,
                 void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir, void* stream);
/* Forward for inference over a zero-padded batch with a length per row (see ptts_lstm_fwd_ragged): real frames as
 * ptts_gru_fwd on the row alone, bit for bit; pad frames 0.0f.  gates and rh may be NULL.  workspace:
 * ptts_gru_fwd_workspace_bytes followed by 2*ndir*B*H floats (z and r*h from a step's first launch to its second). */
int ptts_gru_fwd_ragged(const float* xproj, const float* U, float* h_out, float* gates /*or NULL*/, float* rh /*or NULL*/,
                        const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir,
                        void* stream);
/* dgates [B,T,ndir*3H] out: gradients w.r.t. the gate PRE-activations (hs' = 0.2 inside (0,1), 0
 * where clipped, taken from the stored gate); dx, dW, dU and db follow from them as ptts_gemm
 * products.  workspace: ptts_gru_bwd_workspace_bytes (packed U^T + the [ndir,B,H] carries) */
size_t ptts_gru_bwd_workspace_bytes(int B, int T, int H, int ndir);
int ptts_gru_bwd(const float* dh_out /*[B,T,ndir*H]*/, const float* U, const float* h_out, const float* gates,
                 float* dgates, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir, void* stream);
/* The same over a zero-padded batch with a length per row (masked training; h_out and gates as ptts_gru_fwd_ragged stored
 * them): real frames as ptts_gru_bwd on the row alone, pad frames of dgates +0.0f; pad frames of the inputs are not read. */
int ptts_gru_bwd_ragged(const float* dh_out, const float* U, const float* h_out, const float* gates, float* dgates,
                        const int* lens, void* workspace, size_t workspace_bytes, int B, int T, int H, int ndir, void* stream);

/* ---------------------------------------------------------------------------------------
 * Maximum-likelihood parameter generation (MLPG; external/merlin/mlpg_fast.py:95-135 as
 * modeltts.py:163-179 calls it): [B,T,K*D] statics + deltas -> the [B,T,D] trajectory.
 * K = 1 + number of windows (2 or 3); stream k of feature d is column k*D + d.  Per utterance
 * b and feature d one symmetric positive-definite pentadiagonal system of L = lengths[b] unknowns
 *   P = sum_k W_k^T diag(1/var_k) W_k,  b = sum_k W_k^T (mu_k / var_k),  out = P^-1 b,
 * W_0 = I, W_k[t,t+j] = wins[k-1][j+1] (taps outside the utterance dropped), and the variance
 * of the delta streams set to 1e11 at the utterance's first and last frame.  All B*D systems are
 * solved by one launch, one lane each, by an LDL^T sweep in fp64 (operands and result are fp32
 * in memory); a system's result does not depend on the rest of the batch.
 *   y       [B,T,K*D] the means, or the normalised network output when mean/std are given:
 *           mu = y*std + mean in fp64 (mean, std [K*D], both or neither)
 *   var     [K*D] (var_per_frame = 0: the same for every frame) or [B,T,K*D] (var_per_frame = 1)
 *   wins    [K-1][3] HOST memory, read before the call returns
 *   lengths [B] device int32 or NULL (every utterance has T frames).  A length is CLAMPED to
 *           [0, T]: nothing is read or written out of bounds and nothing is reported.
 *   out     [B,T,D]; frames t >= lengths[b] are written as 0
 * workspace: ptts_mlpg_workspace_bytes = 24 bytes per frame and system; no device allocation.
 * ------------------------------------------------------------------------------------- */
size_t ptts_mlpg_workspace_bytes(int B, int T, int D);
int ptts_mlpg(const float* y, const float* mean, const float* std, const float* var, int var_per_frame,
              const float* wins, const int* lengths, float* out, void* workspace, size_t workspace_bytes,
              int B, int T, int D, int K, void* stream);

/* ---------------------------------------------------------------------------------------
 * Feature composition (compose.py:34-183, 239-298): delta windows, per-column corpus statistics,
 * normalisers.  A chunk of N utterances is packed row-wise, [R, D] fp32, no padding; offsets [N+1]
 * device int32, utterance u owns rows offsets[u] .. offsets[u+1]-1 (clamped into [0, R]: nothing
 * is read or written out of bounds whatever offsets holds).
 *
 * ptts_compose_windows: out [R, K*D], K = 1 + number of windows (1 .. 8).  Columns 0..D-1 are y
 * bit for bit; window k (taps w = wins[k], fp64) fills columns (k+1)*D ..: for an utterance of T
 * frames and t in 1..T-2
 *   mlpg_order = 0:  -(w[2]*y[t-1] + w[1]*y[t] + w[0]*y[t+1])      (-scipy.signal.convolve(y, w))
 *   mlpg_order = 1:    w[0]*y[t-1] + w[1]*y[t] + w[2]*y[t+1]       (W_k y of ptts_mlpg)
 * in fp64, added left to right as written (oldest frame first), rounded once; frame 0 repeats frame 1, frame T-1 repeats frame T-2 (an
 * utterance shorter than 3 frames gets neighbours clamped into it: defined, not the reference's).
 * Fused statistics over utterances u < n_stat_utts (of this chunk): min and max of the fp32
 * results, sum of the fp64 values before rounding.  Two stages, no atomics: one partial per
 * utterance and column in the workspace (a function of that utterance's rows only), then the
 * partials are added in utterance order ONTO run_min / run_max [K*D] fp32 and run_sum [K*D] fp64,
 * which the caller initialises (+inf, -inf, 0) and carries from chunk to chunk: the result does
 * not depend on how a corpus is cut into chunks.  n_stat_utts = 0: no statistics, the running
 * buffers and the workspace may be NULL.
 *   wins  [K-1][3] doubles in HOST memory, read before the call returns (NULL for K = 1)
 * workspace: ptts_compose_windows_workspace_bytes(min(n_stat_utts, N), D, K); no device allocation.
 *
 * ptts_compose_sqdev: run_sq[c] += sum over the rows of utterances u < n_stat_utts of
 * (double(y[r,c]) - mean[c])^2, y [R, W] fp32 (composed rows), mean [W] DEVICE fp64; the centred
 * second pass of the standard deviation, same two stages and the same chunk invariance.
 * workspace: ptts_compose_sqdev_workspace_bytes(min(n_stat_utts, N), W).
 *
 * ptts_compose_normalise: out[r,j] = f(y[r, keepidx[j]]), y [R, Win], out [R, Wout], keepidx [Wout]
 * device int32 or NULL (then Wout = Win and out may be y).  fp32, numpy's operation order, IEEE
 * division, no contraction:
 *   PTTS_NORM_MEANSTD  (y - a[j]) / b[j]
 *   PTTS_NORM_MINMAX   ((((y - a[j]) / b[j]) - 0.5f) * 2.0f) * scale + offset
 * a, b [Wout] (already gathered).  Needs no workspace.
 * ------------------------------------------------------------------------------------- */
#define PTTS_NORM_MEANSTD 0
#define PTTS_NORM_MINMAX  1
size_t ptts_compose_windows_workspace_bytes(int N, int D, int K);
int ptts_compose_windows(const float* y, const int* offsets, const double* wins, int mlpg_order, float* out,
                         float* run_min, float* run_max, double* run_sum, int n_stat_utts, void* workspace,
                         size_t workspace_bytes, int N, int R, int D, int K, void* stream);
size_t ptts_compose_sqdev_workspace_bytes(int N, int W);
int ptts_compose_sqdev(const float* y, const int* offsets, const double* mean, double* run_sq, int n_stat_utts,
                       void* workspace, size_t workspace_bytes, int N, int R, int W, void* stream);
int ptts_compose_normalise(const float* y, const int* keepidx, const float* a, const float* b, int mode, float scale,
                           float offset, float* out, long long R, int Win, int Wout, void* stream);

/* ---------------------------------------------------------------------------------------
 * Spectral envelope decompression and the mel-cepstral post-filter (vocoders.py:147-166
 * decompress_spectrum; external/merlin/generate_pp.py mcep_postproc_sptk).  L = dftlen (even,
 * 8 .. 2^20), K = L/2 + 1 bins, w_k = 2 pi k / L, wt_k = w_k + 2 atan2(alpha sin w_k,
 * 1 - alpha cos w_k), |alpha| < 1.  Rows are contiguous; fp32 in memory, fp64 arithmetic, one
 * rounding of each result.  A frame's result depends on that frame only (no atomics).
 *
 *   logA_k(c) = sum_m c_m cos(m wt_k);   r0(x) = (1/L) (E_0 + E_{K-1} + 2 sum_{0<k<K-1} E_k),
 *   E_k = exp(2 x_k)
 *
 * ptts_mcep_postfilter: out [T, M1] from mcep [T, M1], M1 = 2 .. 512.  With c' = c * [1, 1, pf,
 *   pf, ...]:  out_0 = c_0 + ln(r0(logA(c)) / r0(logA(c'))) / 2,  out_m = c'_m (m >= 1).  One
 *   pass, nothing of size [T, K] is stored.
 * ptts_mcep2spec: spec [T, K] = exp(logA(c)) (log_out != 0: logA(c)); postfilter != 0: of the
 *   post-filtered cepstrum, which is not stored.
 * ptts_fwbnd2spec: fw [T, nb] log-amplitudes of nb = 2 .. 1024 bands with centres
 *   f_b = 700 (exp(b mel(fs/2) / ((nb-1) 1127)) - 1), mel(f) = 1127 ln(1 + f/700);
 *   logA_k = their linear interpolation (in Hz) at k fs / L.  postfilter != 0: with q_k the
 *   trapezoid weights of the nodes wt_k on [0, pi], c_0 = (1/pi) sum q_k logA_k,
 *   c_1 = (2/pi) sum q_k logA_k cos wt_k,  logA'_k = pf logA_k - (pf - 1) (c_0 + c_1 cos wt_k),
 *   spec_k = exp(logA'_k + ln(r0(logA) / r0(logA')) / 2).
 * T = 0 succeeds without a launch.
 *
 * Tables (device memory the CALLER keeps, one per parameter set; no device allocation here):
 *   ptts_mcep_table   [M1][Kp] fp32, Kp = K rounded up to 4: cos(m wt_k), for (M1, alpha, dftlen)
 *   ptts_fwbnd_table  [4][Kp] fp64: lower band, fraction, cos wt_k, q_k, for (nb, fs, alpha, dftlen)
 * built by one small launch on `stream`; 32-byte aligned.  The entry points above take the table
 * that was built with THEIR parameters: alpha (and fs, nb) are checked, the table's contents
 * are not (band indices read from it are clamped).
 *
 * ptts_spec2mcep: out [T, M1] mel-cepstra from x [T, K], the inverse of ptts_mcep2spec: with
 *   v_k = ln max(|x_k|, FLT_MIN) (is_log != 0: v_k = x_k, a log-envelope already), C[m,k] =
 *   cos(m wt_k) and the trapezoid weights q_k above, the weighted least-squares fit
 *     c = argmin sum_k q_k (v_k - sum_m c_m C[m,k])^2 = W v,   W = G^-1 C diag(q),  G = C diag(q) C^T,
 *   the exact left inverse of ptts_mcep2spec(log_out) for a cepstrum of the same order and the
 *   L2 projection on the warped axis otherwise (the discrete form of real cepstrum -> SPTK freqt).
 *   M1 = 2 .. min(512, floor((L/2) (1 - |alpha|) / (1 + |alpha|))): G has condition number about 2
 *   up to that order and turns singular beyond it (PTTS_EINVAL).  One [T, K] x [K, M1] product,
 *   fp64 accumulation in a fixed order.
 *   ptts_spec2mcep_table, for (M1, alpha, dftlen), all fp64: W first, [K][M1p] with M1p = M1 rounded
 *   up to 4, W[m,k] at table[k * M1p + m], zeros for M1 <= m < M1p; behind it the scratch of the
 *   build (the nodes wt_k, q_k; sum_k q_k cos(n wt_k), n <= 2 M1 - 2; the Cholesky factor of G),
 *   which ptts_spec2mcep does not read.  ptts_spec2mcep_table_bytes covers both; four small
 *   launches on `stream`; 32-byte aligned; a parameter set whose table would exceed 32 MiB is
 *   PTTS_EINVAL at both entry points.
 * ------------------------------------------------------------------------------------- */
size_t ptts_mcep_table_bytes(int M1, int dftlen);
int ptts_mcep_table(float* table, size_t table_bytes, int M1, double alpha, int dftlen, void* stream);
size_t ptts_fwbnd_table_bytes(int dftlen);
int ptts_fwbnd_table(double* table, size_t table_bytes, int nb, double fs, double alpha, int dftlen, void* stream);
int ptts_mcep_postfilter(const float* mcep, float* out, int T, int M1, double alpha, int dftlen, double pf_coef,
                         const float* table, size_t table_bytes, void* stream);
int ptts_mcep2spec(const float* mcep, float* spec, int T, int M1, double alpha, int dftlen, int log_out, int postfilter,
                   double pf_coef, const float* table, size_t table_bytes, void* stream);
int ptts_fwbnd2spec(const float* fw, float* spec, int T, int nb, double fs, double alpha, int dftlen, int log_out,
                    int postfilter, double pf_coef, const double* table, size_t table_bytes, void* stream);
size_t ptts_spec2mcep_table_bytes(int M1, int dftlen);
int ptts_spec2mcep_table(double* table, size_t table_bytes, int M1, double alpha, int dftlen, void* stream);
int ptts_spec2mcep(const float* x, float* out, int T, int M1, double alpha, int dftlen, int is_log, const double* table,
                   size_t table_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Pulse-and-noise waveform synthesis of the PML vocoder (csrc/pulsesynth.hip; the definition
 * is this build's own).  L = dftlen, a power of two in 256 .. 8192 (anything
 * else: PTTS_EINVAL without a launch), K = L/2 + 1.  fp32 in memory, fp64 arithmetic.
 *
 * ptts_noise_mask: nmb [T, nb] band values, f0 [T] Hz -> out [T, K]: the bands interpolated at
 *   k fs / L with the band / fraction rows of ptts_fwbnd_table(nb, fs, ., dftlen), bins below
 *   int(2 f0 L / fs) zeroed, thresholded (> 0.5 -> 1), smoothed along k by the 17 taps w * w,
 *   w = hanning(9) / 4, over the odd extension of the row, clipped to [0, 1].
 * ptts_pulse_segments: one workgroup per pulse; seg [P][W] gets the first winlen samples of
 *   irfft(E ((1 - m) D + m N)) (the rest of a row is neither written nor read).  spec, mask
 *   [T, K]; noise [wavlen] N(0,1) samples; itab [5][P] int32 rows start, winlen, lb, rb, fr
 *   (winlen <= W <= L, 0 <= lb <= rb <= wavlen, 0 <= fr < T; a pulse whose row breaks this is
 *   skipped); dtab [2][P] fp64 rows delay, f0.  P = 0 or T = 0 succeeds without a launch.
 * ptts_pulse_overlap_add: wav[j] = sum over the pulses with start <= j < start + winlen of
 *   seg[n][j - start], in pulse order, one lane per sample, no atomics; start is ascending.
 * ------------------------------------------------------------------------------------- */
int ptts_noise_mask(const float* nmb, const float* f0, float* out, int T, int nb, double fs, int dftlen, const double* table,
                    size_t table_bytes, void* stream);
int ptts_pulse_segments(const float* spec, const float* mask, const float* noise, const int* itab, const double* dtab, int P, int T,
                        int dftlen, double fs, long long wavlen, float* seg, int W, void* stream);
int ptts_pulse_overlap_add(const float* seg, const int* itab, int P, int W, float* wav, long long wavlen, void* stream);

/* ---------------------------------------------------------------------------------------
 * Periodic-plus-aperiodic waveform synthesis for the WORLD parameters (csrc/worldsynth.hip; the
 * definition is this build's own).  L = dftlen, a power of two in 256 .. 8192
 * (anything else: PTTS_EINVAL without a launch), K = L/2 + 1.  fp32 in memory, fp64 arithmetic.
 *
 * ptts_aper_rows: aper [T, nb] band aperiodicities in dB, vuv [T] -> out [T, K]: 10^(x/20) per
 *   band, those values interpolated at k fs / L with the band / fraction rows of
 *   ptts_fwbnd_table(nb, fs, ., dftlen), clipped to [0, 1]; the row of a frame with vuv < 0.5 is 1.
 * ptts_world_segments: one workgroup per pulse; seg [P][W] gets the first winlen samples of
 *   irfft(E_p D + E_a N) (the rest of a row is neither written nor read).  spec (amplitude), aper
 *   (rows of ptts_aper_rows) [T, K], blended as (1 - w) row i0 + w row i1; E_a the minimum phase of
 *   spec aper, E_p that of spec sqrt(1 - aper^2) hp for a pulse with v = 1 and 0 otherwise; noise
 *   [wavlen] N(0,1) samples; itab [8][P] int32 rows start, winlen, lb, rb, fr, i0, i1, v
 *   (winlen <= W <= L, 0 <= lb <= rb <= wavlen, start <= lb and rb - start <= L where lb < rb,
 *   0 <= fr, i0, i1 < T; a pulse whose row breaks this is skipped); dtab [3][P] fp64 rows delay,
 *   f0, w (0 <= w <= 1).  P = 0 or T = 0 succeeds without a launch.  The segments are summed by
 *   ptts_pulse_overlap_add, which reads the first two rows of itab.
 * ------------------------------------------------------------------------------------- */
int ptts_aper_rows(const float* aper, const float* vuv, float* out, int T, int nb, double fs, int dftlen, const double* table,
                   size_t table_bytes, void* stream);
int ptts_world_segments(const float* spec, const float* aper, const float* noise, const int* itab, const double* dtab, int P, int T,
                        int dftlen, double fs, long long wavlen, float* seg, int W, void* stream);

/* ---------------------------------------------------------------------------------------
 * The pulse table of the two synthesisers on the device, for a batch of utterances (csrc/pulsetable.hip;
 * the definition is ops.pulse_table's and ops.world_pulse_table's, DESIGN.md section 3, reproduced bit
 * for bit: fp64, no contraction).  B utterances are packed one after the other: f0 [sum T] in Hz,
 * voiced [sum T] bytes (NULL: the PML form, otherwise the WORLD form), offs [2][B+1] int64 with the
 * utterances' first frames in row 0 and first samples in row 1 (wavlen_b = round(shift (T_b - 1) fs),
 * computed by the caller).  cap: pulse slots per utterance.
 *
 * ptts_pulse_walk: one wave per utterance; t [B][cap] gets t_0 = 0, t_{n+1} = t_n + 1 / rate(t_n) while
 *   t_n < wavlen_b / fs; info [B][4] int32 gets the pulse count (<= cap), the largest winlen, the walk's
 *   status bits and a zero for ptts_pulse_rows.  An utterance that sets a bit is not walked further.
 * ptts_pulse_rows: one lane per pulse; P = the sum of the counts, known on the device only.  itab_rel
 *   and itab_off get the int32 rows start, winlen, lb, rb, fr (WORLD: i0, i1, v) at [row * P + pulse],
 *   relative to the own utterance and offset into the packed frames / samples (there winlen = 0 for
 *   the pulse of an utterance with wavlen_b = 0); dtab the fp64 rows delay, f0 (WORLD: w).  The three
 *   buffers hold 5 (8), 5 (8) and 2 (3) times B * cap values.  pulse_off [B+1] gets the utterances'
 *   first pulses; info[b][3] the rows' status bits.  An utterance the walk refused gets no rows.
 * ptts_pulse_overlap_add_batch: ptts_pulse_overlap_add over packed utterances; a sample sums the
 *   pulses of its own utterance (pulse_off, samp_off [B+1]), start ascending within each.
 * ------------------------------------------------------------------------------------- */
#define PTTS_PULSE_BAD_F0 1          /* f0 not finite or not positive */
#define PTTS_PULSE_WINDOW 2          /* a window does not fit dftlen */
#define PTTS_PULSE_TOO_MANY 4        /* more than cap pulses */
#define PTTS_PULSE_RATE 8            /* a rate above f0_cap */
#define PTTS_PULSE_DESCENDING 16     /* starts not ascending */
#define PTTS_PULSE_SEGMENT 32        /* a noise segment outside the waveform or its pulse's frame */
#define PTTS_PULSE_START_RANGE 64    /* |start| >= 2^30 */
int ptts_pulse_walk(const float* f0, const unsigned char* voiced, const long long* offs, int B, double shift, double fs, int dftlen,
                    int cap, double f0_cap, double* t, int* info, void* stream);
int ptts_pulse_rows(const float* f0, const unsigned char* voiced, const long long* offs, int B, double shift, double fs, int dftlen,
                    int cap, const double* t, int* info, int* pulse_off, int* itab_rel, int* itab_off, double* dtab, void* stream);
int ptts_pulse_overlap_add_batch(const float* seg, const int* itab, const int* pulse_off, const long long* samp_off, int B, int P,
                                 int W, float* wav, long long wavlen, void* stream);

/* ---------------------------------------------------------------------------------------
 * Waveform analysis for the PML parameters (csrc/analysis.hip; the counterpart of the synthesis
 * above, the definition is this build's own).  L = dftlen, K = L/2 + 1,
 * rnd(x) = floor(x + 0.5).  fp32 in memory, fp64 arithmetic, every integer decision in fp64.
 *
 * ptts_frame_harmonics: one workgroup per frame; L a power of two in 256 .. 8192.  wav [N] at fs,
 *   f0 [T] Hz (positive; frame i at i shift), Hcap: columns of u, at least H_i - 1 for every
 *   frame, H_i = floor((fs/2 - f0_i/2) / f0_i).  A Blackman window of 2 int(1.5 fs / f0_i) + 1
 *   samples around rnd(i shift fs), normalised to sum 1, zero-phase; its transform's peak in each
 *   harmonic's stretch of bins times fs / f0_i gives a_h; spec [T, K] = exp of a_h interpolated in
 *   Hz (log_out != 0: the logarithm itself); u [T, Hcap, 2] = the unit phasor of
 *   X[k_{h+1}] conj(X[k_h]) conj(X[k_1]), k_h = rnd(h f0_i L / fs), at column h - 1, (0, 0) behind
 *   H_i - 1.  A frame whose window does not fit L or that has more than Hcap + 1 harmonics is
 *   skipped: nothing of it is read or written.
 * ptts_phase_coherence: R [T, Hcap] = |sum of u over the frames within J_i = max(2, rnd(1 / (f0_i
 *   shift))) of frame i that have the harmonic| / their number (1 behind H_i - 1); nm [T, nb] =
 *   the hat-weighted share of bins in each band whose harmonic has R < exp(-0.75^2 / 2).
 * ptts_fwbnd_compress: x [T, K] -> out [T, nb] on the band axis of ptts_fwbnd2spec, with W[k,b]
 *   the weight with which ptts_fwbnd2spec reads band b at bin k.  PTTS_COMPRESS_MEAN:
 *   sum_k W[k,b] x[k] / sum_k W[k,b].  PTTS_COMPRESS_LSQ: the least-squares solution y of
 *   W y = v, v = ln max(|x|, FLT_MIN) (is_log != 0: v = x), the exact left inverse of
 *   ptts_fwbnd2spec(log) wherever every band has weight.  dftlen even, 8 .. 2^20.
 * Tables: fwtable is ptts_fwbnd_table(nb, fs, ., dftlen); ctable [6][nb rounded up to 4] fp64 is
 *   built from it by ptts_fwbnd_compress_table, one small launch (a band's first and last + 1 bin,
 *   sum_k W[k,b], and the factors of the tridiagonal W^T W); 32-byte aligned, the CALLER keeps
 *   both.  Indices read from the tables are clamped.  T = 0 succeeds without a launch.
 * ------------------------------------------------------------------------------------- */
#define PTTS_COMPRESS_MEAN 0
#define PTTS_COMPRESS_LSQ  1
int ptts_frame_harmonics(const float* wav, long long N, const float* f0, float* spec, float* u, int T, int Hcap, double shift,
                         double fs, int dftlen, int log_out, void* stream);
int ptts_phase_coherence(const float* u, const float* f0, float* R, float* nm, int T, int Hcap, int nb, double shift, double fs,
                         int dftlen, const double* fwtable, size_t fwtable_bytes, const double* ctable, size_t ctable_bytes,
                         void* stream);
size_t ptts_fwbnd_compress_table_bytes(int nb);
int ptts_fwbnd_compress_table(double* ctable, size_t ctable_bytes, const double* fwtable, size_t fwtable_bytes, int nb, int dftlen,
                              void* stream);
int ptts_fwbnd_compress(const float* x, float* out, int T, int nb, int dftlen, int mode, int is_log, const double* fwtable,
                        size_t fwtable_bytes, const double* ctable, size_t ctable_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Waveform analysis for the WORLD parameters (csrc/worldanalysis.hip; the counterpart of
 * ptts_world_segments, the definition is this build's own).  L = dftlen, a
 * power of two in 256 .. 8192 (anything else: PTTS_EINVAL without a launch; both kernels fit the
 * 160 KiB of LDS at 8192, so there is no lower cap), K = L/2 + 1, rnd(x) = floor(x + 0.5).  fp32
 * in memory, fp64 arithmetic, every integer decision in fp64.  One workgroup per frame; frame i is
 * centred at c = rnd(i shift fs); wav [N] at fs, no sample outside [0, N) is read.  The window at
 * rate r is w_j = 0.5 + 0.5 cos(pi j / (hw + 1)), j = -hw .. hw, hw = int(1.5 fs / r), scaled to
 * sum w^2 = 1, placed zero-phase.  A frame with r outside (0, fs/2) or 2 hw + 1 > L is skipped:
 * nothing of it is read or written.  T = 0 succeeds without a launch.
 *
 * ptts_world_envelope: rate [T] Hz (f0 of a voiced frame, 500 for an unvoiced one) -> spec [T, K],
 *   the amplitude envelope ptts_world_segments reads (log_out != 0: its logarithm).  P = |rfft|^2
 *   of the frame; below kappa = r L / fs, P_k += P(kappa - k) (linear between bins); the mean of P
 *   over k +- d, d = r L / (3 fs), bins as cells of width 1 mirrored at 0 and L/2;
 *   la = ln max(sqrt(S fs / r), 1e-10); the cepstrum of la times
 *   sinc(r q / fs) (1.3 - 0.3 cos(2 pi r q / fs)) goes back to ln spec.  Three transforms a frame.
 * ptts_world_aperiodicity: f0 [T] Hz, voiced [T] (>= 0.5: voiced) -> aper [T, nb] dB in [-60, 0]
 *   on the band axis of fwtable = ptts_fwbnd_table(nb, fs, ., dftlen) (32-byte aligned, the CALLER
 *   keeps it; band indices read from it are clamped), nb in 2 .. 1024.  Voiced: n0 = rnd(fs / f0),
 *   delta = fs / f0 - n0, X1 and X2 the transforms of the frames at c - (n0 >> 1) and n0 samples
 *   later, X2_k turned by exp(+2 pi i k delta / L); rho_b = sum_k W[k,b] |X1_k - X2_k|^2 /
 *   sum_k W[k,b] (|X1_k|^2 + |X2_k|^2) over the bins k >= f0 L / fs (W as in ptts_fwbnd_compress);
 *   aper = 10 log10(clip(rho, 1e-6, 1)); a band without weight takes the nearest band above that
 *   has some, else 0 dB.  Unvoiced: the row is 0 dB and no transform runs.
 * ------------------------------------------------------------------------------------- */
int ptts_world_envelope(const float* wav, long long N, const float* rate, float* spec, int T, double shift, double fs, int dftlen,
                        int log_out, void* stream);
int ptts_world_aperiodicity(const float* wav, long long N, const float* f0, const float* voiced, float* aper, int T, int nb,
                            double shift, double fs, int dftlen, const double* fwtable, size_t fwtable_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * F0 estimation (csrc/f0.hip; the track the analysis above takes as `f0`; the definition is this
 * build's own, DESIGN.md section 3, after Boersma 1993: the autocorrelation method with a path
 * finder).  L = dftlen, rnd(x) = floor(x + 0.5).  fp32 in memory, fp64 arithmetic, every decision
 * in fp64.  hw = int(1.5 fs / f0_min), W = 2 hw + 1, lmin = ceil(fs / f0_max),
 * lmax = floor(fs / f0_min).
 *
 * ptts_f0_candidates: one workgroup per frame; L a power of two in 256 .. 8192 with
 *   W + lmax + 1 <= L and 0 < f0_min <= f0_max <= fs/2 (anything else: PTTS_EINVAL without a
 *   launch), ncand = 2 .. 16 slots.  The W samples of wav [N] around rnd(i shift fs) (none outside
 *   [0, N) is read), less their mean, under w[j] = 0.5 - 0.5 cos(2 pi (j + 1) / (W + 1)); the power
 *   spectrum weighted by G (1 up to 2.5 f0_max, a cos^2 roll-off to 0 at 3.75 f0_max) goes back to
 *   the autocorrelation rho, r[k] = (rho[k] / rho[0]) / rw[k], k = 0 .. lmax + 1 (0 unless
 *   rho[0] > 0).  rw [lmax + 2] fp64 is the CALLER's table of the window's own normalised
 *   autocorrelation sum_j w[j] w[j+k] / sum_j w[j]^2 (device memory, 8-byte aligned; its contents
 *   are not checked).  Slot 0 of a frame is the unvoiced candidate: freq 0, strength
 *   voicing_threshold + max(0, 2 - (lpeak / gpeak) / (silence_threshold / (1 + voicing_threshold))),
 *   lpeak the frame's largest |sample - mean|, gpeak the waveform's as the host measured it
 *   (gpeak = 0: voicing_threshold + 2).  Slots 1 .. n_i are the lags k in [lmin, lmax] with
 *   r[k] > r[k-1], r[k] >= r[k+1], r[k] > voicing_threshold / 2, refined by the parabola through
 *   the three values to (tau, peak), F = 1 / tau within [f0_min, f0_max], strength
 *   min(peak, 1) - octave_cost log2(f0_min tau): the ncand - 1 strongest, strongest first, ties to
 *   the smaller lag.  Out: freq, strength [T, ncand] fp32, n [T] and lag [T, ncand] int32 (the
 *   integer lag of a kept candidate), zeros in the slots behind n_i; r [T, lmax + 2] fp32 or NULL.
 * ptts_f0_viterbi: one wave64 for the utterance.  cost_0[j] = -S[0,j], cost_i[j] = min_p
 *   (cost_{i-1}[p] + (0.01 / shift) trans(p, j)) - S[i,j] over the slots 0 .. n_i (n clamped to
 *   [0, ncand - 1]), ties to the smaller p; trans = 0 between unvoiced slots,
 *   voiced_unvoiced_cost between a voiced and an unvoiced one, octave_jump_cost
 *   |log2 F_p - log2 F_j| between voiced ones.  The cheapest slot of the last frame (ties to the
 *   smaller) is followed back: f0 [T] = the chosen slot's freq, 0 for slot 0; path [T] int32 (or
 *   NULL) = the slot.  Back-pointers live in LDS, so T <= ptts_f0_viterbi_max_frames(ncand)
 *   (32768 up to ncand = 8, 16384 above; 0 for an ncand outside 2 .. 16): more is PTTS_EINVAL.
 * ptts_f0_refine: the instantaneous frequency of the harmonics around a given track (after the
 *   published StoneMask; the definition is this build's own), one workgroup per frame, no
 *   transform.  c = rnd(i shift fs), f = f0[i]; out [T] fp32, status [T] int32 or NULL:
 *   1. f > 0 is false (NaN included): out 0, status 0 (unvoiced).
 *   2. f < f0_min or f > f0_max: out f, status 2; nothing of the waveform is read.
 *   3. hw = rnd(1.5 fs / f), j = -hw .. hw; c - hw < 0 or c + hw >= N: out f, status 2.
 *   4. u = j / (2 (hw + 1)), w_j = 0.42 + 0.5 cos(2 pi u) + 0.08 cos(4 pi u), its derivative per
 *      sample w'_j = -(pi / (hw + 1)) (0.5 sin(2 pi u) + 0.16 sin(4 pi u)).
 *   5. X(nu) = sum_j wav[c + j] w_j e^{-2 pi i nu j / fs}, Xd(nu) the same sum with w'_j,
 *      IF(nu) = nu - (fs / 2 pi) (Im Xd Re X - Re Xd Im X) / |X|^2.
 *   6. A pass with H harmonics from g: h = 1 .. H, stopping at the first h with h g >= fs/2;
 *      nu = h g; a harmonic whose |X|^2 > 0 is false is skipped; num += |X| IF(nu),
 *      den += |X| h.  den > 0 is false: out f, status 3.  Otherwise g = num / den.
 *   7. Two passes: H = 2 from g = f, then H = 6 from the result; the window stays that of f.
 *   8. g finite, |g / f - 1| <= 0.2 and f0_min <= g <= f0_max: out (float) g, status 1;
 *      otherwise out f, status 3.
 *   PTTS_EINVAL without a launch unless 0 < f0_min <= f0_max <= fs/2, shift > 0, fs > 0,
 *   2 rnd(1.5 fs / f0_min) + 1 <= 16384, T >= 0, N >= 0 and wav (unless N = 0), f0, out are not
 *   NULL.  N = 0 with T > 0 is legal: every voiced frame gets status 2.  Frames are independent,
 *   no atomics: the same input gives the same bytes.
 * T = 0 succeeds without a launch.
 * ------------------------------------------------------------------------------------- */
int ptts_f0_candidates(const float* wav, long long N, const double* rw, size_t rw_bytes, float* freq, float* strength, int* n,
                       int* lag, float* r, int T, int ncand, double shift, double fs, int dftlen, double f0_min, double f0_max,
                       double gpeak, double voicing_threshold, double silence_threshold, double octave_cost, void* stream);
int ptts_f0_viterbi_max_frames(int ncand);
int ptts_f0_viterbi(const float* freq, const float* strength, const int* n, float* f0, int* path, int T, int ncand, double shift,
                    double octave_jump_cost, double voiced_unvoiced_cost, void* stream);
int ptts_f0_refine(const float* wav, long long N, const float* f0, float* out, int* status /* or NULL */, int T,
                   double shift, double fs, double f0_min, double f0_max, void* stream);

/* ---------------------------------------------------------------------------------------
 * Waveform analysis over a batch of utterances (csrc/analysisbatch.hip and the *_batch kernels of
 * csrc/f0.hip, csrc/analysis.hip, csrc/worldanalysis.hip).  B <= 65535 utterances are packed one
 * after the other: wav [wav_total] fp32 with wav_off [B+1], every per-frame tensor [T, ..] with
 * frame_off [B+1], T the packed total (the <= 2^31 row limits of the single forms apply to it);
 * the offsets are int64 in DEVICE memory, ascending from 0.  Global frame g of utterance b is that
 * utterance's frame i = g - frame_off[b], centred at rnd(i shift fs) in its own waveform of
 * N_b = wav_off[b+1] - wav_off[b] samples; a workgroup finds b by a binary search in frame_off.
 * An utterance whose offsets do not lie inside the totals is skipped: nothing of it is read or
 * written.  Each launch runs once for the whole batch; no atomics, nothing between workgroups.
 *
 * ptts_f0_candidates_batch, ptts_f0_refine_batch, ptts_frame_harmonics_batch,
 * ptts_world_envelope_batch, ptts_world_aperiodicity_batch: the single form's frame, computed by
 *   the same device function on the utterance's samples and rows, so utterance b's rows are, bit
 *   for bit, what the single entry point writes for that utterance alone.  ptts_f0_candidates_batch
 *   reads each utterance's gpeak from gpeak [B] fp64 in device memory (ptts_wave_peak's, or the
 *   caller's; a value that is not finite or negative counts as 0).
 * ptts_phase_coherence_batch: as above; the neighbourhood i - J_i .. i + J_i and the clamp
 *   J_i <= T_b are those of the frame's own utterance, never a neighbour's rows.
 * ptts_f0_viterbi_batch: grid B, one wave64 per utterance with its own back-pointers in LDS.
 *   max_frames: the longest utterance (the LDS of a workgroup), at most
 *   ptts_f0_viterbi_max_frames(ncand): the cap is per utterance, not for the batch.  A longer
 *   utterance is skipped.
 * ptts_wave_peak: one workgroup per utterance; gpeak [B] fp64 = max |x - mean(x)| over the
 *   utterance's fp32 samples in fp64, the mean by a fixed-order sum (the same input gives the same
 *   bytes); 0 for N_b = 0.  A sample that is not finite: gpeak 0 and PTTS_ANALYSIS_BAD_WAV.
 * ptts_f0_track: ops.f0_track for every utterance, one workgroup each.
 *   f0 [in_total] Hz, fp32 or (f0_is_double != 0) fp64, <= 0 unvoiced, packed by in_off [B+1];
 *   the unvoiced stretches are interpolated linearly over the frame index between their voiced
 *   neighbours (numpy.interp restated in fp64: the end values held), clipped to [f0_min, f0_max],
 *   rounded to fp32 and moved by one ulp where the rounding left the interval; the first
 *   Tout_b = out_off[b+1] - out_off[b] <= T_b frames go to track [out_total] fp32, and
 *   vuv [out_total] = 1 where f0 > 0, else 0.  An utterance without frames or with a value that
 *   is not finite: PTTS_ANALYSIS_BAD_F0; without a voiced frame: PTTS_ANALYSIS_NO_VOICED; such
 *   an utterance gets no rows.
 * info [B] int32: the status bits of an utterance are OR-ed into info[b]; the CALLER zeroes it
 *   before the first launch and reads it back once after the last.
 * T = 0 or B = 0 succeeds without a launch.
 * ------------------------------------------------------------------------------------- */
#define PTTS_ANALYSIS_BAD_WAV 1      /* a sample of the waveform is not finite */
#define PTTS_ANALYSIS_BAD_F0 2       /* the track is empty or has a value that is not finite */
#define PTTS_ANALYSIS_NO_VOICED 4    /* the track has no voiced frame */
int ptts_wave_peak(const float* wav, const long long* wav_off, long long wav_total, int B, double* gpeak, int* info, void* stream);
int ptts_f0_track(const void* f0, int f0_is_double, const long long* in_off, long long in_total, const long long* out_off,
                  long long out_total, int B, float* track, float* vuv, int* info, double f0_min, double f0_max, void* stream);
int ptts_f0_candidates_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B, int T,
                             const double* rw, size_t rw_bytes, float* freq, float* strength, int* n, int* lag, float* r /* or NULL */,
                             int ncand, double shift, double fs, int dftlen, double f0_min, double f0_max, const double* gpeak,
                             double voicing_threshold, double silence_threshold, double octave_cost, void* stream);
int ptts_f0_viterbi_batch(const float* freq, const float* strength, const int* n, float* f0, int* path /* or NULL */,
                          const long long* frame_off, int B, int T, int max_frames, int ncand, double shift, double octave_jump_cost,
                          double voiced_unvoiced_cost, void* stream);
int ptts_f0_refine_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B, int T,
                         const float* f0, float* out, int* status /* or NULL */, double shift, double fs, double f0_min, double f0_max,
                         void* stream);
int ptts_frame_harmonics_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B, int T,
                               const float* f0, float* spec, float* u, int Hcap, double shift, double fs, int dftlen, int log_out,
                               void* stream);
int ptts_phase_coherence_batch(const float* u, const float* f0, float* R, float* nm, const long long* frame_off, int B, int T, int Hcap,
                               int nb, double shift, double fs, int dftlen, const double* fwtable, size_t fwtable_bytes,
                               const double* ctable, size_t ctable_bytes, void* stream);
int ptts_world_envelope_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B, int T,
                              const float* rate, float* spec, double shift, double fs, int dftlen, int log_out, void* stream);
int ptts_world_aperiodicity_batch(const float* wav, const long long* wav_off, long long wav_total, const long long* frame_off, int B,
                                  int T, const float* f0, const float* voiced, float* aper, int nb, double shift, double fs, int dftlen,
                                  const double* fwtable, size_t fwtable_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * DTW alignment of utterance pairs of unequal length (csrc/dtw.hip; the build's own definition,
 * DESIGN.md section 3; the reference has no counterpart).  G [g_total, D] generated and
 * R [r_total, D] reference rows, fp32, B <= 65535 pairs packed one after the other by g_off and
 * r_off [B+1] (int64, DEVICE memory, as for the analysis batch); pair b has Tg = g_off[b+1] -
 * g_off[b] and Tr = r_off[b+1] - r_off[b] frames.
 *   local cost   c(i,j) = sqrt( sum_{d=c0}^{c1-1} (scale (G[i,d] - R[j,d]))^2 ) in fp64, the
 *                columns added in index order, one IEEE square root, no contraction
 *   accumulated  A(0,0) = c(0,0); A(i,j) = c(i,j) + min(A(i-1,j-1), A(i-1,j), A(i,j-1)), fp64; a
 *                predecessor outside the matrix does not take part.  TIE RULE: the diagonal
 *                predecessor wins a tie, then (i-1,j), then (i,j-1) -- a candidate replaces the
 *                best so far only if it is strictly smaller, tried in that order
 *   path         the back-pointers from (Tg-1, Tr-1) to (0,0), reported FORWARDS as gi[k], ri[k],
 *                k = 0 .. L-1, max(Tg,Tr) <= L <= Tg+Tr-1, in the pair's slots path_off[b] ..
 *                path_off[b] + Tg + Tr - 2 of gi, ri [path_total] int32 (path_off [B+1] int64
 *                DEVICE memory; only the first L slots are written); L [B] int32; cost [B] fp64 =
 *                A(Tg-1,Tr-1)
 * info [B] int32 is WRITTEN (not OR-ed into): 0, or the PTTS_DTW_* bits of a pair that is not
 * aligned -- it gets L = 0 and cost NaN, nothing of it is read or written out of bounds, and its
 * neighbours are not affected.  PTTS_DTW_NOT_FINITE is set by the cost pass (a vector atomic OR).
 * max_gen, max_ref: the longest Tg and Tr as the host measured them (the grid of the cost pass),
 * each at most ptts_dtw_max_frames() = 2048 (three diagonals of A in LDS); a longer pair is
 * PTTS_DTW_TOO_LONG.  cells: sum Tg Tr over the batch as the host measured it (the workspace).
 * Workspace: ptts_dtw_workspace_bytes(cells, B, path_total) bytes (0 for arguments out of range),
 * 256-byte aligned: the cell offsets, the fp64 local costs and the back-pointer bytes, both
 * skewed (diagonal-major), and the backward paths; a shorter one is PTTS_EWORKSPACE.
 * phases: PTTS_DTW_PHASE_ALL; a subset runs only those launches on what an earlier call left in
 * the same workspace (tools/dtw_probe.py times them one by one).
 * No atomics on results, nothing between workgroups: the same input gives the same bytes and a
 * pair's result depends on nothing but that pair.  B = 0 succeeds without a launch; D < 1, a
 * column range that is not 0 <= c0 < c1 <= D, a scale that is not finite or a null pointer is
 * PTTS_EINVAL without a launch.
 * ------------------------------------------------------------------------------------- */
#define PTTS_DTW_EMPTY 1            /* Tg = 0 or Tr = 0 */
#define PTTS_DTW_TOO_LONG 2         /* Tg > max_gen or Tr > max_ref */
#define PTTS_DTW_NOT_FINITE 4       /* a local cost is not finite */
#define PTTS_DTW_BAD_OFFSETS 8      /* the offsets do not lie inside the totals, or the cells exceed `cells` */
#define PTTS_DTW_PHASE_COSTS 1      /* the layout and the local costs */
#define PTTS_DTW_PHASE_WAVEFRONT 2  /* the accumulated costs and the back-pointers */
#define PTTS_DTW_PHASE_BACKTRACK 4  /* the path, backwards, and its reversal */
#define PTTS_DTW_PHASE_ALL 7
int ptts_dtw_max_frames(void);
size_t ptts_dtw_workspace_bytes(long long cells, int B, long long path_total);
int ptts_dtw_align_batch(const float* G, const long long* g_off, long long g_total, const float* R, const long long* r_off,
                         long long r_total, int B, int D, int c0, int c1, double scale, int max_gen, int max_ref, long long cells,
                         const long long* path_off, long long path_total, int* gi, int* ri, int* L, double* cost, int* info,
                         int phases, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Forced alignment by flat-start Viterbi training (segmental k-means; csrc/align.hip; the build's
 * own definition; the reference has no counterpart and nothing is claimed
 * about HTK's numbers).  Monophone, left-to-right, no skips, one diagonal Gaussian per state, no
 * transition probabilities.  All arithmetic fp64; the features fp32 in memory.
 *   chain       utterance b is a chain of N = state_off[b+1] - state_off[b] states in a fixed order
 *               over T = frame_off[b+1] - frame_off[b] rows of X [t_total, Dx] (offsets [B+1] int64
 *               in DEVICE memory, B <= 65535).  Chain state n uses the Gaussian gauss[state_off[b]
 *               + n] in [0, Q) (gauss [n_total] int32); the kernels know nothing else about phones
 *   emission    e(t,n) = -0.5 (sum_d ((x_d - mu[q,d]) (x_d - mu[q,d])) w[q,d] + g[q]), x = X[t, c0:c1],
 *               D = c1 - c0, q = gauss[n]; the columns added in index order, no contraction.
 *               mu, w [Q,D] and g [Q] fp64: w = 1 / var, g = sum_d log var[q,d]; the constant
 *               D log 2 pi is dropped
 *   alignment   V(0,0) = e(0,0), V(0,n>0) unreachable; V(t,n) = e(t,n) + max(V(t-1,n), V(t-1,n-1)),
 *               an unreachable predecessor does not take part.  TIE RULE: staying wins -- the
 *               advance from n-1 replaces it only if it is strictly greater.  The path is followed
 *               back from (T-1, N-1).  dur [n_total] int32: frames in chain state n, every dur >= 1
 *               and sum dur = T; state [t_total] int32 (or NULL): the chain state of frame t;
 *               score [B] fp64 = V(T-1,N-1)
 * info [B] int32 is WRITTEN (not OR-ed into): 0, or the PTTS_ALIGN_* bits of an utterance that is
 * not aligned -- it gets dur = zeros, state = -1 and score = NaN (with PTTS_ALIGN_BAD_OFFSETS the
 * score alone: its slots are not known); nothing else of it is read or written, and every other
 * utterance of the batch comes out exactly as it does alone.  NOT_FINITE and BAD_GAUSS are set by
 * the emission pass (a vector atomic OR on the flag word).
 * cells: sum T N over the utterances that can be aligned, as the host measured it (the workspace);
 * an utterance that does not fit into what is left of it is PTTS_ALIGN_BAD_OFFSETS.
 * Workspace: ptts_align_workspace_bytes(cells, B, t_total) bytes (0 for arguments out of range),
 * 256-byte aligned: two offset arrays, the time loop's scores, the fp64 emissions row-major
 * (a row of N rounded up to the states of a lane, at most 31 more) and 64 back-pointer words per
 * frame; a shorter one is PTTS_EWORKSPACE.
 * phases: PTTS_ALIGN_PHASE_ALL; a subset runs only those launches on what an earlier call left in
 * the same workspace (tools/align_probe.py times them one by one).  The outputs are written by
 * the backtrack phase.
 * ptts_align_accumulate: count[q] += frames, s1[q,d] += sum x_d, s2[q,d] += sum x_d x_d (count
 * [Q] int64, s1 and s2 [Q,D] fp64) over the frames whose chain state uses q, ADDED to what the
 * arrays hold, so that a corpus goes through in several calls; a Gaussian without frames in the
 * call is left untouched.  occ [n_total] int32: the indices into gauss / dur of the chain states,
 * sorted by Gaussian (the host built gauss); occ_off [Q+1] int64: Gaussian q's run of occ (both
 * DEVICE memory).  An entry whose state does not use q, and an utterance whose dur are negative
 * or sum to more than its frames (a flagged one has zeros), add nothing.  The frames of a
 * Gaussian are added in a fixed order, four partial sums in the table's order, then those four.
 * Workspace: ptts_align_accumulate_workspace_bytes(n_total) (the first row of every state).
 * ptts_align_update: for count[q] >= min_count (>= 1): mu = s1 / count, var = max(s2 / count -
 * mu mu, floor[d]), w = 1 / var, g = sum_d log var in index order; kept[q] = 0 and floored[q] =
 * the variances that took the floor.  Below min_count mu, w, g stay and kept[q] = 1.
 * No floating-point atomics, nothing between workgroups, no device allocation: the same call on
 * the same inputs writes the same bytes.  B = 0 succeeds without a launch; invalid scalar
 * arguments (Dx < 1, not 0 <= c0 < c1 <= Dx, Q < 1, B > 65535, phases) or a null pointer are
 * PTTS_EINVAL without a launch.
 * ------------------------------------------------------------------------------------- */
#define PTTS_ALIGN_EMPTY 1          /* T = 0 or N = 0 */
#define PTTS_ALIGN_TOO_LONG 2       /* N > ptts_align_max_states() */
#define PTTS_ALIGN_TOO_SHORT 4      /* T < N */
#define PTTS_ALIGN_NOT_FINITE 8     /* an emission or the score is not finite */
#define PTTS_ALIGN_BAD_OFFSETS 16   /* the offsets do not lie inside the totals, or the cells exceed `cells` */
#define PTTS_ALIGN_BAD_GAUSS 32     /* an index of gauss lies outside [0, Q) */
#define PTTS_ALIGN_PHASE_EMISSIONS 1  /* the layout and the emissions */
#define PTTS_ALIGN_PHASE_TIME_LOOP 2  /* the recurrence and the back-pointer bits */
#define PTTS_ALIGN_PHASE_BACKTRACK 4  /* the path: dur, state; the outputs of flagged utterances */
#define PTTS_ALIGN_PHASE_ALL 7
int ptts_align_max_states(void);
size_t ptts_align_workspace_bytes(long long cells, int B, long long t_total);
int ptts_align_viterbi_batch(const float* X, const long long* frame_off, long long t_total, int Dx, int c0, int c1,
                             const int* gauss, const long long* state_off, long long n_total, const double* mu, const double* w,
                             const double* g, int Q, int B, long long cells, int* dur, int* state /* or NULL */, double* score,
                             int* info, int phases, void* workspace, size_t workspace_bytes, void* stream);
size_t ptts_align_accumulate_workspace_bytes(long long n_total);
int ptts_align_accumulate(const float* X, const long long* frame_off, long long t_total, int Dx, int c0, int c1,
                          const int* gauss, const long long* state_off, long long n_total, const int* dur, const int* occ,
                          const long long* occ_off, int Q, int B, long long* count, double* s1, double* s2, void* workspace,
                          size_t workspace_bytes, void* stream);
int ptts_align_update(const long long* count, const double* s1, const double* s2, const double* floor, int Q, int D,
                      long long min_count, double* mu, double* w, double* g, int* kept, int* floored, void* stream);

/* ---------------------------------------------------------------------------------------
 * Waveform pre-processing (csrc/preproc.hip; the reference's Vocoder.preprocwav,
 * vocoders.py:45-63; both definitions are this build's own).  fp32 in
 * memory, fp64 arithmetic, one rounding per sample.  Both entry points take a packed batch:
 * utterance u is the samples off[u] .. off[u+1] of one array, the offsets [n_utts + 1] 64-bit
 * in DEVICE memory, the totals as the host measured them; an utterance whose offsets do not lie
 * inside the totals is skipped, nothing of it is read or written.  n_utts <= 65535.  No
 * atomics, nothing between workgroups, no device allocation; an utterance's result does not
 * depend on what else is in the launch.
 *
 * ptts_resample: up = fs_out / gcd, down = fs_in / gcd, up <= 1024; h [up][2 hw] fp64 is the
 *   CALLER's table (device memory, at most 4 MiB) of the Kaiser-windowed sinc, row p column
 *   j + hw - 1 = h(p / up - j), j = -hw + 1 .. hw.  Utterance u of N samples gives
 *   M = (N up + down - 1) div down samples (no more than y_off[u+1] - y_off[u] are written):
 *   y[m] = sum_j h[p][j] x[q + j], q = (m down) div up, p = (m down) mod up, x = 0 outside
 *   [0, N), summed in increasing j.  max_out: the longest output of the batch (the grid).  One
 *   thread per output sample.  n_utts = 0 or max_out = 0 succeeds without a launch.
 * ptts_highpass_zerophase: the order-4 Butterworth high-pass at fc (fs / 4000 <= fc < fs / 2) as
 *   two second-order sections, K = tan(pi fc / fs), Q = 1 / (2 cos(pi / 8)), 1 / (2 cos(3 pi / 8)),
 *   n = 1 / (1 + K / Q + K^2), b = (n, -2 n, n), a1 = 2 (K^2 - 1) n, a2 = (1 - K / Q + K^2) n
 *   (ptts_highpass_sections writes them as sos [2][6] = b0 b1 b2 1 a1 a2, on the host), run
 *   forward and backward over the signal with padlen samples of odd extension at both ends
 *   (every utterance longer than padlen, else it is skipped), each pass starting from the steady
 *   state of its first sample: scipy.signal.sosfiltfilt(sos, x, padtype='odd', padlen=padlen).
 *   y may not overlap x.  One workgroup per utterance walks it in tiles of
 *   ptts_highpass_tile()'s `tile` samples, a lane owning `chunk` consecutive ones; the signal
 *   between the passes is fp64 in the workspace, ptts_highpass_workspace_bytes(total, n_utts,
 *   padlen) = 8 (total + 2 padlen n_utts) bytes (0 for arguments out of range), 8-byte aligned; a
 *   shorter one is PTTS_EINVAL.  n_utts = 0 or total = 0 succeeds without a launch.
 * ------------------------------------------------------------------------------------- */
int ptts_resample(const float* x, const long long* x_off, long long total_in, float* y, const long long* y_off,
                  long long total_out, long long max_out, int n_utts, const double* h, size_t h_bytes, int up, int down, int hw,
                  void* stream);
int ptts_highpass_tile(int* chunk, int* tile);
int ptts_highpass_sections(double fs, double fc, double* sos);
size_t ptts_highpass_workspace_bytes(long long total, int n_utts, int padlen);
int ptts_highpass_zerophase(const float* x, float* y, const long long* off, long long total, int n_utts, double fs, double fc,
                            int padlen, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------
 * Label front end (external/merlin/label_normalisation.py: pattern_matching_binary,
 * pattern_matching_continous_position, load_labels_with_state_alignment :661-710,
 * load_labels_with_phone_alignment :546-568): HTS full-context labels -> frame-level context rows.
 *
 * ptts_labels_match: V [P, nQS + nCQS] fp32 and status [P] int32 from P labels (one per phone).
 *   labels     packed bytes [label_bytes], label_off [P+1] device int32 (clamped into the buffer);
 *              max_label_len is the longest label as the host measured it: above
 *              PTTS_LABELS_MAX_LABEL the call fails with PTTS_EINVAL before anything is launched.
 *   patterns   pat_bytes [n_pat_bytes]; per pattern pat_off and pat_meta = length (low 16 bits)
 *              | PTTS_LABELS_ANCHOR_START | PTTS_LABELS_ANCHOR_END | PTTS_LABELS_WILD (the pattern
 *              holds '*' = any run of characters or '?' = one character).  A pattern is an HTK
 *              question with its outer '*' stripped; without an anchor it may match anywhere.
 *   QS         qs_first [nQS+1]: question q owns patterns qs_first[q] .. qs_first[q+1]-1; its
 *              column is 1.0 when one of them matches, else 0.0.
 *   CQS        cqs [nCQS][3] = {prefix pattern, suffix pattern, PTTS_LABELS_CAPTURE_*} (neither
 *              pattern may hold '*'): leftmost prefix match, longest run of digits (and '.' for
 *              _DECIMAL) behind it after which the suffix matches; the column is the captured
 *              decimal -- integer mantissa / power of ten in fp64, rounded to fp32 -- or -1.0.
 *   status[p]  0, or ((CQS index + 1) << 2) | PTTS_LABELS_ERR_* of the first CQS of label p whose
 *              capture is not a number of at most 15 digits with at most one '.'.
 * All tables are device memory; every index read from them is clamped.  No atomics, no workspace.
 *
 * ptts_labels_expand: X [T, Q + F] fp32 from V [P, Q] and seg [S][8] device int32 (16-byte
 * aligned, as X): {phone row, first output row, frame_number, state_index, state_index_backward,
 * phone_duration, state_duration_base, 0} per HMM state or phone, first rows ascending, T the end
 * of the last.  Row r of segment s copies V[phone] and appends, with i = r - first row (ratios
 * divided in fp64, rounded once to fp32):
 *   PTTS_LABELS_FULL (F = 9)   (i+1)/fn, (fn-i)/fn, fn, state_index, state_index_backward, pd,
 *                              fn/pd, (pd-i-base)/pd, (base+i+1)/pd
 *   _MINIMAL_FRAME (2)         (i+1)/fn, state_index        _STATE_ONLY (1)  state_index
 *   _MINIMAL_PHONEME (3)       (i+1)/fn, (fn-i)/fn, fn      _NONE (0)
 *   _COARSE_CODING (4)         cc[0][300+k], cc[1][200+k], cc[2][100+k], pd with
 *                              k = int((200/pd)*(base+i)); cc_table [3][PTTS_LABELS_CC_POINTS] fp32
 *
 * ptts_labels_segments: the segment table of ptts_labels_expand from durations instead of a label
 * file's times.  dur [P][D] device fp32, D = PTTS_LABELS_SEG_STATES (state durations) or 1 (phone
 * durations), in frames; unit_off [U+1] device int32: utterance u owns phones unit_off[u] ..
 * unit_off[u+1]-1 (ascending from 0 to P; clamped into that range).  Per duration n = rint(d), ties
 * to even; NaN and n < min_frames become min_frames; n > max_frames becomes max_frames and sets
 * PTTS_LABELS_SEG_CLAMPED in status[u] (status [U] device int32, 0 otherwise).  seg [P*D][8]
 * (16-byte aligned) row p*D+k = {p, first output row, n, k+1, D-k, sum_k n, sum_{j<k} n, 0}, for
 * D = 1 {p, first output row, n, 0, 0, n, 0, 0}; first rows run on across the utterances of the call.
 * rows [U+1] device int32: the first row of every utterance, rows[U] = T, the rows ptts_labels_expand
 * will write.  0 <= min_frames <= max_frames <= PTTS_LABELS_SEG_MAX_FRAMES, and P*D*max_frames has
 * to stay below 2^31 (PTTS_EINVAL otherwise: no total can then reach 2^31 rows).  P = 0 is allowed
 * (dur and seg may be null): rows and status come back as zeros.  No atomics, no workspace; the
 * output does not depend on the launch geometry.
 * ------------------------------------------------------------------------------------- */
#define PTTS_LABELS_MAX_LABEL       1024
#define PTTS_LABELS_CC_POINTS       600
#define PTTS_LABELS_ANCHOR_START    0x10000
#define PTTS_LABELS_ANCHOR_END      0x20000
#define PTTS_LABELS_WILD            0x40000
#define PTTS_LABELS_CAPTURE_DIGITS  0
#define PTTS_LABELS_CAPTURE_DECIMAL 1
#define PTTS_LABELS_ERR_DIGITS      1
#define PTTS_LABELS_ERR_FORMAT      2
#define PTTS_LABELS_FULL            0
#define PTTS_LABELS_MINIMAL_FRAME   1
#define PTTS_LABELS_STATE_ONLY      2
#define PTTS_LABELS_NONE            3
#define PTTS_LABELS_MINIMAL_PHONEME 4
#define PTTS_LABELS_COARSE_CODING   5
#define PTTS_LABELS_SEG_STATES      5
#define PTTS_LABELS_SEG_CLAMPED     1
#define PTTS_LABELS_SEG_MAX_FRAMES  16777216
int ptts_labels_feature_count(int mode);
int ptts_labels_match(const unsigned char* labels, const int* label_off, int P, int label_bytes, int max_label_len,
                      const unsigned char* pat_bytes, int n_pat_bytes, const int* pat_off, const int* pat_meta, int NP,
                      const int* qs_first, int nQS, const int* cqs, int nCQS, float* V, int* status, void* stream);
int ptts_labels_expand(const float* V, const int* seg, const float* cc_table, float* X, int P, int Q, int S, int T,
                       int mode, void* stream);
int ptts_labels_segments(const float* dur, const int* unit_off, int P, int D, int U, int min_frames, int max_frames, int* seg,
                         int* rows, int* status, void* stream);

/* ---------------------------------------------------------------------------------------
 * Random numbers: Philox4x32-10 (Salmon et al., SC'11; the Random123 constants), counter-based.
 * Every number is a pure function of (seed, call counter, index); nothing is stored per thread
 * and no mask is kept.  Philox counter = (index lo, index hi, call lo, call hi), key = (seed
 * lo, seed hi).
 * state: a caller-owned DEVICE block of two 64-bit words {seed, call counter}, one per device.
 * A forward entry point reads it in its main kernel, which leaves the call counter it used in the
 * caller's 8-byte device word `used`, then enqueues a one-thread kernel on the same stream that
 * adds one to the counter: replays of a captured graph draw fresh numbers, and the backward pass
 * of a replay (which reads `used`, not the live counter) sees its own forward's mask.  Calls that
 * share a block are ordered by the stream they are launched on.
 * ------------------------------------------------------------------------------------- */
int ptts_rng_seed(unsigned long long* state, unsigned long long seed, unsigned long long counter, void* stream);
/* out_host[0] = seed, out_host[1] = call counter; synchronises the stream */
int ptts_rng_state_get(const unsigned long long* state, unsigned long long* out_host, void* stream);
/* Dropout with Keras noise_shape = (batch, 1, None) (networktts.py:65-70): one mask per sample and
 * column, shared along time.   y[b,t,d] = a[b,t,d] * m[b0+b,d] / (1 - rate),
 *   a = x (PTTS_IN_NONE) or lrelu(scale[d]*x + shift[d]) (PTTS_IN_LRELU; scale/shift both or NULL),
 *   m = 1 where float(w >> 8) * 2^-24 < 1 - rate (fp32), w = word d & 3 of the Philox block of
 *   index (b0 + b) * ceil(D/4) + (d >> 2).
 * b0: global index of the first sample (a batch sharded over ranks draws the masks of the whole
 * batch).  One pass: 16-byte accesses where D % 4 == 0 and x, y are 16-byte aligned, scalar ones
 * otherwise; the masks of a workgroup's column groups are drawn once and reused down the rows. */
int ptts_dropout_fwd(const float* x /*[B,T,D]*/, const float* scale, const float* shift, float* y,
                     unsigned long long* state, unsigned long long* used, float rate /*[0,1)*/, float alpha,
                     int mode, int B, int T, int D, long long b0, void* stream);
/* da = dy * m / (1 - rate), the mask regenerated from `used` (and the block's seed); in place
 * allowed.  The gradient through a fused input activation is ptts_affine_act_bwd on da. */
int ptts_dropout_bwd(const float* dy, float* da, const unsigned long long* used, const unsigned long long* state,
                     float rate, int B, int T, int D, long long b0, void* stream);
/* out[i] = element i0 + i of the call's N(0, stddev^2) sequence, i < n (i0: a rank's offset into
 * the whole batch's noise).  Box-Muller, four values per Philox block e >> 2 of element e: for the
 * word pairs (0,1) and (2,3), r = stddev * sqrt(-2 ln u1), u1 = ((w >> 8) + 1) * 2^-24 in (0, 1],
 * values r cos(2 pi u2), r sin(2 pi u2), u2 = (w' >> 8) * 2^-24. */
int ptts_normal_fill(float* out, unsigned long long* state, unsigned long long* used, float stddev /*>= 0*/,
                     long long i0, long long n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PERCIVAL_HIP_H */
