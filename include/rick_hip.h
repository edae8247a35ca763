/* rick_hip.h — C ABI of librick_hip.so: the MI355X (gfx950) kernels behind the RICK
 * StyleGAN2 train-step hot path.
 *
 * Conventions (all entry points):
 *   - plain device pointers + explicit sizes; no framework types; fp32 tensors unless said;
 *   - launched asynchronously on `stream` (a hipStream_t passed as void*), never
 *     synchronises, never allocates; workspaces are caller-provided;
 *   - returns 0 on success, RICK_EINVAL for bad arguments, or 1000 + hipError_t from
 *     hipGetLastError() after the launch (the reference's extensions raise through
 *     TORCH_CHECK -> RuntimeError, op/upfirdn2d.cpp:8,15-16; the Python binding in
 *     rick_amd/_lib.py turns a non-zero status into RuntimeError);
 *   - re-entrant, no global mutable state (the reference ops are called from
 *     DataParallel worker threads, train_dynamic_update_prune.py:941-944).
 *
 * Activation layout: 4-D activations are channels-last ("NHWC": [N, H, W, C] in memory);
 * this is the reference extension's own [major, H, W, minor] view
 * (op/upfirdn2d_kernel.cu:209-240) with major = N, minor = C.  RGB-side tensors (3 channels)
 * stay planar ([N, 3, H, W], i.e. major = N*3, minor = 1).
 */
#ifndef RICK_HIP_H
#define RICK_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RICK_EINVAL 22
#define RICK_MAX_TAPS 16

int rick_abi_version(void);

/* ---------------------------------------------------------------------------------------
 * upfirdn2d — replaces upfirdn2d_op.upfirdn2d(input[M,H,W,minor], kernel, up_x, up_y,
 * down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1) (op/upfirdn2d.cpp:12-19,
 * op/upfirdn2d_kernel.cu:209-369).  out is [major, out_h, out_w, minor] with
 * out_h = (in_h*up_y + pad_y0 + pad_y1 - kh)/down_y + 1 (kernel.cu:237-240); the caller
 * allocates it.  Forward, backward (flipped kernel, up<->down, op/upfirdn2d.py:19-60) and
 * double-backward are the same entry with different parameters.  Tap order and fmaf
 * accumulation match oracle/csrc/oracle_ops.c bit for bit. */
int rick_upfirdn2d_f32(const float *input, const float *kernel, float *out,
                       int64_t major, int in_h, int in_w, int minor, int kh, int kw,
                       int up_x, int up_y, int down_x, int down_y,
                       int pad_x0, int pad_x1, int pad_y0, int pad_y1, void *stream);
/* Layouts: minor == 1 (planar [major, H, W]; 4-byte accesses only, any float alignment) or channels-last with minor in
 * {4, 8, ..., 64} or minor % 64 == 0; anything else is RICK_EINVAL.  Every channels-last kernel makes 16-byte accesses: `input`,
 * `out`, and with rick_upfirdn2d_ex_f32 `chan_scale` and the split image, must be 16-byte aligned there, RICK_EINVAL otherwise
 * (channels-last needs major <= 65535; planar takes any major, in slabs of 65535 planes).
 * The form a call takes — host only, nothing is launched: out12 = {kernel (RICK_UFD_*), output tile h, w, staged input window
 * h, w, LDS bytes per block, grid x, y, z, launches (> 1: the planar slab loop; grid y is then the first slab's), out_h, out_w}.
 * has_tail / has_ex: a fused tail / the extended result handling is asked for; aligned16: the pointers named above are
 * 16-byte aligned.  Returns what the launch would return for the geometry (RICK_EINVAL: no kernel takes it). */
#define RICK_UFD_K4_T8 0      /* 4x4 taps, up 1, down 1: 8 x 8 outputs x 64 channels per block */
#define RICK_UFD_K4_T16 1     /* the same on 16 x 16 outputs x 32 channels (RICK_TUNE_UFD_TILE16) */
#define RICK_UFD_K4_D2 2      /* 4x4 taps, up 1, down 2: 4 x 8 outputs x 64 channels */
#define RICK_UFD_NHWC 3       /* generic channels-last: the largest tile whose staged window fits 60 KB of LDS */
#define RICK_UFD_PLANAR 4     /* generic planar */
int rick_upfirdn2d_plan(int64_t major, int in_h, int in_w, int minor, int kh, int kw, int up_x, int up_y, int down_x, int down_y,
                        int pad_x0, int pad_x1, int pad_y0, int pad_y1, int has_tail, int has_ex, int aligned16, int *out12);

/* The same operator in the reference's other dtypes (op/upfirdn2d_kernel.cu:311-367 dispatches half / float / double):
 * dtype 1 = float64, 2 = float16 (fp32 accumulation); planar [major, H, W] layout (minor == 1), kernel taps in the same
 * dtype.  Correctness-first (one thread per output): for `.double()` gradcheck and `.half()` inference of drop-in users. */
int rick_upfirdn2d_any(const void *input, const void *kernel, void *out, int dtype, int64_t major, int in_h, int in_w,
                       int kh, int kw, int up_x, int up_y, int down_x, int down_y, int pad_x0, int pad_x1, int pad_y0,
                       int pad_y1, void *stream);

/* ---------------------------------------------------------------------------------------
 * fused bias + activation — replaces fused.fused_bias_act(input, bias, refer, act, grad,
 * alpha, scale) (op/fused_bias_act.cpp:11-21, op/fused_bias_act_kernel.cu:18-99):
 *   v = x[i] + (bias ? bias[(i / step_b) % size_b] : 0)
 *         + (noise ? nw[0] * noise[((i / n_div) % noise_nb) * noise_hw + (i / hw_div) % noise_hw] : 0)
 *   act*10+grad: 30: v>0 ? v : v*alpha   31: ref>0 ? v : v*alpha   10/11: v   12/32: 0
 *   out[i] = y * scale
 * NULL bias / ref / noise mean "absent" (the reference passes empty tensors).  The noise
 * term is this build's fusion of NoiseInjection (model_probe_tune.py:293-298) into the same
 * pass; nw is a device pointer to the scalar noise strength. */
int rick_bias_act_f32(const float *x, const float *bias, const float *ref, float *out,
                      int64_t n, int64_t step_b, int64_t size_b, int act, int grad,
                      float alpha, float scale,
                      const float *noise, const float *nw, int64_t n_div, int64_t hw_div,
                      int64_t noise_nb, int64_t noise_hw, void *stream);

/* Backward of the fused activation for a [rows, C] (channels-last) tensor in ONE pass:
 *   gx[r,c] = scale * g[r,c] * (ref[r,c] > 0 ? 1 : alpha)          (fused_act.py:28-30)
 *   gb[c]   = sum_r gx[r,c]                                          (fused_act.py:32-37)
 *   gnw     = sum_{r,c} gx[r,c] * noise[(r / rows_per_img % noise_nb)*noise_hw + r % noise_hw]
 * The per-channel / scalar sums use wavefront shuffles + a deterministic two-stage
 * reduction through `partials` (float[(C + 1) * rick_bias_act_bwd_blocks(rows, C)]).
 * gb / gnw / noise may be NULL.  accumulate != 0: the second stage ADDS the sums into gb / gnw (the caller passes
 * the parameters' gradient buffers: no temporary, no separate accumulation pass); one second-stage launch serves both. */
/* rick_bias_act_f32 without the noise term in dtype 1 = float64 / 2 = float16 (op/fused_bias_act_kernel.cu:79). */
int rick_bias_act_any(const void *x, const void *bias, const void *ref, void *out, int dtype, int64_t n, int64_t step_b,
                      int64_t size_b, int act, int grad, float alpha, float scale, void *stream);
int rick_bias_act_bwd_blocks(int64_t rows, int C);
int rick_bias_act_bwd_f32(const float *g, const float *ref, float *gx, float *gb, float *gnw,
                          const float *noise, int64_t rows, int C, int64_t rows_per_img,
                          int64_t noise_nb, int64_t noise_hw, float alpha, float scale,
                          float *partials, int accumulate, void *stream);
/* ... and, from the same pass, the demodulation gradient of the modulated convolution the activation follows
 * (model_probe_tune.py:246-252: y = act(d * conv(..) + noise + bias)):  gd[n, c] = (sum over the image's rows of gx * t) / divisor[n, c],
 * t = the convolution's output reconstructed from `ref` (ref / scale for ref > 0, ref / (scale * alpha) otherwise, minus
 * noise_w * noise and bias).  Needs rick_bias_act_bwd_dot_ok(): C % 4 == 0 and blocks that never straddle an image.
 * dpartials: rick_bias_act_bwd_blocks() * C floats.  (round 5: replaces a second read of gx and ref, rick_hw_dot_act_f32) */
int rick_bias_act_bwd_dot_ok(int64_t rows, int C, int64_t rows_per_img);
int rick_bias_act_bwd_dot_f32(const float *g, const float *ref, float *gx, float *gb, float *gnw, const float *noise,
                              int64_t rows, int C, int64_t rows_per_img, int64_t noise_nb, int64_t noise_hw, float alpha,
                              float scale, float *partials, int accumulate, const float *bias, const float *noise_w,
                              const float *divisor, float *gd, float *dpartials, void *stream);

/* ---------------------------------------------------------------------------------------
 * Convolution family (replaces the F.conv2d / F.conv_transpose2d calls of
 * model_probe_tune.py:122,265,274,280 and their autograd).  One implicit-GEMM MFMA kernel,
 * parameterised by a tap table, covers 3x3/1x1, stride 1/2, transposed stride 2, and the
 * data-gradient of each.  fp32 in HBM; on the way into LDS an operand is multiplied by a
 * power of two (chosen per block from a sample of the block's own data, per packed tensor for
 * the weights) and split into fp16 hi + fp16 lo; the products hi*hi + hi*lo + lo*hi run on
 * v_mfma_f32_16x16x32_f16 with fp32 accumulation (split = 2: 2^-22 relative per product) or
 * hi*hi only (split = 1); the exponents are removed again in the epilogue (exact).
 *
 * Geometry: activations NHWC.  The launch covers a grid of GH x GW "positions" per image;
 * position (gy, gx) writes output pixel (gy*os + oy0, gx*os + ox0) of [N, OH, OW, Co] and
 * tap t reads input pixel (gy*is + dy[t], gx*is + dx[t]) of [N, IH, IW, Ci] (zero outside)
 * with packed weight slice wt[t]:
 *   out[n, pix, co] = alpha * oscale[n, co] * sum_t sum_ci W[wt[t]][co][ci] *
 *                     (iscale[n, ci] * x[n, inpix(t), ci])
 * oscale / iscale (NULL = 1) carry StyleGAN2's demodulation / modulation
 * (model_probe_tune.py:246-251) without materialising per-sample weights. */
typedef struct {
    int N, IH, IW, Ci;      /* input  [N, IH, IW, Ci] */
    int OH, OW, Co;         /* output [N, OH, OW, Co] */
    int GH, GW;             /* positions per image */
    int is, os, oy0, ox0;   /* input stride, output stride / offset */
    int ntaps;              /* taps used by this launch */
    int nslices;            /* tap slices in the packed weight / in gw (wt[t] < nslices) */
    int dy[RICK_MAX_TAPS], dx[RICK_MAX_TAPS], wt[RICK_MAX_TAPS];
    int split;              /* 1 = fp16, 2 = fp16x3 (fp32-grade) */
    float alpha;
} rick_conv_geom;

/* Packed-weight buffer size in bytes for `nslices` tap slices of a [Co, Ci] matrix (tiles + a 64-byte
 * trailer that holds the tensor's pack exponent). */
int64_t rick_conv_packed_bytes(int Co, int Ci, int nslices);
/* Pack W (element (co, ci, slice s) at w[co*s_co + ci*s_ci + s*s_t]) * scale into the MFMA
 * A-operand LDS image (fp16 hi/lo of W * scale * 2^e, swizzled, zero padded to 128 x 32 tiles; e from a
 * device-side sample of the tensor, stored in the trailer).  Two launches, no host synchronisation. */
int rick_conv_pack_weight(const float *w, int64_t s_co, int64_t s_ci, int64_t s_t,
                          int Co, int Ci, int nslices, float scale, int split, void *packed, void *stream);
/* The same packing for MANY weights in one launch (every convolution of a network after an optimiser step;
 * replaces one launch per layer and orientation).  `descs_device` is an array of n descriptors in DEVICE
 * memory; descriptor d owns blocks [blk_begin[d], blk_begin[d] + rick_conv_pack_blocks(Co, Ci)), in order;
 * total_blocks = the sum.  `w` need not be a whole tensor: any (s_co, s_ci, s_t) view, e.g. the transposed
 * view the data gradient uses.
 * PAIRS: two descriptors that are the mutually transposed views of one storage (Co/Ci and s_co/s_ci swapped, same w, s_t,
 * nslices) may name each other in `partner` (index + 1, 0 = none).  Where one of the two is a row view (s_t == 1,
 * s_ci == nslices) and nslices <= 9, a launch that covers BOTH entries (both indices < n, < 1024) reads the source once and
 * writes both images from one pass; the two then need no blocks of their own (an empty block range is allowed, and blocks they
 * do own stay idle).  A launch with a smaller n — one captured before the partner was appended — packs the entry through its
 * own blocks as before, so an entry that such a launch covers must keep them.  total_blocks may be 0. */
typedef struct {
    const float *w;
    int64_t s_co, s_ci, s_t;
    void *packed;           /* rick_conv_packed_bytes(Co, Ci, nslices) bytes */
    int Co, Ci, nslices;
    float scale;
    int blk_begin;
    int partner;            /* index + 1 of the transposed view's descriptor, 0 = none */
} rick_pack_desc;
int rick_conv_pack_blocks(int Co, int Ci);
int rick_conv_pack_weights_multi(const rick_pack_desc *descs_device, int n, int total_blocks, int split, void *stream);
/* Launches with too few output tiles to fill the chip (the 4x4..32x32 512-channel layers) are
 * split over the channel-chunk dimension; partial sums go through `workspace`
 * (rick_conv_igemm_workspace_bytes bytes, 0 = not needed, may then be NULL) and a deterministic
 * second-stage kernel applies alpha / oscale. */
int64_t rick_conv_igemm_workspace_bytes(const rick_conv_geom *g);
/* Optional tail fused into the convolution's epilogue — replaces a separate rick_bias_act_f32 pass (one read and
 * one write of the whole activation) after EqualConv2d + FusedLeakyReLU (model_probe_tune.py:595-641) and after the
 * non-upsampling StyledConv (conv -> NoiseInjection -> FusedLeakyReLU, :314-348):
 *   out = gain * lrelu_slope(conv + bias[co] + noise_w[0] * noise[n % noise_nb][oy][ox])
 * in exactly that operation order (bit-identical to the two-pass form).  Needs Co % 4 == 0. */
typedef struct {
    const float *bias;      /* [Co] or NULL */
    const float *noise;     /* [noise_nb][OH*OW] or NULL */
    const float *noise_w;   /* device scalar, required with noise */
    int noise_nb;           /* 1 (shared map) or N */
    int act;                /* 0: none, 1: LeakyReLU(slope) * gain */
    float slope, gain;
    float *amax;            /* NULL, or an amax word: max |out| is folded into it (the exact bound the producer of the next
                             * split image needs; see "Split images" below) */
    /* also write out * split_scale[n, co] as a split image (the next modulated convolution's operand: its style scale
     * folded in; split_scale may be NULL), bounded by split_coef * (*split_bound) * ... — the caller's bound covers the scale.
     * Launches without split-K only (rick_conv_igemm_workspace_bytes(g) == 0). */
    void *split_out;
    float *split_hdr;
    const float *split_bound;   /* amax word */
    float split_coef;
    const float *split_scale;   /* [N, Co] or NULL */
} rick_conv_epilogue;
int rick_conv_igemm_f32(const float *x, const void *packed_w, float *out,
                        const float *iscale, const float *oscale,
                        const rick_conv_geom *g, void *workspace, void *stream);
/* rick_upfirdn2d_f32 with the same tail fused after the FIR (the blur that follows every upsampling StyledConv,
 * model_probe_tune.py:263-268,344-348): channels-last 4x4 taps, up = 1, minor % 64 == 0 only (else non-zero).  The FIR takes the
 * tail's bias / noise / activation fields; its amax / split_out fields must be NULL (RICK_EINVAL otherwise): the FIR's own result
 * handling is rick_split_out (rick_upfirdn2d_ex_f32). */
int rick_upfirdn2d_act_f32(const float *input, const float *kernel, float *out,
                           int64_t major, int in_h, int in_w, int minor, int kh, int kw,
                           int up_x, int up_y, int down_x, int down_y,
                           int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                           const rick_conv_epilogue *tail, void *stream);
/* rick_conv_igemm_f32 with the fused tail (epilogue may be NULL). */
int rick_conv_igemm_act_f32(const float *x, const void *packed_w, float *out, const float *iscale, const float *oscale,
                            const rick_conv_geom *g, const rick_conv_epilogue *epilogue, void *workspace, void *stream);

/* Several geometries over the same tensors and weights (the 4 output-parity classes of a stride-2
 * transposed convolution) in one launch.  ngeom <= 4; all share Ci, Co, split. */
int64_t rick_conv_igemm_multi_workspace_bytes(const rick_conv_geom *geoms, int ngeom);
int rick_conv_igemm_multi_f32(const float *x, const void *packed_w, float *out,
                              const float *iscale, const float *oscale,
                              const rick_conv_geom *geoms, int ngeom, void *workspace, void *stream);

/* Transposed 3x3 stride-2 convolution, padding 0 — F.conv_transpose2d(stride=2) of the upsampling StyledConvs
 * (model_probe_tune.py:257-268) and the data gradient of the discriminator's stride-2 3x3 convolutions (:608-630):
 *   out[n, 2*iy+ky, 2*ix+kx, co] = alpha * oscale[n,co] * sum W[ky*3+kx][co][ci] * (iscale[n,ci] * x[n, iy, ix, ci])
 * All four output-parity classes come from ONE staged input patch per block (the generic multi-class launch above
 * stages it once per class).  packed_w = rick_conv_pack_weight(..., nslices = 9); out is [N, OH, OW, Co] with
 * OH in {2*IH, 2*IH+1} (likewise OW; the smaller size crops the last row / column); Ci % 4 == Co % 4 == 0.
 * Short grids are split over channel chunks through `workspace` (rick_convt2_workspace_bytes, 0 = not needed). */
int64_t rick_convt2_workspace_bytes(int N, int IH, int IW, int Ci, int Co, int OH, int OW);
int rick_convt2_f32(const float *x, const void *packed_w, float *out, const float *iscale, const float *oscale,
                    int N, int IH, int IW, int Ci, int Co, int OH, int OW, int split, float alpha,
                    void *workspace, void *stream);
/* The tile / split plan the launch above will use: out8 = {TW, TH, NB, tiles, nsplit, chunks per split, nfull, subq}:
 * tiles x nsplit work items; the first nfull run as one block each, every later one as subq blocks with 8 / subq of the
 * tile's fragment columns (the last, partly filled round of 256 blocks). */
int rick_convt2_plan(int N, int IH, int IW, int Ci, int Co, int OH, int OW, int *out8);
/* The plan's lane-slot -> tile-position table (128 entries, bit 7 = unused slot) and its patch-window pitch in pixels:
 * the permutation that makes the kernel's LDS reads bank-conflict-free (tools/lds_sim.py checks it). */
int rick_convt2_posmap(int N, int IH, int IW, int Ci, int Co, int OH, int OW, unsigned char *out128, int *pitch);

/* Weight gradient for the same geometry:
 *   gw[(co, ci, t)] = alpha * sum_{n, pos} (ascale[n,co] * gy[n, outpix(pos), co]) *
 *                                           (bscale[n,ci] * x[n, inpix(pos, t), ci])
 * written to gw[co*s_co + ci*s_ci + wt[t]*s_t].  Split-K over position tiles with a
 * deterministic second-stage reduction through `workspace`
 * (rick_conv_wgrad_workspace_bytes bytes).  `accumulate` != 0 adds into gw. */
int64_t rick_conv_wgrad_workspace_bytes(const rick_conv_geom *g);
int rick_conv_wgrad_f32(const float *x, const float *gy, float *gw,
                        int64_t s_co, int64_t s_ci, int64_t s_t,
                        const float *ascale, const float *bscale,
                        const rick_conv_geom *g, int accumulate, void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Split images — activations / gradients stored pre-split for the MFMA kernels (no counterpart in the reference: its
 * convolutions are cuDNN's, model_probe_tune.py:122,265,274,280; this is how the fp16x3 arithmetic of this build avoids
 * converting the same fp32 operand once per co-tile block, again in dgrad and again in wgrad).
 * A split image of an NHWC fp32 tensor [npix, C] (C % 4 == 0) has the same byte size and addressing; the 16 bytes of
 * channels c .. c+3 hold {hi x 4 | lo x 4} as fp16, hi = fp16(v * 2^e), lo = fp16(v * 2^e - hi), with ONE
 * exponent per tensor in a 16-byte device header {2^e, 2^-e, bound, 0}.  The exponent comes from a guaranteed bound
 * coef * (*amax0 + *amax1) on |v| (amax1 may be NULL), placed in [2^13, 2^14): nothing can saturate, and values down to
 * 2^-10 of the bound keep 2^-22 relative precision.  A RUNNING MAXIMUM ("amax word": every `amax`, `amax0`, `bound0` ...
 * pointer below) is RICK_AMAX_FLOATS floats: RICK_AMAX_SLOTS slots, one per 128-byte line, the value being the maximum over
 * the slots (thousands of blocks folding into one address serialise in the L2).  Callers zero the word; rick_amax_f32 folds
 * max |x| into it with atomic max, the kernels that produce activations do the same in their epilogues. */
#define RICK_AMAX_SLOTS 16
#define RICK_AMAX_FLOATS (16 * 32)
int rick_amax_f32(const float *x, int64_t n, float *amax_word, void *stream);
/* Identity of the hipGraph capture `stream` is recording into (hipStreamGetCaptureInfo's id), 0 when it is not capturing.
 * Running maxima and headers a CAPTURED launch accumulates into must be zeroed by a fill inside the SAME graph: the host side
 * (rick_amd/op/split.py) starts a fresh block of words whenever this value changes. */
int rick_stream_capture_id(void *stream, unsigned long long *id);
/* What a producer kernel does with its result besides (or instead of) the fp32 store. */
typedef struct {
    void *split_out;        /* also write the result as a split image (NULL: no) */
    float *split_hdr;       /* its 16-byte header, published by the launch */
    const float *bound0;    /* |result| <= bound_coef * (*bound0 + *bound1); bound1 may be NULL */
    const float *bound1;
    float bound_coef;
    float *amax;            /* NULL, or: fold max |result| (after accumulation) into this word */
    int accumulate;         /* add the result to what the fp32 output holds (a second gradient arriving at a branch point) */
    int no_f32;             /* do not write the fp32 result (the output pointer may be NULL) */
    const float *chan_scale;/* NULL, or [N, C]: the split image holds result * chan_scale[n, c] (a modulated convolution's
                             * style / demodulation scale folded in; the bound must cover it) */
    /* activation adjoint fused behind the FIR (4x4 up = 1 form only): result <- result * (adj_ref > 0 ? 1 : adj_slope) * adj_gain
     * with adj_ref the activation's saved OUTPUT (same shape as the result), and the per-channel sums of that (the bias
     * gradient) reduced per block into adj_partials [blocks per channel slab = images * tiles][C]
     * (rick_upfirdn2d_adjoint_rows() rows; the caller column-sums them: rick_colsum_f32). */
    const float *adj_ref;
    float adj_slope, adj_gain;
    float *adj_partials;
} rick_split_out;
/* Saturation events since the last reset, host-synchronous: values that exceeded a split-image producer's bound (a caller's
 * mistake) and waves of the igemm / convt2 / wgrad kernels that clamped an fp32 -> fp16 conversion of an on-the-fly split
 * (an operand ~8 000 x above the sampled block maximum: the hardware's sticky OVERFLOW status, read once per wave).  Every
 * event means a finite but wrong product somewhere: 0 in every test and in tools/stability.py. */
int rick_saturation_count(unsigned *count, int reset);
/* Kernel-form switches (process-wide, host side; every form computes the same convolution — the eight-wave igemm is
 * bit-identical to the four-wave one on split images and differs by per-block operand exponents, 2^-22, on fp32 operands).
 * Used by the parity tests and the same-process A/B micro-benchmarks; returns the previous value, -1 for an unknown key.
 *   RICK_TUNE_IGEMM_W8: 3x3 stride-1 launches with >= RICK_TUNE_IGEMM_W8_MINBLK (default 192) blocks of 128 co x 256
 *   positions run the eight-wave form (conv.hip, igemm_body NW = 8) — 0 (default): never (four-wave 128 x 128 blocks: equal or
 *   faster end to end, conv.hip igemm_w8_plan); 1: fp32 operands with Ci >= 512; 2: wherever the form exists.
 *   RICK_TUNE_SPLITK_FUSED (default 0: measured 8 - 17 us per launch SLOWER than the second-stage launch, conv.hip): 1 = igemm
 *   split-K launches sum their partial tiles inside the launch — the block that arrives last for an output tile (one atomic
 *   ticket per tile) adds the partials in split order, exactly the sums of igemm_splitk_reduce_kernel. */
#define RICK_TUNE_IGEMM_W8 0
#define RICK_TUNE_IGEMM_W8_MINBLK 1
#define RICK_TUNE_SPLITK_FUSED 2
#define RICK_TUNE_IGEMM_S2W8 4      /* (default 2) 3x3 stride-2 launches with Co % 256 == 0 and >= RICK_TUNE_IGEMM_W8_MINBLK blocks: eight-wave 256 co x 128
                                     * position blocks (conv.hip, igemm_body WDMA = 5: +8 ... +16 % per launch, +1.05 % end to end); 1: Ci >= 256 only; 0: four-wave */
#define RICK_TUNE_UFD_TILE16 3      /* (default 0: measured 0.5 % slower end to end) 1 = 4x4 FIR, up = down = 1, outputs >= 32 x 32: 16 x 16 tiles on 32-channel slabs instead of 8 x 8 x 64 */
int rick_conv_tuning(int key, int value);
/* Producers.  rick_upfirdn2d_f32 / rick_upfirdn2d_act_f32 (tail may be NULL) with the extended result handling, channels-last
 * only; `out` may be NULL with ex->no_f32.  The activation adjoint (rick_bias_act_bwd_f32) leaving as split images:
 * out1 = g * (ref > 0 ? 1 : alpha) * scale and, when out2 != NULL, out2 = g * mul2 (the same gradient entering a parallel linear
 * branch), both bounded through *amax_g >= max |g|; any C % 4 == 0 with 16-byte aligned g / ref / images (the layout of
 * rick_split_pack_f32 — the consumers check their own C % 32), RICK_EINVAL otherwise.  The ResBlock merge y = (a + b) * alpha (rick_add_scale_f32) written as
 * fp32 and as a split image. */
int rick_upfirdn2d_ex_f32(const float *input, const float *kernel, float *out,
                          int64_t major, int in_h, int in_w, int minor, int kh, int kw,
                          int up_x, int up_y, int down_x, int down_y,
                          int pad_x0, int pad_x1, int pad_y0, int pad_y1,
                          const rick_conv_epilogue *tail, const rick_split_out *ex, void *stream);
/* rows of adj_partials for an output of out_h x out_w pixels and `major` images (4x4 up = 1 down = 1 form: 8 x 8 tiles) */
int64_t rick_upfirdn2d_adjoint_rows(int64_t major, int out_h, int out_w);
/* out[c] (+)= sum_r partials[r * stride + c], c < ncols: the deterministic second stage of the per-block channel sums */
int rick_colsum_f32(const float *partials, float *out, int64_t rows, int stride, int ncols, int accumulate, void *stream);
/* Up to any number of such column sums in one launch per 32 items (bit-identical to rick_colsum_f32 item by item): out[c] (c < split,
 * or all columns when out2 is NULL) / out2[c - split] = (accumulate ? old : 0) + sum_r partials[r * stride + col0 + c], r < nb.
 * `items` is a HOST array: it travels in the kernel arguments, so the call may be captured into a hipGraph.  Used for the second
 * stages of the bias / noise-strength gradients of a whole backward pass (rick_bias_act_bwd_f32 with accumulate bit 1 set leaves
 * its partial rows [blocks][C + 1] unsummed: column C is the noise-strength term). */
#define RICK_COLSUM_MAX 32
typedef struct rick_colsum_item {
    const float *partials;
    float *out, *out2;
    int nb, stride, ncols, col0, split, accumulate;
} rick_colsum_item;
int rick_colsum_multi_f32(const rick_colsum_item *items, int n, void *stream);
int rick_bias_act_bwd_split_f32(const float *g, const float *ref, void *out1, float *hdr1, void *out2, float *hdr2,
                                float mul2, const float *amax_g, float *gb, float *gnw, const float *noise,
                                int64_t rows, int C, int64_t rows_per_img, int64_t noise_nb, int64_t noise_hw,
                                float alpha, float scale, float *partials, int accumulate, void *stream);
/* The discriminator's input layer (model_probe_tune.py:679: 1x1 conv of the planar image t [N, J, P] with W [J, C], then
 * FusedLeakyReLU) in one pass: x[n,p,c] = gain * lrelu(sum_j t[n,j,p] * W[j,c] + bias[c]); ex (may be NULL) adds a split image. */
int rick_d_input_f32(const float *t, const float *W, const float *bias, float *x, int N, int64_t P, int C, int J,
                     float slope, float gain, const rick_split_out *ex, void *stream);
/* Bound of an activation tail for the producers above, evaluated on the device (one tiny launch, no host sync):
 *   out[slot 0] = max|mul| * gain * (c0 * amax(w0) + max|nw| * amax(w_noise) + max|bias|)
 * — |gain * lrelu(v + nw * noise + bias) * mul[n,c]| for |v| <= c0 * amax(w0).  Any of nw / w_noise, bias, mul may be NULL
 * (term dropped / factor 1).  out is an amax word (the other slots are zeroed). */
int rick_bound_tail_f32(float *out_word, const float *w0, float c0, const float *nw, const float *w_noise,
                        const float *bias, int nbias, float gain, const float *mul, int nmul, void *stream);
/* rick_bias_act_bwd_split_f32 for modulated layers: image 1 = adjoint * chan_scale[n, c] (chan_scale [rows / rows_per_img, C]),
 * bounded by the amax word bound1 alone (|scale| * max |chan_scale| * max |g|, combined by rick_bound_tail_f32); out_f32
 * (may be NULL) also receives the unscaled adjoint. */
int rick_bias_act_bwd_split2_f32(const float *g, const float *ref, void *out1, float *hdr1, void *out2, float *hdr2,
                                 float mul2, const float *amax_g, const float *chan_scale, const float *bound1,
                                 float *out_f32, float *gb, float *gnw, const float *noise,
                                 int64_t rows, int C, int64_t rows_per_img, int64_t noise_nb, int64_t noise_hw,
                                 float alpha, float scale, float *partials, int accumulate, void *stream);
int rick_add_scale_split_f32(const float *a, const float *b, float *y, void *y_split, float *hdr,
                             const float *amax_a, const float *amax_b, int64_t rows, int C, float alpha, void *stream);
int rick_split_pack_f32(const float *x, void *out, float *hdr, const float *amax0, const float *amax1, float coef,
                        int64_t npix, int C, void *stream);
int rick_split_unpack_f32(const void *split, const float *hdr, float *out, int64_t npix, int C, void *stream);
/* Weight gradient (rick_conv_wgrad_f32) with one or both operands given as split images: x_hdr / gy_hdr non-NULL marks
 * the operand as a split image (its per-channel scales, if the layer has any, are already folded in by the producer).
 * Only geometries for which rick_conv_wgrad_split_supported() returns 1 (whole 64-position tiles, Co % 128 == 0,
 * Ci % 32 == 0: every 3x3 / 1x1 layer of both networks at >= 8x8). */
int rick_conv_wgrad_split_supported(const rick_conv_geom *g);
/* rick_conv_igemm_act_f32 / rick_convt2_f32 with the input given as a split image (Ci % 32 == 0; per-channel input scales
 * are folded into the image by its producer).  The igemm entry serves the 3x3 stride-1 / stride-2 forms with a full grid and
 * the small-patch (1x1, parity-class) form; other geometries return RICK_EINVAL and take the fp32 entry. */
int rick_conv_igemm_split_supported(const rick_conv_geom *g);
int rick_conv_igemm_split_f32(const void *x_split, const float *x_hdr, const void *packed_w, float *out,
                              const float *oscale, const rick_conv_geom *g, const rick_conv_epilogue *epilogue,
                              void *workspace, void *stream);
int rick_convt2_split_f32(const void *x_split, const float *x_hdr, const void *packed_w, float *out, const float *oscale,
                          int N, int IH, int IW, int Ci, int Co, int OH, int OW, float alpha, float *amax /* word or NULL */,
                          void *workspace, void *stream);
int rick_conv_wgrad_split_f32(const void *x, const float *x_hdr, const void *gy, const float *gy_hdr, float *gw,
                              int64_t s_co, int64_t s_ci, int64_t s_t, const rick_conv_geom *g, int accumulate,
                              void *workspace, void *stream);

/* ---------------------------------------------------------------------------------------
 * Thin (J <= 4 channel) products for the RGB side (ToRGB 1x1 modulated conv,
 * model_probe_tune.py:351-370; discriminator input conv, :679).  x is NHWC [N, P, C],
 * the thin tensor is planar [N, J, P], W is [N or 1, J, C] (w_bstride = J*C or 0).
 *   fwd :  t[n,j,p]  = sum_c x[n,p,c] * W[n,j,c]  (+ add[n,j,p] if add)
 *   bwdx:  x[n,p,c]  = sum_j t[n,j,p] * W[n,j,c]
 *   wgrad: G[n,j,c]  = sum_p t[n,j,p] * x[n,p,c]   (partials: float[N*J*C*rick_thin_wgrad_blocks]) */
int rick_thin_fwd_f32(const float *x, const float *W, int64_t w_bstride, const float *add,
                      float *t, int N, int64_t P, int C, int J, void *stream);
int rick_thin_bwdx_f32(const float *t, const float *W, int64_t w_bstride, float *x,
                       int N, int64_t P, int C, int J, void *stream);
/* ToRGB (model_probe_tune.py:246-248, 366-370) with the per-sample weight formed on the fly,
 * W[n,j,c] = (wscale * w[j,c]) * s[n,c]  (w [J, C] shared, s [N, C] the style; both 16-byte aligned):
 *   fwd :  t[n,j,p] = sum_c x[n,p,c] * W[n,j,c] + bias[j] (+ add[n,j,p])     (bias / add may be NULL)
 *   bwdx:  gx[n,p,c] = sum_j g[n,j,p] * W[n,j,c] */
int rick_torgb_fwd_f32(const float *x, const float *w, const float *s, float wscale, const float *bias,
                       const float *add, float *t, int N, int64_t P, int C, int J, void *stream);
int rick_torgb_bwdx_f32(const float *g, const float *w, const float *s, float wscale, float *gx, int N, int64_t P,
                        int C, int J, void *stream);
/* ... added INTO gx (gx[n,p,c] += ...): the activation that feeds ToRGB also feeds the next layer, whose data gradient is
 * already in gx — the second gradient arriving at the branch point is added by the kernel that produces it (same fp32 addition
 * as autograd's accumulation: torch.equal). */
int rick_torgb_bwdx_acc_f32(const float *g, const float *w, const float *s, float wscale, float *gx, int N, int64_t P,
                            int C, int J, void *stream);
int rick_thin_wgrad_blocks(int64_t P);
int rick_thin_wgrad_f32(const float *t, const float *x, float *G, int N, int64_t P, int C, int J,
                        float *partials, void *stream);

/* ---------------------------------------------------------------------------------------
 * Elementwise / reduction helpers on NHWC [N, P, C] tensors. */
/* y[n,p,c] = x[n,p,c] * s[n,c] */
int rick_chan_scale_f32(const float *x, const float *s, float *y, int N, int64_t P, int C, void *stream);
/* d[n,c] = sum_p a[n,p,c] * b[n,p,c] (/ divisor[n,c] when divisor != NULL); partials: float[N*C*rick_hw_dot_blocks(P)] */
int rick_hw_dot_blocks(int64_t P);
int rick_hw_dot_f32(const float *a, const float *b, float *d, int N, int64_t P, int C,
                    float *partials, const float *divisor, void *stream);
/* rick_hw_dot_f32 that also writes scaled[n,p,c] = a[n,p,c] * scale[n,c] in the same pass (C % 4 == 0). */
int rick_hw_dot_scale_f32(const float *a, const float *b, float *d, const float *scale, float *scaled, int N,
                          int64_t P, int C, float *partials, void *stream);
/* d[n,c] = sum_p g[n,p,c] * (lrelu^-1(y[n,p,c]) - noise_w[0]*noise[n % noise_nb][p] - bias[c]) where y is the output
 * of a fused tail gain*lrelu_slope(v + bias + noise_w*noise): the sum over pixels of g times the PRE-tail value v,
 * without keeping v (demodulation gradient of the fused StyledConv).  C % 4 == 0; partials and divisor as
 * rick_hw_dot_f32. */
int rick_hw_dot_act_f32(const float *g, const float *y, float *d, int N, int64_t P, int C, const float *bias,
                        const float *noise, const float *noise_w, int noise_nb, float slope, float gain,
                        float *partials, const float *divisor, void *stream);
/* y = (a + b) * alpha  (ResBlock merge, model_probe_tune.py:658); b may be NULL */
int rick_add_scale_f32(const float *a, const float *b, float *y, int64_t n, float alpha, void *stream);

/* Minibatch standard deviation (model_probe_tune.py:748-756) on NHWC x[B, P, C]: `groups` runs of
 * B/groups consecutive samples, each treated like one discriminator call whose stddev group is its whole
 * batch: out[B, P, C+1], channel C = mean_{p,c} sqrt(var_b(x) + 1e-8) of the sample's run; backward.
 * (groups = 2 lets D(fake) and D(real) of the D step share one pass with unchanged results.) */
int rick_mbstd_fwd_f32(const float *x, float *out, float *stat, int B, int P, int C, int groups, void *stream);
int rick_mbstd_bwd_f32(const float *x, const float *gout, float *gx, int B, int P, int C, int groups, void *stream);

/* ---------------------------------------------------------------------------------------
 * Fisher information + optimiser side (train_dynamic_update_prune.py:252-269, 279-299,
 * 427-438, 68-73, 908-931). */
/* acc[i] += g[i]^2 */
int rick_sq_accumulate_f32(float *acc, const float *g, int64_t n, void *stream);
/* out[f] = scale * sum_{o, i} x[o*outer_stride + f*filter_stride + i], i < inner
 * (per-filter mean of a Fisher tensor: one wavefront-shuffle reduction per filter) */
int rick_filter_reduce_f32(const float *x, float *out, int64_t outer, int64_t outer_stride,
                           int64_t nfilters, int64_t filter_stride, int64_t inner,
                           float scale, void *stream);
/* Style demodulation of the modulated convolution (model_probe_tune.py:246-252; w is [O, I, K] contiguous):
 *   rick_wsq_f32          wsq[o,i] = scale^2 * sum_k w[o,i,k]^2
 *   rick_demod_f32        d[b,o]   = rsqrt(sum_i s[b,i]^2 wsq[o,i] + eps)                      (B <= 32)
 *   rick_demod_bwd_s_f32  gs[b,i]  = 2 s[b,i] sum_o t[b,o] wsq[o,i],   t = -0.5 d^3 gd
 *   rick_demod_bwd_w_f32  gw[o,i,k] = 2 scale^2 w[o,i,k] sum_b t[b,o] s[b,i]^2 */
int rick_wsq_f32(const float *w, float *wsq, int O, int I, int K, float scale, void *stream);
int rick_demod_f32(const float *s, const float *wsq, float *d, int B, int I, int O, float eps, void *stream);
int rick_demod_bwd_s_f32(const float *s, const float *wsq, const float *d, const float *gd, float *gs, int B, int I, int O,
                         void *stream);
int rick_demod_bwd_w_f32(const float *w, const float *s, const float *d, const float *gd, float *gw, int B, int I, int O,
                         int K, float scale, int accumulate, void *stream);
/* Modulation bank: s_l = EqualLinear_l(latent[:, idx_l]) for EVERY modulated convolution of the generator
 * (ModulatedConv2d.modulation, model_probe_tune.py:233,246) in one launch, and the weight / bias gradients of all of
 * them in one more.  lat is [B, n_latent, K]; layer l owns blocks [blk_begin, blk_begin + rick_modbank_blocks(C_l));
 *   fwd: out[io_off + b*C + c] = scale * sum_k lat[b, lat_idx, k] * w[c*K + k] + b[c]
 *   bwd: grad[gw_off + c*K + k] = scale * sum_b gs[io_off + b*C + c] * lat[b, lat_idx, k];  grad[gb_off + c] = sum_b gs[..]
 * (gw_off / gb_off < 0: no weight / bias gradient; a layer with neither is skipped and its gs is not read;
 * accumulate != 0: the gradients are ADDED to what grad holds — grad + offsets then address the parameters' own
 * gradient buffers).  `descs_device` lives in device memory.  K % 256 == 0, B <= 8, grad 16-byte aligned.  The forward
 * stages the latent rows in LDS: B * K * 4 bytes > 64 KB is refused with RICK_EINVAL before anything is launched. */
typedef struct {
    const float *w;         /* [C, K] */
    const float *b;         /* [C] or NULL */
    int64_t io_off;         /* float offset of s_l / gs_l ([B, C] contiguous) */
    int64_t gw_off, gb_off; /* float offsets of the weight / bias gradient */
    int C, lat_idx, blk_begin, reserved;
} rick_modbank_desc;
int rick_modbank_blocks(int C);
int rick_modbank_fwd_f32(const float *lat, int B, int n_latent, int K, const rick_modbank_desc *descs_device, int n,
                         int total_blocks, float scale, float *out, void *stream);
int rick_modbank_bwd_f32(const float *lat, const float *gs, int B, int n_latent, int K, const rick_modbank_desc *descs_device,
                         int n, int total_blocks, float scale, float *grad, int accumulate, void *stream);
/* Demodulation bank: the demodulation coefficients of EVERY demodulated convolution of a generator (model_probe_tune.py:246-252)
 * in one launch, their weight gradient in one more, wsq[o,i] = scale^2 sum_k w[o,i,k]^2 in a third that only runs when the
 * weights have changed.  Same arithmetic and order per element as rick_wsq_f32 / rick_demod_f32 / rick_demod_bwd_w_f32
 * (bit-identical).  Layer l reads s_l [B, I] at float offset s_off of the modulation bank's flat output and owns d_l / gd_l
 * [B, O] at d_off of the flat coefficient / gradient buffers; gw (the parameter's gradient buffer, accumulated into) may be NULL.
 * Block ranges: [blk_wsq, next) of rick_demod_blocks_wsq(O, I) blocks for the wsq and weight-gradient launches,
 * [blk_demod, next) of rick_demod_blocks(O) for the coefficient launch, [blk_bwd_s, next) of rick_demod_blocks_bwd_s(I) for the
 * style gradient gs_l [B, I] (written at s_off of gs_flat).  B <= 8. */
typedef struct rick_demod_desc {
    const float *w;         /* [O, I, K] contiguous */
    float *wsq;             /* [O, I] */
    float *gw;              /* [O, I, K] or NULL */
    int64_t s_off, d_off;
    int O, I, K;
    float scale2;           /* (conv scale)^2 */
    int blk_wsq, blk_demod, blk_bwd_s, reserved;
} rick_demod_desc;
int rick_demod_blocks_wsq(int O, int I);
int rick_demod_blocks(int O);
int rick_wsq_multi_f32(const rick_demod_desc *descs_device, int n, int total_blocks, void *stream);
int rick_demod_multi_f32(const float *s_flat, float *d_flat, const rick_demod_desc *descs_device, int n, int total_blocks,
                         int B, int max_I, float eps, void *stream);
int rick_demod_bwd_w_multi_f32(const float *s_flat, const float *d_flat, const float *gd_flat,
                               const rick_demod_desc *descs_device, int n, int total_blocks, int B, void *stream);
int rick_demod_blocks_bwd_s(int I);
int rick_demod_bwd_s_multi_f32(const float *s_flat, const float *d_flat, const float *gd_flat, float *gs_flat,
                               const rick_demod_desc *descs_device, int n, int total_blocks, int B, int max_O, void *stream);
/* EqualLinear forward on a short batch (the mapping network, model_probe_tune.py:139-173, 418-428; no autograd):
 *   x' = pixelnorm ? x * rsqrt(mean_k x^2 + 1e-8) : x                                  (PixelNorm, :92-98)
 *   out[b,o] = act(scale * sum_k x'[b,k] W[o,k] + bias[o] * bias_mul);  act != 0: gain * leaky_relu(., slope)
 * x [B, K], W [O, K], bias [O] or NULL, out [B, O].  B <= 16, K % 4 == 0, x / W 16-byte aligned.  x is staged in LDS:
 * B * K * 4 bytes > 160 KB (the CU's LDS; the discriminator's [4, 8192] layer takes 128 KB) is refused with RICK_EINVAL
 * before anything is launched. */
int rick_equal_linear_f32(const float *x, const float *W, const float *bias, float *out, int B, int K, int O,
                          float scale, float bias_mul, int act, float slope, float gain, int pixelnorm, void *stream);
/* EqualLinear WITH gradients on a short batch (the discriminator's final layers, model_probe_tune.py:699-702, in every D pass;
 * F.linear(input, weight * scale, bias * lr_mul) of :157-168): three products closed under differentiation, each one pass
 * over the [O, K] matrix, summed in a fixed order (bit-reproducible run to run — the library GEMMs they replace may use
 * atomically accumulated split-K solutions for M = batch, K = 8192).  B <= 16, K % 4 == 0, matrices 16-byte aligned.
 *   fwd   out[b,o] = alpha * sum_k x[b,k] W[o,k] + bias_mul * bias[o]          (bias may be NULL)
 *   dgrad out[b,k] = alpha * sum_o g[b,o] W[o,k]
 *   wgrad gw[o,k] (+)= alpha * sum_b g[b,o] x[b,k];  gb[o] (+)= bias_mul * sum_b g[b,o]   (gw or gb may be NULL)
 * `workspace`: rick_linear_{fwd,dgrad}_workspace_floats() floats (0: may be NULL), 16-byte aligned. */
int64_t rick_linear_fwd_workspace_floats(int B, int K, int O);
int rick_linear_fwd_f32(const float *x, const float *W, const float *bias, float *out, int B, int K, int O, float alpha,
                        float bias_mul, float *workspace, void *stream);
int64_t rick_linear_dgrad_workspace_floats(int B, int K, int O);
int rick_linear_dgrad_f32(const float *g, const float *W, float *out, int B, int K, int O, float alpha, float *workspace,
                          void *stream);
int rick_linear_wgrad_f32(const float *g, const float *x, float *gw, float *gb, int B, int K, int O, float alpha,
                          float bias_mul, int accumulate, void *stream);

/* Masked Adam over a flat parameter buffer (mask bits: 1 = freeze (grad := 0),
 * 2 = prune (param := 0, grad := 0); mask may be NULL), torch.optim.Adam semantics
 * (no weight decay, no amsgrad), bias corrections passed in. */
int rick_masked_adam_f32(float *p, float *g, float *m, float *v, const uint8_t *mask, int64_t n,
                         float lr, float beta1, float beta2, float eps, float bc1, float bc2,
                         void *stream);
/* The same update with the step counters and bias corrections kept in DEVICE memory, so that a whole train step
 * (incl. the optimiser) can be captured once into a hipGraph and replayed: rick_adam_prepare_f32 increments
 * steps[first .. first+count) (int32, all equal) and writes bc = {1 - beta1^t, 1 - beta2^t} for the new count t;
 * rick_masked_adam_dev_f32 is rick_masked_adam_f32 reading the two corrections from `bc`. */
int rick_adam_prepare_f32(int *steps, int first, int count, float beta1, float beta2, float *bc, void *stream);
int rick_masked_adam_dev_f32(float *p, float *g, float *m, float *v, const uint8_t *mask, int64_t n,
                             float lr, float beta1, float beta2, float eps, const float *bc, void *stream);
/* ema[i] = ema[i]*decay + p[i]*(1-decay) */
int rick_ema_f32(float *ema, const float *p, int64_t n, float decay, void *stream);

/* ---------------------------------------------------------------------------------------
 * Data path (dataset.py:8-40, train_dynamic_update_prune.py:789-843).  The dataset stays resident in device memory as
 * uint8 [N, H, W, 3]; one launch builds a training batch: out[b, c, y, x] = (images[index[b], y, flip[b] ? W-1-x : x, c]
 * / 255 - 0.5) / 0.5 — ToTensor + RandomHorizontalFlip + Normalize(0.5, 0.5) of the reference transform, [B, 3, H, W]. */
int rick_image_batch_f32(const uint8_t *images, const int64_t *index, const uint8_t *flip, float *out,
                         int N, int H, int W, int B, void *stream);
/* PNG scanline reconstruction (filter types 0-4), in place, HOST memory: H rows of 1 filter byte + stride bytes. */
int rick_png_unfilter(uint8_t *data, int H, int stride, int bpp);

/* ---------------------------------------------------------------------------------------
 * Adaptive discriminator augmentation — replaces augment(img, p, (G, C)) of non_leaking.py:316-398 (random_apply_affine:
 * reflect pad -> upfirdn2d(up=2) -> grid_sample -> upfirdn2d(down=2) -> crop; random_apply_color) for given matrices.
 * Images are planar fp32 [N, 3, H, W], contiguous (the generator's output, the rick_image_batch_f32 batch, the
 * discriminator's input).  Per-sample parameters live in device memory (`params`, N entries), so a captured graph replays
 * with new transforms after one copy into the block:
 *   a     maps warped-region pixel (c, r) to up-sampled canvas coordinates: ix = a0 c + a1 r + a2, iy = a3 c + a4 r + a5
 *         (the region is warped-canvas rows 2 py1 .. 2 py1 + 2H + 9, columns 2 px1 .. 2 px1 + 2W + 9);
 *   ainv  the inverse of the 2x2 part (c = ainv0 ex + ainv1 ey, r = ainv2 ex + ainv3 ey for ex = ix - a2, ey = iy - a5);
 *   col   the first three rows of the 4x4 colour matrix, row-major;
 *   py1, px1  the sample's low reflect pads (without the 6 of the FIR), hp, wp its padded-canvas size
 *         (H + py1 + py2 + 12, W + px1 + px2 + 12); the up-sampled canvas is (2 hp - 11) x (2 wp - 11).
 * Pads must satisfy pad + 6 < H (resp. W), as the reference's reflect pad requires.
 * rick_augment_fwd_f32: out = augment(x) (bias != 0: with the colour offset col[:, 3]; 0: the linear part only);
 * rick_augment_adj_f32: gx = the transpose of the linear part applied to gy.  Both use `ws`, rick_augment_workspace_floats()
 * floats, and write every element of their output (no accumulation, no atomics: bit-identical from run to run). */
typedef struct {
    double a[6];
    double ainv[4];
    float col[12];
    int py1, px1, hp, wp;
} rick_aug_param;
int64_t rick_augment_workspace_floats(int N, int H, int W);
int rick_augment_fwd_f32(const float *x, const rick_aug_param *params, float *ws, float *out, int N, int H, int W, int bias,
                         void *stream);
int rick_augment_adj_f32(const float *gy, const rick_aug_param *params, float *ws, float *gx, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * Inception — the torchvision InceptionV3 feature extractor up to pool3 (rick_amd/inception.py), the network behind
 * the reference's FID (gan_training/metrics/inception.py).  Activations NHWC fp32; BatchNorm folded on the host.
 * rick_inc_input_f32: planar images x [N, 3, H, W] -> bilinear resize to OH x OW (F.interpolate, align_corners=False)
 *   and the ImageNet affine x * (std / 0.5) + (mean - 0.5) / 0.5 -> out [N, OH, OW, 4] (channel 3 = 0).
 * rick_inc_conv_f32: out = relu(conv(in, W) + bias) as an implicit GEMM on the f32-input MFMA (exact fp32 products).
 *   in [N, IH, IW, Ci] (Ci % 4 == 0); wpk [Kp][Cop] with K = KH*KW*Ci ordered (ky, kx, ci), Kp = K rounded up to 32,
 *   Cop = Co rounded up to bn (64 or 128), zero-padded; bias [Cop].  Output columns [seg_start[s], seg_start[s+1]) go to
 *   dst[s] + pixel * ldc[s] + c0[s] (a channel slice of a wider NHWC tensor: concats are free); seg_start[0] = 0, unused
 *   slots >= Co.  Columns of one GEMM that read the same input (the fused 1x1 heads) are routed this way.
 * rick_inc_conv_bwd_f32: the data gradient of a 3x3 stride-1 pad-1 convolution, the same implicit GEMM with another epilogue
 *   (rick_inc_conv_f32's kernels are unchanged): gout [N, H, W, Ci] is the gradient of the forward convolution's output (Ci =
 *   its output channels, Ci % 4 == 0), Co its input channels; wt [Kp][Cop] is the transposed, 180-degree rotated filter packed
 *   once, wt[(ky, kx, co_f)][ci_f] = W[co_f][ci_f][2 - ky][2 - kx], padded like wpk.  a: KH = KW = 3, SH = SW = PH = PW = 1,
 *   OH = IH, OW = IW, nseg = 1, c0[0] = 0, ldc[0] = Co.  No bias, no ReLU:
 *   dst[0][p, c] = (mask[p, c] > 0) ? acc + add[p, c] : 0, with mask the stored forward activation the gradient is taken with
 *   respect to (torch's ReLU rule, out > 0) and add a gradient that reaches that activation by another way (a tap); both
 *   [M, Co] like the output, either may be NULL (no mask / nothing added).  No split-K: an image's gradient is bit-identical
 *   whatever batch it is computed in.
 * rick_inc_maxpool_f32: 3x3 stride 2 max, no padding, [N, IH, IW, C] -> channels [c0, c0 + C) of an ldc-wide output.
 * rick_inc_avgpool_f32: 3x3 stride 1 pad 1 average with count_include_pad, [N, H, W, C] -> same shape.
 * rick_inc_mean_f32: [N, HW, C] -> [N, C] mean over HW in pixel order.
 * rick_inc_input_raw_f32: rick_inc_input_f32's resize without the affine, for the Inception Score's network
 *   (gan_training/metrics/inception_score.py: inception_v3(transform_input=False) on the images as they are, or after
 *   nn.Upsample(size=(299, 299), mode='bilinear')).  At OH == H and OW == W it copies the values bit for bit.
 * rick_is_rows_f32: logits [M, C] (C >= 1) -> p [M, C] fp32 = softmax of each row as F.softmax forms it (subtract the row
 *   maximum, expf, divide by the fp32 sum), and per row in fp64 s[m] = sum_c p[m, c] and h[m] = sum_c q log q with
 *   q = p / s[m]; a term with p == 0 is exactly 0.  One wave per row: lane l adds the classes l, l + 64, ... in ascending
 *   order (lanes past C hold -inf for the maximum and 0 for the sums), then a 32, 16, ..., 1 xor butterfly.
 * rick_is_accum_f64: folds the M rows of one call into the statistic acc [S][2 C + 1] fp64: per split the class sums of p,
 *   the class sums of q = p / s and the sum of h.  The call's row i is row g = row0 + i of the sample and belongs to split
 *   g / per (per = N_total / S); rows with g >= S * per are ignored.  One thread owns one (split, column) accumulator and adds
 *   the call's rows in ascending order onto the stored value: the state after the whole sample is bit-identical however the
 *   sample was cut into calls.  acc starts as zeros.
 * No atomics: every output element has one writer and a fixed summation order (bit-identical from run to run). */
typedef struct {
    int N, IH, IW, Ci, KH, KW, SH, SW, PH, PW, OH, OW;
    int Co, Cop, bn, nseg;
    int seg_start[4], ldc[4], c0[4];
    float *dst[4];
} rick_inc_conv;
int rick_inc_input_f32(const float *x, float *out, int N, int H, int W, int OH, int OW, void *stream);
int rick_inc_conv_f32(const float *in, const float *wpk, const float *bias, const rick_inc_conv *a, void *stream);
int rick_inc_conv_bwd_f32(const float *gout, const float *wt, const float *mask, const float *add, const rick_inc_conv *a,
                          void *stream);
int rick_inc_maxpool_f32(const float *in, float *out, int N, int IH, int IW, int C, int ldc, int c0, void *stream);
int rick_inc_avgpool_f32(const float *in, float *out, int N, int H, int W, int C, void *stream);
int rick_inc_mean_f32(const float *in, float *out, int N, int HW, int C, void *stream);
int rick_inc_input_raw_f32(const float *x, float *out, int N, int H, int W, int OH, int OW, void *stream);
int rick_is_rows_f32(const float *logits, float *p, double *s, double *h, int M, int C, void *stream);
int rick_is_accum_f64(const float *p, const double *s, const double *h, double *acc, int M, int C, int S, int64_t row0,
                      int64_t per, void *stream);

/* ---------------------------------------------------------------------------------------
 * LPIPS — lpips 0.1 with the VGG16 backbone (rick_amd/lpips.py), the metric behind the reference's intra-cluster LPIPS
 * (gan_training/eval.py).  The 13 convolutions run on rick_inc_conv_f32; activations and taps are NHWC fp32.
 * rick_lpips_input_f32: planar [N, 3, H, W] -> out [N, H, W, 4] (channel 3 = 0) through lpips' scaling layer
 *   (x - shift) / scale.  mode 0: float x as is.  mode 1: float x through the reference's PNG round trip,
 *   q = uint8(clamp((x / 2 + 0.5) * 255 + 0.5, 0, 255)), then (q / 255 - 0.5) / 0.5; q is also written to u8out (planar,
 *   may be NULL).  mode 2: uint8 xq, then (q / 255 - 0.5) / 0.5.  Every step is one correctly rounded fp32 operation.
 * rick_lpips_maxpool2_f32: 2x2 stride 2 max with floor, [N, IH, IW, C] -> [N, IH / 2, IW / 2, C] (C % 4 == 0).
 * rick_lpips_invnorm_f32: in [P, C] -> out[p] = 1 / (sqrt(sum_c in[p, c]^2) + 1e-10); 0 where the sum is 0.
 * rick_lpips_pair_f32: one tap of two image sets, fa [na, HW, C] with inverse norms ia [na, HW], fb / ib likewise, lin
 *   weights w [C] (C <= 1024) -> part[s][i][j] (fp64) = sum over the positions [s pps, (s + 1) pps) of slice s and all
 *   channels of w_c (fa_ic ia_i - fb_jc ib_j)^2, for s < ceil(HW / pps).  Summation order depends on (position, channel)
 *   only: d(x, x) = 0 and D(A, B) = D(B, A)^T exactly, and a pair's value does not depend on the other images of the call.
 * rick_lpips_paired_f32: one tap of n pairs, image i of fa against image i of fb only.  Image i of fa is at fa + i sa HW C with
 *   its inverse norms at ia + i sa HW (sa, sb >= 1: strides in images; with sa = sb = 2, fb = fa + HW C and ib = ia + HW one set of
 *   2n interleaved images serves as both operands) -> part[s][i] (fp64), the layout rick_lpips_reduce_f32 reads with na = n,
 *   nb = 1.  Every value is bit-identical to part[s][i][i] of rick_lpips_pair_f32 for the same two images: the same fp32 chain
 *   inside each 256-element stage, the same fp64 sum of stages.  Work and partials are proportional to n.  pps * C <= 8192.
 * rick_lpips_reduce_f32: part = the nlayers taps' partials one after the other ([nslices[l]][na][nb] each) -> out [na, nb]
 *   fp32 = sum over taps in order of (sum over slices in order) / hw[l], in fp64.
 * The backward pass of the paired distance (rick_amd/lpips.py: LPIPS.loss), first order, with respect to the image:
 * rick_lpips_tap_bwd_f32: one tap.  a [n, HW, C] with inverse norms ia [n, HW] (the image), t / it the target's, of nt = n
 *   images or nt = 1 image broadcast, lin weights w [C] (C % 4 == 0, C <= 1024), upstream gradient go [n] ->
 *   g [n, HW, C] = d/da of go (1 / HW) sum_p sum_c w_c (a_c ia - t_c it)^2: with u = a ia, r_c = 2 w_c (u_c - t_c it) go / HW
 *   and |a| = 1 / ia - 1e-10, g_k = ia r_k - a_k (sum_c r_c a_c) ia^2 / |a|; exactly 0 where ia = 0, and exactly 0 where the
 *   image equals the target.  One wave per position: lane l sums channels 4 l + 256 j (j ascending), then the wave_sum
 *   butterfly.  relu != 0 also applies the ReLU rule g = (a > 0) ? g : 0 (the gradient in front of the tap's ReLU).
 * rick_lpips_maxpool2_bwd_f32: the adjoint of rick_lpips_maxpool2_f32 in gather form, fused with the stage output's tap
 *   gradient and ReLU mask.  act [N, IH, IW, C] is the pooled activation, gpool [N, IH / 2, IW / 2, C] the gradient of the pool's
 *   output, add [N, IH, IW, C] (may be NULL) the tap gradient:
 *   out[p] = (act[p] > 0) ? add[p] + (p is the first maximum of its window in (dy, dx) scan order ? gpool[window] : 0) : 0.
 *   Positions that the floor leaves outside every window receive only add.
 * rick_lpips_input_bwd_f32: the adjoint of rick_lpips_input_f32, mode 0: g [N, H, W, 4] -> out [N, 3, H, W] planar,
 *   out = g_c / scale_c (one correctly rounded fp32 division).
 * No atomics: every output element has one writer and a fixed summation order. */
typedef struct {
    int nlayers;
    int nslices[8], hw[8];
} rick_lpips_layers;
int rick_lpips_input_f32(const float *x, const uint8_t *xq, float *out, uint8_t *u8out, int N, int H, int W, int mode,
                         void *stream);
int rick_lpips_maxpool2_f32(const float *in, float *out, int N, int IH, int IW, int C, void *stream);
int rick_lpips_invnorm_f32(const float *in, float *out, int64_t P, int C, void *stream);
int rick_lpips_pair_f32(const float *fa, const float *ia, int na, const float *fb, const float *ib, int nb, const float *w,
                        int HW, int C, int pps, double *part, void *stream);
int rick_lpips_paired_f32(const float *fa, const float *ia, int sa, const float *fb, const float *ib, int sb, int n, const float *w,
                          int HW, int C, int pps, double *part, void *stream);
int rick_lpips_reduce_f32(const double *part, float *out, int na, int nb, const rick_lpips_layers *d, void *stream);
int rick_lpips_tap_bwd_f32(const float *a, const float *ia, const float *t, const float *it, int n, int nt, const float *w,
                           const float *go, int HW, int C, int relu, float *g, void *stream);
int rick_lpips_maxpool2_bwd_f32(const float *act, const float *add, const float *gpool, float *out, int N, int IH, int IW, int C,
                                void *stream);
int rick_lpips_input_bwd_f32(const float *g, float *out, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * PPL — the latent path points of the perceptual path length (rick_amd/ppl.py; Karras et al., StyleGAN / StyleGAN2).
 * rick_ppl_latents_f32: a, b [B, L] fp32, t [B] -> out [2B, L]: row 2i is the path point at t[i], row 2i + 1 the point at
 *   t[i] + eps (1 <= L <= 1024, eps finite and > 0).
 *   mode 0 (W space): a + (b - a) t, both rows from the same fp32 d = b - a.
 *   mode 1 (Z space): slerp.  an = a / |a|, bn = b / |b|, d = clamp(sum an bn, -1, 1), p = t acos(d), c = normalize(bn - d an),
 *   out = normalize(an cos p + c sin p); normalize divides by max(norm, 1e-12), so a == b yields an.
 *   One wave per pair; between the fp32 loads and stores the arithmetic is fp64 (per-lane FMA chains over elements
 *   lane + 64 j, j ascending, then the fixed 32 ... 1 xor butterfly), so each output is the fp32 rounding of a value exact to
 *   ~1e-15.  No atomics, run-to-run identical, capture-safe; a pair's two rows depend on that pair alone.
 *   RICK_EINVAL for a null pointer, B < 0, L outside [1, 1024], eps not finite or <= 0, mode outside {0, 1}. */
int rick_ppl_latents_f32(const float *a, const float *b, const float *t, double eps, float *out, int B, int L, int mode,
                         void *stream);

/* ---------------------------------------------------------------------------------------
 * VGG16 fc2 — the features behind the reference's improved precision / recall (rick_amd/vgg.py;
 * gan_metrics/precision_recall.py:124-152, IPR.extract_features, called from gan_training/eval.py:58-65).  The 13
 * convolutions of vgg16.features run on rick_inc_conv_f32 and its five 2x2 max pools on rick_lpips_maxpool2_f32 (the last
 * one, 14^2 -> 7^2, included); activations are NHWC fp32.
 * rick_vgg_input_f32: planar x [N, 3, H, W] -> out [N, 224, 224, 4] (channel 3 = 0), the reference's
 *   F.interpolate(size=(224, 224)) (precision_recall.py:135-139, 146; default mode 'nearest'): source index
 *   min(int(floorf(dst * (float(in) / float(out)))), in - 1) with the scale in fp32; the identity at 224.  Values are copied:
 *   there is no affine on this path.
 * rick_fc_f32: out[M, N] = act(x[M, K] W^T + bias), 1 <= M <= 64, act = ReLU if relu else identity: classifier[0] + [1] and
 *   classifier[3] of precision_recall.py:149 (Dropout is the identity in eval).  f32-input MFMA, exact fp32 products.
 *   wpk = W [N, K] packed once as [Np / 32][Kp / 8][64 lanes][4] (rick_fc_packed_floats(K, N) floats, Np = N rounded up to
 *   128, Kp = K rounded up to 8, zero padded): lane (h = lane >> 5, c = lane & 31) of column block nb and k block kb holds
 *   W[32 nb + c][8 kb + 2 j + h] in component j.  Stage 1 writes split-K partials ws[s][m][n] (rick_fc_workspace_floats(M, K,
 *   N) floats; the slicing is a function of (K, N) only), each the sum of two fp32 fma chains, over the even and over the odd k blocks of the
 *   slice, in the order k block ascending, j ascending, h ascending; stage 2 sums the slices in order, adds the bias and applies the activation.
 *   Row m of out is bit-identical whatever M is and whatever the other rows hold.  x rows are contiguous (stride K).
 * No atomics: every output element has one writer and a fixed summation order (bit-identical from run to run). */
int rick_vgg_input_f32(const float *x, float *out, int N, int H, int W, void *stream);
int64_t rick_fc_packed_floats(int K, int N);
int64_t rick_fc_workspace_floats(int M, int K, int N);
int rick_fc_f32(const float *x, const float *wpk, const float *bias, float *ws, float *out, int M, int K, int N, int relu,
                void *stream);

/* ---------------------------------------------------------------------------------------
 * CLIP — the ViT image tower of CLIP (Radford et al., 2021; rick_amd/clip.py): unnormalised image embeddings as
 * `encode_image` returns them, for FID / KID in CLIP space, and their gradient with respect to the image (the weights are
 * frozen: no weight gradients) for the CLIP-guided adaptation losses (rick_amd/clipguide.py).
 * Activations are fp32 rows [N * T][Wd] (T = G^2 + 1 tokens per image).
 * rick_clip_input_f32: planar x [N, 3, H, W] in [-1, 1] -> out [N, S, S, 4] (channel 3 = 0): F.interpolate(mode='bicubic',
 *   align_corners=False) to S x S (source s = (float(in) / float(S)) * (dst + 0.5) - 0.5, taps floor(s) - 1 .. floor(s) + 2
 *   with indices clamped at the border, cubic convolution weights with A = -0.75, no antialiasing, overshoot kept; the four
 *   taps of a row summed in order, then the four rows), then v = (x * 0.5 + 0.5 - mean_c) / std_c as four correctly rounded
 *   fp32 operations, mean = (0.48145466, 0.4578275, 0.40821073), std = (0.26862954, 0.26130258, 0.27577711).  At H == W == S
 *   the weights are exactly (0, 1, 0, 0): finite values are copied bit for bit before the affine.
 * rick_inc_conv_lin_f32: rick_inc_conv_f32's GEMM (same operands, same tiles, exact fp32 products, no split-K) with the
 *   linear epilogue v = acc + bias[col]; v = act(v), act = 0 the identity, 1 QuickGELU; v += res[m, col] if res != NULL.
 *   One destination: nseg = 1, written at dst[0] + m * ldc[0] + c0[0] + col; res is indexed like dst[0] and may be dst[0]
 *   itself (the in-place residual: every element is read and written by one thread).  QuickGELU in fp32, every operation
 *   rounded on its own: u * (1 / (1 + expf(-(1.702f * u)))).  A row's result does not depend on the other rows.  A linear
 *   layer on rows [M, K] is the 1 x 1 convolution of N = M images of 1 x 1 x K.
 * rick_clip_tokens_f32: patches [N, T - 1, C] (the patch GEMM's output, row-major patches), cls [C], pos [T, C] ->
 *   out [N, T, C] = LayerNorm([cls ; patches] + pos) with ln_pre's w, b [C].
 * rick_clip_layernorm_f32: rows in[r * ldx + c], r < R, c < C (ldx >= C: ln_post reads token 0 of every image with
 *   ldx = T * C) -> out [R, C] compact.  C % 4 == 0, C <= 2048, ldx % 4 == 0.
 *   Both: one wave per row, the row held in registers, lane l owning columns 4 l + 256 j.  Pass 1: the lane adds its columns
 *   in ascending order, then the 32, 16, ..., 1 xor butterfly; mean = sum / C.  Pass 2: the same order over fmaf(d, d, .),
 *   d = x - mean; var = sum / C (biased).  y = fmaf(d * (1 / sqrtf(var + eps)), w, b).
 * rick_clip_attention_f32: qkv [N, T, 3 Wd] (columns q | k | v, head h owning [h D, (h + 1) D) of each), Wd = heads * D,
 *   D in {16, 32, 64}, T <= 257 -> out [N, T, Wd] = softmax(q k^T / sqrt(D)) v per head.  One block per (image, head) with K
 *   and V of the head in LDS (up to 137 KB).  score[k] = (fmaf chain over c ascending) * (1 / sqrt(D)) in fp32; the row
 *   maximum is subtracted, e = expf, the denominator is the sum per lane over its keys l + 64 j ascending, then the xor
 *   butterfly; p = e / den; out[c] = fmaf chain of p[k] v[k][c] over k ascending.  A query row's result depends on its own
 *   image and head only.
 * The projection runs on rick_fc_f32.  Unsupported shapes return 22.
 * No atomics: every output element has one writer and a fixed summation order (bit-identical from run to run).
 * The data gradient.  The five GEMMs of the backward pass (c_proj, c_fc, out_proj, q/k/v with K = 3 Wd, the patch embedding
 * onto 4 P^2 columns) are rick_inc_conv_lin_f32 on the transposed operand with a zero bias and act = 0; the projection's is
 * rick_fc_f32 on the transposed head.  Around them:
 * rick_clip_quickgelu_f32: out[i] = u[i] * (1 / (1 + expf(-(1.702f * u[i])))), the act = 1 epilogue's five operations as a
 *   kernel of its own (the same bits), for a forward that keeps the pre-activation u.  out may be u.
 * rick_clip_quickgelu_bwd_f32: out[i] = g[i] * (s + 1.702f * u[i] * s * (1 - s)), s = 1 / (1 + expf(-(1.702f * u[i]))).  out
 *   may be g.
 * rick_clip_layernorm_bwd_f32: rows x[r * ldx + c] (the forward's input), g[r * ldg + c] (the gradient of the forward's
 *   output), w [C] -> out[r * ldo + c] = dx [+ add[r * ldo + c]]; add may be NULL or out.  Mean and rstd are recomputed in the
 *   forward's order; xhat = (x - mean) rstd, gw = g w, m1 = sum gw / C (the lane's columns ascending, then the butterfly),
 *   m2 = sum gw xhat / C (one fmaf chain per lane, then the butterfly), dx = rstd (gw - m1 - xhat m2).  No dw / db.  One wave
 *   per row, C % 4 == 0, C <= 2048, every stride >= C and a multiple of 4.
 * rick_clip_tokens_bwd_f32: the adjoint of rick_clip_tokens_f32 with respect to the patches: the same row gradient on
 *   x = patches + pos[t] for the tokens t >= 1, g [N, T, C] -> out [N, T - 1, C] (the class row is dropped).
 * rick_clip_attention_bwd_f32: qkv [N, T, 3 Wd] (the forward's input), g_out [N, T, Wd] -> g_qkv [N, T, 3 Wd]; stats
 *   [N, heads, T, 3] is scratch (row maximum, denominator, delta).  Two launches of one block per (image, head).  One, a wave
 *   per query row i with K and V in LDS: p recomputed by the forward's chain, dP_j = g_out_i . v_j (fmaf chain over c),
 *   delta_i = sum_j p_j dP_j (per lane over its keys ascending, then the butterfly), dQ_i = scale sum_j p_j (dP_j - delta_i)
 *   k_j (fmaf chain, j ascending).  Two, a wave per key row j with Q, g_out and the stats in LDS (up to 145 KB): p_ij =
 *   expf(s_ij - max_i) / den_i, dV_j = sum_i p_ij g_out_i, dK_j = scale sum_i p_ij (dP_ij - delta_i) q_i, fmaf chains with i
 *   ascending.  Nothing of size T x T goes to memory.  The forward's domain.
 * rick_clip_input_bwd_f32: the adjoint of rick_clip_input_f32.  g [N G^2][(ky, kx, c4)], G = S / P, is the patch embedding's
 *   data gradient in patch-row layout (pixel (G_y P + ky, G_x P + kx) of the S x S image); out [N, 3, H, W] planar.  Gather
 *   form: a source pixel sums, over the destination pixels that tap it in ascending (row, column) order, fmaf(wy wx, g, .)
 *   with the forward's fp32 weights (taps clamped onto one border pixel add their weights), then out = (sum * 0.5) / std_c.
 *   Source pixels that no destination taps get exact zeros; at H == W == S the result is exactly g * 0.5 / std_c.  S % P == 0.
 * The text tower (rick_amd/cliptext.py), forward only: its weights are frozen and its input is discrete.  It shares
 * rick_inc_conv_lin_f32, rick_clip_layernorm_f32 and rick_fc_f32 with the image tower; rows are [N * T][Wd], T positions per prompt.
 * rick_clip_text_tokens_f32: ids [N, T] int32, table [V, C], pos [T, C] -> out[n, t, :] = table[ids[n, t]] + pos[t], one fp32
 *   add per element, 16-byte accesses.  C % 4 == 0, C <= 2048, 1 <= T <= 257, V >= 1, N T C / 1024 (the blocks of the launch)
 *   below 2^31.  The ids are device memory: the host
 *   validates 0 <= id < V before upload, and the kernel forces every id into [0, V), so no launch reads outside the table.
 * rick_clip_attention_causal_f32: rick_clip_attention_f32 (the same kernel template: layout, LDS staging, key ownership, fmaf
 *   chains, butterfly, softmax form, domain) with query row i seeing the keys k <= i only.  A masked slot holds -inf before the
 *   maximum and adds an exact 0.f to the denominator, as a slot k >= T does in the unmasked kernel; the P V chain runs k = 0 ... i
 *   ascending.  Row i of a prompt of T tokens is therefore bit-identical to row i of rick_clip_attention_f32 on the first i + 1
 *   tokens, and depends on the rows <= i of its own prompt and head alone.  The score chains behind the diagonal are not run.
 * rick_clip_layernorm_rows_f32: in holds rows of C floats (compact), idx [R] int32 row numbers (device memory, any order,
 *   repeats allowed) -> out [R, C] = LayerNorm of row idx[r], the arithmetic of rick_clip_layernorm_f32 and the same bits as
 *   that entry on the same rows gathered contiguously.  The entry takes no row count and cannot read idx, so it CANNOT bound
 *   an index from above (a negative one is read as 0): a caller that passes an index past the rows of `in` makes the kernel
 *   read out of bounds.  Checking idx on the host before its upload is the caller's duty (rick_amd/cliptext.py check_rows).
 * All of them: one writer per output element, fixed summation order, a row's (image's, prompt's) result independent of the other
 * rows (images, prompts) of the launch, no host branch on device data. */
int rick_clip_text_tokens_f32(const int32_t *ids, const float *table, const float *pos, float *out, int N, int T, int V, int C,
                              void *stream);
int rick_clip_attention_causal_f32(const float *qkv, float *out, int N, int T, int heads, int D, void *stream);
int rick_clip_layernorm_rows_f32(const float *in, const int32_t *idx, const float *w, const float *b, float *out, int R, int C,
                                 float eps, void *stream);
int rick_clip_input_f32(const float *x, float *out, int N, int H, int W, int S, void *stream);
int rick_inc_conv_lin_f32(const float *in, const float *wpk, const float *bias, const float *res, int act,
                          const rick_inc_conv *a, void *stream);
int rick_clip_tokens_f32(const float *patches, const float *cls, const float *pos, const float *w, const float *b, float *out,
                         int N, int T, int C, float eps, void *stream);
int rick_clip_layernorm_f32(const float *in, int64_t ldx, const float *w, const float *b, float *out, int R, int C, float eps,
                            void *stream);
int rick_clip_attention_f32(const float *qkv, float *out, int N, int T, int heads, int D, void *stream);
int rick_clip_quickgelu_f32(const float *u, float *out, int64_t n, void *stream);
int rick_clip_quickgelu_bwd_f32(const float *u, const float *g, float *out, int64_t n, void *stream);
int rick_clip_layernorm_bwd_f32(const float *x, int64_t ldx, const float *w, const float *g, int64_t ldg, const float *add,
                                float *out, int64_t ldo, int R, int C, float eps, void *stream);
int rick_clip_tokens_bwd_f32(const float *patches, const float *pos, const float *w, const float *g, float *out, int N, int T,
                             int C, float eps, void *stream);
int rick_clip_attention_bwd_f32(const float *qkv, const float *g_out, float *stats, float *g_qkv, int N, int T, int heads, int D,
                                void *stream);
int rick_clip_input_bwd_f32(const float *g, float *out, int N, int H, int W, int S, int P, void *stream);

/* ---------------------------------------------------------------------------------------
 * DINOv2 — the ViT of DINOv2 (Oquab et al., 2023; rick_amd/dinov2.py): the final LayerNorm's class token, the feature space of
 * FD-DINOv2 (Stein et al., 2023).  Forward only.  It runs on the CLIP section's transformer (rick_clip_layernorm_f32 with
 * eps = 1e-6, rick_clip_attention_f32, rick_inc_conv_lin_f32 for the patch embedding and q/k/v) and adds what that lacks:
 * rick_inc_conv_vit_f32: rick_inc_conv_lin_f32's GEMM (same operands, same descriptor checks, same tiles, exact fp32 products,
 *   no split-K, nseg = 1) with the epilogue, in this order, v = acc + bias[col]; v = act(v); v = v * scale[col] if
 *   scale != NULL; v = v + res[m, col] if res != NULL.  Every operation is rounded on its own (nothing is contracted into an
 *   FMA).  act = 0 is the identity, act = 1 the exact GELU 0.5f * u * (1.f + erff(u * 0.70710678118654752f)) in that operation
 *   order: (0.5f * u) * (1.f + erff(.)).  It is finite for every finite u; erff is exactly +-1 from |u| = 6 on, so such a u
 *   comes back as u itself or as a zero.  scale is [Co] floats (LayerScale).  res follows rick_inc_conv_lin_f32's rules,
 *   res == dst[0] included.  Any other act returns 22.  A row's result does not depend on the other rows.
 * rick_vit_input_f32: rick_clip_input_f32 (the same kernel: resize rule, tap order, the affine's four correctly rounded
 *   operations, NHWC4 output) with mean and std of the affine as arguments; with CLIP's constants the bits of
 *   rick_clip_input_f32.  mean finite, std finite and > 0, else 22.
 * rick_vit_tokens_f32: patches [N, T - 1, C], cls [C], pos [T, C] -> out [N, T, C]: out[n, 0, :] = cls + pos[0],
 *   out[n, t, :] = patches[n, t - 1, :] + pos[t].  One fp32 add per element, 16-byte accesses, no LayerNorm.  C % 4 == 0,
 *   C <= 2048, 2 <= T <= 257, N T C / 1024 (the blocks of the launch) below 2^31, every pointer 16-byte aligned; else 22.
 * All of them: one writer per output element, fixed summation order, no atomics, no host branch on device data. */
int rick_inc_conv_vit_f32(const float *in, const float *wpk, const float *bias, const float *scale, const float *res, int act,
                          const rick_inc_conv *a, void *stream);
int rick_vit_input_f32(const float *x, float *out, int N, int H, int W, int S, float mean0, float mean1, float mean2, float std0,
                       float std1, float std2, void *stream);
int rick_vit_tokens_f32(const float *patches, const float *cls, const float *pos, float *out, int N, int T, int C, void *stream);

/* ---------------------------------------------------------------------------------------
 * Gram — the Gram matrix of a few very long rows and its adjoint (rick_amd/cdc.py): the device side of the cross-domain
 * distance-consistency loss, which needs the cosine similarity of whole generator feature maps between batch members.
 * x is B rows (1 <= B <= 8) of n >= 1 fp32 values, row stride n, 64-bit indices.  A row is an unordered bag of values: any
 * memory layout, as long as all rows of a call share it.
 * rick_gram_f32: G [B][B] fp64 (device) = x x^T, one pass over x.  Block s takes the elements [s L, (s + 1) L) of every row,
 *   L = 4096 ceil(n / (4096 * 1024)) (at most 1024 slices; the slicing depends on n only).  Thread l of the block owns the
 *   elements s L + 4 l + 1024 k + {0, 1, 2, 3} (k ascending) and keeps one fp32 fma chain per pair (i, j >= i) over them in
 *   that order; the 32, 16, ..., 1 xor butterfly adds the lanes, ((w0 + w1) + w2) + w3 the four waves, and the slice's
 *   B (B + 1) / 2 sums go to ws (fp32, rick_gram_workspace_bytes(B, n) bytes).  A second launch adds the slices in ascending
 *   order in fp64 and writes G[i][j] and G[j][i].  G is bit-identical from run to run and exactly symmetric, and G[i][j]
 *   depends on rows i and j alone: the Gram matrix of two rows by themselves equals the entries of any batch that holds them,
 *   bit for bit, wherever the rows lie.  Rows are read with 16-byte loads when x % 16 == 0 and n % 4 == 0, element by element
 *   otherwise (the same sums).
 * rick_rowmix_f32: y[k][t] = sum_m A[k][m] x[m][t], A [B][B] fp32 in device memory, y laid out like x (y != x).  Per element
 *   one fp32 chain A[k][0] x[0][t], then fma(A[k][m], x[m][t], .) for m = 1 .. B - 1: with A = I it returns x (finite values;
 *   -0 may come back as +0).  Reads B rows, writes B rows.
 * rick_xgram_f32 (rick_amd/dcl.py): the same for two row sets in separate allocations, a [Ba][n] and b [Bb][n] (1 <= Ba, Bb <= 8,
 *   both at row stride n, both in one memory layout): C [Ba][Bb] = <a_i, b_j>, na [Ba] = <a_i, a_i>, nb [Bb] = <b_j, b_j>, all
 *   fp64 (device), from ONE pass over both operands.  Slices, element -> thread map, fma chain order, butterfly, wave order and
 *   the ascending fp64 sum of the slices are rick_gram_f32's, so every entry is bit-identical to the entry rick_gram_f32 gives
 *   for the same two rows (C[i][j] = G[i][Ba + j] of the rows stacked) and depends on its two rows alone.  ws holds
 *   rick_xgram_workspace_bytes(Ba, Bb, n) bytes (-1 for sizes out of range).  16-byte loads only when a % 16 == 0, b % 16 == 0
 *   and n % 4 == 0; otherwise both operands are read element by element (the same sums).
 * rick_xrowmix_f32: its adjoint, y[k][t] = d[k] a[k][t] + sum_m M[k][m] b[m][t], M [Ba][Bb] and d [Ba] fp32 in device memory,
 *   y [Ba][n] laid out like a and overlapping neither a nor b.  Per element one fp32 chain d[k] a[k][t], then
 *   fma(M[k][m], b[m][t], .) for m = 0 .. Bb - 1: with M = 0, d = 1 it returns a, with d = 0 and M one-hot that row of b (finite
 *   values; -0 may come back as +0).  dA = gC B + 2 diag(gna) A is one call; dB the same call with the roles swapped and gC^T.
 * Both return RICK_EINVAL on null or misaligned pointers (4 bytes; 8 for the fp64 outputs), sizes out of range, or y aliasing.
 * No atomics, no host synchronisation, no allocation; every launch is on `stream` and can be captured. */
int64_t rick_gram_workspace_bytes(int B, int64_t n);
int rick_gram_f32(const float *x, int B, int64_t n, void *ws, double *G, void *stream);
int rick_rowmix_f32(const float *A, const float *x, float *y, int B, int64_t n, void *stream);
int64_t rick_xgram_workspace_bytes(int Ba, int Bb, int64_t n);
int rick_xgram_f32(const float *a, int Ba, const float *b, int Bb, int64_t n, void *ws, double *C, double *na, double *nb,
                   void *stream);
int rick_xrowmix_f32(const float *M, const float *d, const float *a, const float *b, float *y, int Ba, int Bb, int64_t n,
                     void *stream);

/* ---------------------------------------------------------------------------------------
 * EWC — the elastic-weight-consolidation penalty on the flat parameter buffers (rick_amd/ewc.py):
 *   L = sum_i F_i (theta_i - theta*_i)^2,   d(weight L) / d theta_i = 2 weight F_i (theta_i - theta*_i),
 * one pass over theta, anchor (theta*), fisher (F) and grad, n >= 0 fp32 values each at any 4-byte-aligned address; with every
 * F_i = 1 it is the L2-SP penalty.
 * rick_ewc_f32: for every i with (mask[i] & 3) == 0 (the bits of rick_masked_adam_f32; mask may be NULL: nothing is masked), in
 *   fp32:  d = theta[i] - anchor[i];  t = fisher[i] * d;  grad[i] = fmaf(2.f * weight, t, grad[i])
 *   — three roundings — and the fp64 term (double)fisher[i] * (double)d * (double)d (a rounded fp64 product, not contracted
 *   into the sum).  A masked element adds no term and its grad[i] is not written.  Block b of rick_ewc_blocks(n) =
 *   ceil(n / 4096) blocks of 256 threads owns the elements [4096 b, min(n, 4096 (b + 1))): the block -> element map depends on
 *   n alone, never on the device or a grid size (4096 = four 16-byte loads per thread and stream: enough in flight to stream at
 *   HBM rate, 5 800 blocks at the 256-px generator's size).  When the four streams share a 16-byte phase a block takes the 0 - 3
 *   elements in front of its first 16-byte boundary one by one (element j to thread j), then groups of four with 16-byte loads
 *   (group k to thread k % 256), then the 0 - 3 elements left (to threads 0 - 2); otherwise element j of the block goes to thread
 *   j % 256.  A thread adds its terms in ascending index order; the 32, 16, ..., 1 xor butterfly adds the lanes,
 *   ((w0 + w1) + w2) + w3 the four waves, and the block stores partials[b] (fp64, 8-byte aligned, rick_ewc_blocks(n) entries,
 *   every one written).  The sum is bit-identical from run to run for given addresses modulo 16.  n == 0 launches nothing.
 *   Moves 20 B per element, 21 B with a mask.
 * rick_ewc_finish_f64: out[0] = sum of partials[0 .. nblocks), one block: thread t adds partials[t], partials[t + 256], ... in
 *   ascending order, then the same butterfly and wave order — a function of nblocks alone.  nblocks == 0 writes 0.
 * No atomics, no host synchronisation, no allocation; both launches are on `stream` and can be captured. */
int64_t rick_ewc_blocks(int64_t n);
int rick_ewc_f32(const float *theta, const float *anchor, const float *fisher, float *grad, const uint8_t *mask, int64_t n,
                 float weight, double *partials, void *stream);
int rick_ewc_finish_f64(const double *partials, int64_t nblocks, double *out, void *stream);

/* ---------------------------------------------------------------------------------------
 * KML — kernel modulation of the frozen filters (AdAM's rank-constrained KML; rick_amd/kml.py).  A layer's weight is viewed as
 * W[co][ci][taps] (a row o is ci * taps contiguous floats); with factors a[co][R], b[ci][R] (R = rank, 1 ... 8), a snapshot W0
 * and a per-row flag:
 *   s[o,i] = sum_r a[o,r] b[i,r]      W^[o,i,t] = W0[o,i,t] (1 + s[o,i])       P[o,i] = sum_t G[o,i,t] W0[o,i,t]
 *   da[o,r] = sum_i P[o,i] b[i,r]     db[i,r] = sum_{o flagged} P[o,i] a[o,r]           (flagged rows only; da = 0 elsewhere)
 * W (the optimised slice of the flat parameter buffer), W0 and G (the flat gradient) are n floats in ONE layout; every a and b
 * lies in one factor buffer `fac` of nfac floats, da / db at the same offsets in `dfac`.  All layers of a network go in one
 * launch, driven by tables in DEVICE memory that the host builds when the flags change:
 *   layers[nlayers]   rick_kml_layer, below
 *   rows[nrows_total] per layer (from rows_off) its nrows flagged row indices, ascending
 *   blocks[nblocks]   pairs (layer, group): block k works on rows [group rg, min(nrows, (group + 1) rg)) of the layer's list,
 *                     rg = rick_kml_rows_per_group(ci, taps); sum of ngroups = nblocks
 *   rowflags[nflags]  per layer (from flags_off) co bytes, non-zero = flagged
 * A kernel checks every table entry it uses against n, nfac, nrows_total, npart and nflags and skips a layer that does not fit.
 * Work and traffic are proportional to the flagged rows: nblocks == 0 launches nothing in apply and grad.
 * rick_kml_apply_f32: writes W^ over the flagged rows of w, nothing else (no other row, no padding): s = a[o,0] b[i,0], then
 *   fmaf(a[o,r], b[i,r], s) for r = 1 .. R - 1; m = 1 + s; W^ = W0 * m — fp32, no contraction.  a = 0 returns W0 bit for bit.
 *   Reads W0, writes W^: 8 B per modulated element.
 * rick_kml_grad_f32 + rick_kml_grad_finish_f32: one pass over G and W0 of the flagged rows (8 B per modulated element); P is
 *   never stored.  P[o,i] = G[.,0] W0[.,0], then fmaf over t = 1 .. taps - 1.  A block owns whole rows.  The 256 threads of a
 *   block are `slots` groups of `lanes` threads, lanes = the power of two >= min(U, 256), U = the units of a row (four
 *   consecutive i when the vector form applies: grad, w0 and the layer's offset 16-byte aligned, ci % 4 == 0, taps 1 or 9 —
 *   4 taps floats as `taps` 16-byte loads; one i otherwise, element by element); row k of a group goes to slot k % slots, unit
 *   u of a row to lane u % lanes.  da[o,r]: a lane adds fmaf(P[o,i], b[i,r], .) over its i ascending, the lanes are added by
 *   the xor butterfly (lanes / 2, ..., 1; with 128 / 256 lanes the 2 / 4 waves in ascending order after it): it depends on row
 *   o and on b alone, whatever else is flagged.  db: the lane that owns i adds fmaf(P[o,i], a[o,r], .) over the rows of its
 *   slot ascending, the slots are added ascending, and the block writes partials[part_off + group R ci + r ci + i].  The finish
 *   launch adds a layer's partials in ascending group order into db[i,r] (0 for a layer without a flagged row) and writes 0
 *   into da of every unflagged row.  No atomics; every element of dfac inside a layer has exactly one writer; results are
 *   bit-identical from run to run (for given addresses modulo 16).  grad needs R * max(1024, max_ci) floats of LDS (<= 64 KB:
 *   RICK_EINVAL otherwise); max_co / max_ci: the largest co / ci of the table.
 * No host synchronisation, no allocation; every launch is on `stream`. */
typedef struct {
    int64_t off;              /* first element of the layer's weight in w / w0 / grad */
    int64_t a_off, b_off;     /* first element of a[co][R] / b[ci][R] in fac (da / db in dfac) */
    int64_t part_off;         /* first float of the layer's db partials: ngroups x R x ci */
    int32_t co, ci, taps;
    int32_t rows_off, nrows;  /* the layer's flagged rows in `rows` */
    int32_t rg, ngroups;      /* rows per group, ceil(nrows / rg) */
    int32_t flags_off;        /* first byte of the layer's row flags */
} rick_kml_layer;
int rick_kml_rows_per_group(int ci, int taps);
int rick_kml_apply_f32(const float *w0, float *w, int64_t n, const float *fac, int64_t nfac, int rank,
                       const rick_kml_layer *layers, int nlayers, const int32_t *rows, int64_t nrows_total,
                       const int32_t *blocks, int nblocks, void *stream);
int rick_kml_grad_f32(const float *grad, const float *w0, int64_t n, const float *fac, float *dfac, int64_t nfac,
                      float *partials, int64_t npart, int rank, const rick_kml_layer *layers, int nlayers,
                      const int32_t *rows, int64_t nrows_total, const int32_t *blocks, int nblocks, int max_ci, void *stream);
int rick_kml_grad_finish_f32(const float *partials, int64_t npart, float *dfac, int64_t nfac, const uint8_t *rowflags,
                             int64_t nflags, int rank, const rick_kml_layer *layers, int nlayers, int max_co, int max_ci,
                             void *stream);

/* ---------------------------------------------------------------------------------------
 * DiffAugment — Differentiable Augmentation (Zhao et al. 2020), policy color,translation,cutout (rick_amd/diffaug.py), for given
 * per-image draws.  Images are planar fp32 [N, 3, H, W], contiguous, H, W <= 16384, N <= 65535; the draws live in device memory
 * (`params`, N entries), so a captured graph replays with new draws after one copy into the block.  Brightness b, saturation s and
 * contrast c collapse to one affine map per image, and the whole operator is
 *   y = Cut . Shift . (L x + b 1),    L x = (c s) x + c (1 - s) mean_ch(x) + (1 - c) mean_all(x)        (L is self-adjoint)
 *   y[:, r, q] = (L x + b)[:, r + tr, q + tc] where that lies inside the image and (r, q) is outside the cut, else exactly 0;
 * a stage that is left out carries its identity: b = 0, s = 1, c = 1, tr = tc = 0, an empty cut.
 * rick_diffaug_fwd_f32: out = y (bias != 0) or its linear part (bias == 0: b taken as 0);
 * rick_diffaug_adj_f32: gx = L . Shift^T . Cut . gy, the transpose of the linear part.
 * Each is two launches on `stream`.  (1) Block k of ceil(3 H W / 4096) per image sums the elements [4096 k, 4096 (k + 1)) of the
 *   image's 3 H W — the adjoint only those of gy that the shift keeps and the cut does not zero — in fp64: a thread adds its
 *   elements in ascending order, the lanes by the 32, 16, ..., 1 xor butterfly, the waves as ((w0 + w1) + w2) + w3 (the order of
 *   rick_ewc_f32), into ws[n * blocks + k].  (2) Every block re-adds its image's partials in ascending order, forms
 *   mean = sum / (3 H W) and t = (1 - c) * mean + b in fp64 (no b in the adjoint and with bias == 0), rounds t once, and writes each
 *   output element once as  fmaf(c * s, v, fmaf(c * (1 - s), m, t)),  m = ((v0 + v1) + v2) / 3 in fp32, v the three channels of the
 *   source pixel (in the adjoint 0 where gy is not read); the forward writes exact zeros in the fill and the cut.
 * With W % 4 == 0 and 16-byte aligned images the launches use 16-byte stores and, where the column shift is a multiple of four
 * (launch 1: always), 16-byte loads.  No atomics; every output element and every partial has one writer; results are bit-identical
 * from run to run (for given addresses modulo 16) and an image's result does not depend on N or on the other images.  `ws`:
 * rick_diffaug_workspace_bytes() bytes, 8-byte aligned.  No host synchronisation, no allocation: capture-safe.
 * RICK_EINVAL for a null pointer, N, H or W below 1 or above the limits, a misaligned pointer; nothing is launched then.  The draws
 * are in device memory, which an entry point cannot read without a synchronisation: rick_diffaug_check_params checks a HOST copy of
 * the block before its upload — RICK_EINVAL for |tr| >= H, |tc| >= W, a cut bound outside [0, H] / [0, W], a NaN — and the kernels
 * force every field of a block they are given into the image, so no launch reads or writes outside its buffers. */
typedef struct {
    float b, s, c;
    int tr, tc;
    int r0, r1, c0, c1;       /* cut = rows [r0, r1) x cols [c0, c1), empty when r0 >= r1 or c0 >= c1 */
    int pad;
} rick_diffaug_param;         /* 40 B */
int64_t rick_diffaug_workspace_bytes(int N, int H, int W);
int rick_diffaug_check_params(const rick_diffaug_param *host_params, int N, int H, int W);
int rick_diffaug_fwd_f32(const float *x, const rick_diffaug_param *params, void *ws, float *out, int N, int H, int W, int bias,
                         void *stream);
int rick_diffaug_adj_f32(const float *gy, const rick_diffaug_param *params, void *ws, float *gx, int N, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------
 * SVD — FSGAN's singular-value adaptation (rick_amd/svd.py).  A layer's weight is viewed as W[co][ci][taps] (tap innermost).  For
 * every tap t the fp32 factors U[t][co][r] and Vt[t][r][ci], r = min(co, ci), of the source weight are frozen; the shift d[t][r] of
 * the singular values is learnt on top of a snapshot W0:
 *   W^[o,i,t] = W0[o,i,t] + sum_k (U[t,o,k] d[t,k]) Vt[t,k,i]         dd[t,k] = sum_o sum_i U[t,o,k] G[o,i,t] Vt[t,k,i]
 * W (the optimised slice of the flat parameter buffer), W0 and G (the flat gradient) are n floats in ONE layout; every U lies in
 * one buffer of nu floats, every Vt in one of nvt, every d in one of nd (dd at the same offsets in a buffer of its own).  All layers
 * of a network go in one launch, driven by tables the host builds once:
 *   layers[nlayers]    rick_svd_layer, below — in DEVICE memory for the kernels and the same bytes in HOST memory (layers_host)
 *                      for the entry points, which validate every record before anything is launched
 *   blocks[2 nblocks]  pairs (layer, tile) in device memory; a layer has rick_svd_apply_tiles() / rick_svd_grad_tiles() tiles,
 *                      numbered from 0, and the list holds each of them once: nblocks = their sum over the table
 * Products run on v_mfma_f32_32x32x2_f32: exact fp32 products, one fp32 fma chain per output element.
 * rick_svd_apply_f32: a block takes rows [32 a, 32 a + 32) x columns [32 s b, 32 s (b + 1)) of a layer with ALL its taps
 *   (s = 1 for taps >= 3, 2 for taps = 2, 4 for taps = 1; tile = a * ceil(ci / 32 s) + b).  The operand U[o,k] d[k] is rounded to
 *   fp32 once (while a wave turns its 32 x 16 chunk of U through LDS), k ascends from 0 to r - 1, the epilogue adds W0 and stores;
 *   the per-tap tiles are transposed through LDS so that
 *   each row's run of columns x taps floats is stored contiguously.  d = 0 returns W0 bit for bit.  Nothing outside the layers
 *   is written.
 * rick_svd_grad_f32 + rick_svd_grad_finish_f32: a block takes directions [32 s a, 32 s (a + 1)) x columns [32 b, 32 b + 32) with
 *   ALL taps (tile = a * ceil(ci / 32) + b): T[k,i] = sum_o U[t,o,k] G[o,i,t] with o ascending from 0 to co - 1, G staged in LDS
 *   32 rows at a time as the contiguous run it is in memory; then T[k,i] Vt[t,k,i], the 32 columns added by the 16, 8, 4, 2, 1 xor
 *   butterfly, into partials[part_off + (t r + k) ceil(ci / 32) + b].  T is never stored.  The finish launch adds the partials of
 *   (t, k) in ascending b into dd[d_off + t r + k].
 * Every summation order is a function of (co, ci, taps) alone: a layer's result does not depend on its place in the table, on
 * addresses or on the other layers, and is bit-identical from run to run.  Rows and columns beyond co, ci and r enter as zeros by
 * selection (clamped address inside the layer, value replaced).  No atomics, no allocation, no host synchronisation, one stream.
 * RICK_EINVAL, with nothing launched, for: a null or misaligned pointer; a data or table pointer that is not device memory; a
 * record with co, ci or taps < 1, taps > 16, r != min(co, ci), or an offset + extent past n / nu / nvt / nd / npart
 * (rick_svd_check_table, also exported); a block count that is not the table's tile count; w == w0. */
typedef struct {
    int64_t off;              /* first element of the layer's weight in w / w0 / grad */
    int64_t u_off, vt_off;    /* first element of U[taps][co][r] / Vt[taps][r][ci] */
    int64_t d_off;            /* first element of d[taps][r] (dd at the same offset) */
    int64_t part_off;         /* first float of the layer's partials: taps x r x ceil(ci / 32) = rick_svd_partials() */
    int32_t co, ci, taps, r;
    int32_t pad[2];
} rick_svd_layer;             /* 64 B */
int rick_svd_apply_tiles(int co, int ci, int taps);
int rick_svd_grad_tiles(int co, int ci, int taps);
int64_t rick_svd_partials(int co, int ci, int taps);
int rick_svd_check_table(const rick_svd_layer *layers_host, int nlayers, int64_t n, int64_t nu, int64_t nvt, int64_t nd,
                         int64_t npart);
int rick_svd_apply_f32(const float *w0, float *w, int64_t n, const float *u, int64_t nu, const float *vt, int64_t nvt,
                       const float *d, int64_t nd, const rick_svd_layer *layers, const rick_svd_layer *layers_host, int nlayers,
                       const int32_t *blocks, int nblocks, void *stream);
int rick_svd_grad_f32(const float *grad, int64_t n, const float *u, int64_t nu, const float *vt, int64_t nvt, float *partials,
                      int64_t npart, const rick_svd_layer *layers, const rick_svd_layer *layers_host, int nlayers,
                      const int32_t *blocks, int nblocks, void *stream);
int rick_svd_grad_finish_f32(const float *partials, int64_t npart, float *dd, int64_t nd, const rick_svd_layer *layers,
                             const rick_svd_layer *layers_host, int nlayers, void *stream);

/* ---------------------------------------------------------------------------------------
 * Patch head — the head of CDC's patch-level discriminator (rick_amd/patchd.py): ConvLayer(C, 1, 3) of the reference
 * (model_probe_tune.py:595-641: EqualConv2d :101-136 + FusedLeakyReLU, op/fused_act.py:73-82) on a tapped feature map, as thin
 * HBM-bound kernels instead of an implicit GEMM with one live output column.  x is the map in channels-last memory [N][H][W][C],
 * w the weight [1][C][3][3] (w[c][t] at 9 c + t, t = 3 ky + kx), b the bias [1] in DEVICE memory, out / g the logit map and its
 * gradient [N][H][W]:
 *   z[n,y,x]    = b + sum_c sum_t (wscale w[c,t]) X[n,c,y+ky-1,x+kx-1]          (zero outside; correlation, as F.conv2d)
 *   out         = gain (z > 0 ? z : slope z)
 *   gz          = g gain (out > 0 ? 1 : slope)          (the sign of the STORED output, as fused_act's backward takes it)
 *   gb          = sum gz
 *   gw[c,t]     = wscale sum_{n,y,x} gz[n,y,x] X[n,c,y+ky-1,x+kx-1]
 *   gX[n,c,u,v] = sum_t (wscale w[c,t]) gz[n,u-ky+1,v-kx+1]
 * C % 4 == 0, 4 <= C <= 2048, N, H, W >= 1, N H W C < 2^31; x, w and gx 16-byte aligned, ws 8-byte, everything else 4-byte.
 * rick_patch_head_fwd_f32: one launch, one wave per output pixel, 8 pixels per block.  Lane l owns the channels
 *   4 l + 256 k + {0, 1, 2, 3}, k ascending, and keeps one fp32 fma chain per tap over them in that order (16-byte loads; the
 *   9 C scaled weights are rounded once and staged per block in LDS); the lane adds its nine chains in ascending tap order (a tap
 *   outside the image loads nothing and stays the chain's initial zero), the 32, 16, ..., 1 xor butterfly adds the lanes, then
 *   b + sum.  The order is a function of C and the pixel's place in its own image: out[n] does not depend on N or on n.
 * rick_patch_head_bwd_f32: one pass over x.  Block (slab, chunk) takes the pixels [slab L, (slab + 1) L) of the flattened
 *   N H W map, L = 32 ceil(N H W / (32 * 512)) (at most 512 slabs), and the channels [256 chunk, 256 chunk + 256); lane l owns
 *   four channels, wave v the pixels slab L + v + 4 k, k ascending.  gz of the nine neighbours of a pixel is formed from g and out
 *   on the fly.  gx (may be NULL: not computed) = one fp32 chain over the taps ascending, (wscale w[c,0]) gz_0 first — gX[n]
 *   depends on image n alone.  The weight and bias sums: one fp32 fma chain per (tap, channel) and wave over its pixels, the four
 *   waves added ((w0 + w1) + w2) + w3 (the bias sum in fp64 throughout), into ws (rick_patch_head_workspace_bytes(N, H, W, C)
 *   bytes, 8-byte aligned; -1 for sizes out of range): nslabs doubles of bias sums, then the floats [slab][t C + c].  Every
 *   entry of ws is written.
 * rick_patch_head_bwd_finish_f32: gw[c,t] = (float)(wscale * sum over the slabs, ascending, in fp64), gb = (float)(the same sum of
 *   the bias partials).  The partition is a function of (N, H, W, C) alone; results are bit-identical from run to run.
 * RICK_EINVAL, before any HIP call, for a null (but gx) or misaligned pointer, a size out of range, gx == x.
 * No atomics, no host synchronisation, no allocation; every launch is on `stream`. */
int64_t rick_patch_head_workspace_bytes(int N, int H, int W, int C);
int rick_patch_head_fwd_f32(const float *x, const float *w, const float *b, float *out, int N, int H, int W, int C, float wscale,
                            float slope, float gain, void *stream);
int rick_patch_head_bwd_f32(const float *x, const float *w, const float *g, const float *out, float *gx, void *ws, int N, int H,
                            int W, int C, float wscale, float slope, float gain, void *stream);
int rick_patch_head_bwd_finish_f32(const void *ws, float *gw, float *gb, int N, int H, int W, int C, float wscale, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RICK_HIP_H */
