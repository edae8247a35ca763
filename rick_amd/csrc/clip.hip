// CLIP ViT image tower (Radford et al., 2021), forward and the data gradient (frozen weights) — include/rick_hip.h "CLIP".
//
// The five GEMMs of a layer run on rick_inc_conv_lin_f32 (inception.hip), forward and, on transposed operands, backward.  This
// file holds what a transformer needs around them: the bicubic input, token assembly fused with ln_pre, LayerNorm, multi-head
// attention and QuickGELU as a kernel of its own, each with its adjoint with respect to the data.  Activations are fp32 rows
// [tokens][width].  Every output element is written by exactly one thread with a fixed summation order: no atomics, run-to-run
// bit-identical, and an image's values do not depend on the other images of the call.
//
// The text tower (rick_amd/cliptext.py, forward only) shares the GEMMs, the LayerNorm and the attention kernel, the last with
// a causal mask as a compile-time flag, and adds the token-embedding lookup and a LayerNorm of rows picked by index (ln_final
// on each prompt's EOT row).
//
// DINOv2's ViT (rick_amd/dinov2.py, forward only) shares the input kernel (the affine's constants are kernel arguments), the
// GEMMs, the LayerNorm and the attention kernel, and adds the stem without ln_pre (vit_tokens_kernel).
#include <float.h>

#include "common.h"

#define CL_MAXJ 8              // a row of up to 2048 columns in registers: lane l holds columns 4 l + 256 j, j < 8
#define CL_MAXC (256 * CL_MAXJ)
#define CL_MAXT 257            // ViT-L/14 at 224
#define CL_KEYS ((CL_MAXT + 63) / 64)

// ---- input: bicubic resize (F.interpolate, mode='bicubic', align_corners=False, no antialias) + CLIP's affine, NCHW -> NHWC4 --
// ATen's cubic convolution, A = -0.75: weights of the taps floor(s) - 1 .. floor(s) + 2 at t = s - floor(s).  At t = 0 they
// are exactly (0, 1, 0, 0) in these forms, with or without contraction into FMAs.
__device__ __forceinline__ float cl_cubic1(float x) { return ((-0.75f + 2.f) * x - (-0.75f + 3.f)) * x * x + 1.f; }
__device__ __forceinline__ float cl_cubic2(float x) { return ((-0.75f * x - 5.f * -0.75f) * x + 8.f * -0.75f) * x - 4.f * -0.75f; }
__device__ __forceinline__ void cl_cubic_taps(int dst, float scale, int n_in, int idx[4], float w[4]) {
    const float s = __fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f);     // area_pixel_compute_source_index, cubic: no clamp at 0
    const float fl = floorf(s), t = s - fl;
    const int i0 = (int)fl;
    w[0] = cl_cubic2(t + 1.f);
    w[1] = cl_cubic1(t);
    w[2] = cl_cubic1(1.f - t);
    w[3] = cl_cubic2(2.f - t);
#pragma unroll
    for (int k = 0; k < 4; k++) idx[k] = min(max(i0 - 1 + k, 0), n_in - 1);   // border: clamped source indices
}

// mean and std of the affine arrive as kernel arguments: CLIP's constants from rick_clip_input_f32, the caller's from
// rick_vit_input_f32.  The four operations are correctly rounded, so a constant gives the same bits either way.
struct cl_affine {
    float mean[3], std[3];
};
__global__ __launch_bounds__(256) void clip_input_kernel(const float *__restrict__ x, float *__restrict__ out, int N, int H, int W,
                                                         int S, float sh, float sw, cl_affine k) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * S * S) return;
    const int ox = (int)(i % S), oy = (int)((i / S) % S), n = (int)(i / ((int64_t)S * S));
    int iy[4], ix[4];
    float wy[4], wx[4];
    cl_cubic_taps(oy, sh, H, iy, wy);
    cl_cubic_taps(ox, sw, W, ix, wx);
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *p = x + ((int64_t)n * 3 + c) * H * W;
        float v = 0.f;
#pragma unroll
        for (int a = 0; a < 4; a++) {                         // rows in tap order; within a row the four taps in order
            const float *q = p + (int64_t)iy[a] * W;
            float row = wx[0] * q[ix[0]];
#pragma unroll
            for (int b = 1; b < 4; b++) row = fmaf(wx[b], q[ix[b]], row);
            v = a == 0 ? wy[0] * row : fmaf(wy[a], row, v);
        }
        // (v * 0.5 + 0.5 - mean) / std: four correctly rounded fp32 operations, as torch evaluates the expression
        r[c] = __fdiv_rn(__fsub_rn(__fadd_rn(__fmul_rn(v, 0.5f), 0.5f), k.mean[c]), k.std[c]);
    }
    reinterpret_cast<float4 *>(out)[i] = make_float4(r[0], r[1], r[2], 0.f);
}

// ---- LayerNorm of one row held in registers ---------------------------------------------------------------------------------
// Lane l owns columns 4 l + 256 j.  Pass 1: the lane adds its columns in ascending order, wave_sum (xor butterfly 32 .. 1),
// mean = sum / C.  Pass 2: the lane adds fmaf(d, d, .) of d = x - mean in the same order, wave_sum, var = sum / C (biased).
// y = fmaf(d * rstd, w, b), rstd = 1 / sqrtf(var + eps).  Never E[x^2] - mean^2.
__device__ __forceinline__ void cl_layernorm_row(const float4 (&x)[CL_MAXJ], int C, int lane, const float *__restrict__ w,
                                                 const float *__restrict__ b, float eps, float *__restrict__ out) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++)
        if (4 * lane + 256 * j < C) {
            s += x[j].x;
            s += x[j].y;
            s += x[j].z;
            s += x[j].w;
        }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++)
        if (4 * lane + 256 * j < C) {
            const float dx = x[j].x - mean, dy = x[j].y - mean, dz = x[j].z - mean, dw = x[j].w - mean;
            q = fmaf(dx, dx, q);
            q = fmaf(dy, dy, q);
            q = fmaf(dz, dz, q);
            q = fmaf(dw, dw, q);
        }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        if (c < C) {
            const float4 wv = *reinterpret_cast<const float4 *>(w + c), bv = *reinterpret_cast<const float4 *>(b + c);
            float4 y;
            y.x = fmaf((x[j].x - mean) * rstd, wv.x, bv.x);
            y.y = fmaf((x[j].y - mean) * rstd, wv.y, bv.y);
            y.z = fmaf((x[j].z - mean) * rstd, wv.z, bv.z);
            y.w = fmaf((x[j].w - mean) * rstd, wv.w, bv.w);
            *reinterpret_cast<float4 *>(out + c) = y;
        }
    }
}

// rows [R, C] with a row stride ldx -> out [R, C] compact.  One wave per row, four rows per block.
__global__ __launch_bounds__(256) void clip_layernorm_kernel(const float *__restrict__ in, int64_t ldx, const float *__restrict__ w,
                                                             const float *__restrict__ b, float *__restrict__ out, int R, int C,
                                                             float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;                                     // wave-uniform
    const float *p = in + (int64_t)row * ldx;
    float4 x[CL_MAXJ];
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        x[j] = c < C ? *reinterpret_cast<const float4 *>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    cl_layernorm_row(x, C, lane, w, b, eps, out + (int64_t)row * C);
}

// tokens [N, T, C] = ln_pre([class_embedding ; patches [N, T - 1, C]] + positional_embedding [T, C]): one wave per token
__global__ __launch_bounds__(256) void clip_tokens_kernel(const float *__restrict__ patches, const float *__restrict__ cls,
                                                          const float *__restrict__ pos, const float *__restrict__ w,
                                                          const float *__restrict__ b, float *__restrict__ out, int N, int T, int C,
                                                          float eps) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)N * T) return;                        // wave-uniform
    const int t = (int)(row % T);
    const int64_t n = row / T;
    const float *p = t == 0 ? cls : patches + (n * (T - 1) + (t - 1)) * C;
    const float *e = pos + (int64_t)t * C;
    float4 x[CL_MAXJ];
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const float4 a = *reinterpret_cast<const float4 *>(p + c), d = *reinterpret_cast<const float4 *>(e + c);
            x[j] = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
        }
    }
    cl_layernorm_row(x, C, lane, w, b, eps, out + row * C);
}

// ---- attention ----------------------------------------------------------------------------------------------------------------
// One block per (image, head); K [T][D + 1] (the odd stride spreads the lanes' key rows over the banks) and V [T][D] of that
// head are staged once in LDS.  Wave w takes the query rows w, w + 4, ...:
//   score[k] = (sum_c q[c] K[k][c], one fmaf chain over c ascending from 0) * (1 / sqrt(D)), lane l owning keys l + 64 j;
//   m = max (per lane over j, then the xor butterfly); e[k] = expf(score[k] - m);
//   den = per lane e over j ascending, then wave_sum; p[k] = e[k] / den (F.softmax's form), through LDS to every lane;
//   out[c] = sum_k p[k] V[k][c], one fmaf chain over k ascending from 0, lane c < D.
// The two barriers per row are taken by all four waves (the row loop has one trip count for the block).
__device__ __forceinline__ float cl_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}

static size_t cl_attention_lds(int T, int D) { return sizeof(float) * ((size_t)T * D + (size_t)T * (D + 1) + 4 * (size_t)((T + 3) & ~3)); }

// CAUSAL (the text tower): query row i sees the keys k <= i.  With lim = i + 1 in the place of T in everything a row does, row i
// runs the arithmetic of the non-causal kernel on the first i + 1 tokens, operation for operation: the slots k >= lim hold
// -inf before the maximum and an exact 0.f in the denominator, as the slots k >= T do there, and the P V chain ends at k = i.
// So row i is bit-identical to row i of rick_clip_attention_f32 on the first i + 1 tokens.  The score chains of the keys
// behind the diagonal are not run (a 64-key slot that lies wholly behind it is skipped by the whole wave).
template <int D, bool CAUSAL>
__global__ __launch_bounds__(256) void clip_attention_kernel(const float *__restrict__ qkv, float *__restrict__ out, int T, int Wd,
                                                             int heads) {
    extern __shared__ __attribute__((aligned(16))) float cl_lds[];
    constexpr int KS = D + 1;
    constexpr float scale = D == 16 ? 0.25f : D == 64 ? 0.125f : 0.17677669529663687f;      // 1 / sqrt(D)
    const int Tp = (T + 3) & ~3;
    float *Vs = cl_lds, *Ks = Vs + T * D, *Ps = Ks + T * KS;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads;
    const int64_t ld = 3 * (int64_t)Wd;
    const float *base = qkv + (int64_t)n * T * ld + h * D;
    for (int i = t; i < T * (D / 4); i += 256) {
        const int k = i / (D / 4), c = 4 * (i % (D / 4));
        const float4 kv = *reinterpret_cast<const float4 *>(base + k * ld + Wd + c);
        const float4 vv = *reinterpret_cast<const float4 *>(base + k * ld + 2 * Wd + c);
        Ks[k * KS + c] = kv.x;
        Ks[k * KS + c + 1] = kv.y;
        Ks[k * KS + c + 2] = kv.z;
        Ks[k * KS + c + 3] = kv.w;
        *reinterpret_cast<float4 *>(Vs + k * D + c) = vv;
    }
    __syncthreads();
    float *pw = Ps + w * Tp;
    for (int r0 = 0; r0 < T; r0 += 4) {
        const int row = r0 + w;
        const bool ok = row < T;                              // wave-uniform
        const int lim = CAUSAL ? row + 1 : T;                 // the keys this row sees: [0, lim), wave-uniform
        if (ok) {
            float4 q[D / 4];
#pragma unroll
            for (int c = 0; c < D / 4; c++) q[c] = *reinterpret_cast<const float4 *>(base + row * ld + 4 * c);
            float s[CL_KEYS], mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++) {
                const int k = lane + 64 * j;
                s[j] = -INFINITY;
                if (k < lim) {
                    const float *kr = Ks + k * KS;
                    float a = 0.f;
#pragma unroll
                    for (int c = 0; c < D / 4; c++) {
                        a = fmaf(q[c].x, kr[4 * c], a);
                        a = fmaf(q[c].y, kr[4 * c + 1], a);
                        a = fmaf(q[c].z, kr[4 * c + 2], a);
                        a = fmaf(q[c].w, kr[4 * c + 3], a);
                    }
                    s[j] = a * scale;
                }
                mx = fmaxf(mx, s[j]);
            }
            mx = cl_wave_max(mx);
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++) {
                s[j] = lane + 64 * j < lim ? expf(s[j] - mx) : 0.f;
                den += s[j];
            }
            den = wave_sum(den);
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++)
                if (lane + 64 * j < lim) pw[lane + 64 * j] = s[j] / den;
        }
        __syncthreads();
        if (ok && lane < D) {
            float o = 0.f;
            for (int k = 0; k < lim; k++) o = fmaf(pw[k], Vs[k * D + lane], o);
            out[((int64_t)n * T + row) * Wd + h * D + lane] = o;
        }
        __syncthreads();
    }
}

// The 160 KB limit is raised once per kernel variant and device: the flags of RICK_LDS160_ONCE belong to its expansion site,
// and this function template is one expansion site per (D, CAUSAL).
template <int D, bool CAUSAL>
static void cl_attention_launch(const float *qkv, float *out, int N, int T, int Wd, int heads, hipStream_t st) {
    const size_t lds = cl_attention_lds(T, D);
    if (lds > 64 * 1024) RICK_LDS160_ONCE((clip_attention_kernel<D, CAUSAL>));
    hipLaunchKernelGGL((clip_attention_kernel<D, CAUSAL>), dim3((unsigned)(N * heads)), dim3(256), lds, st, qkv, out, T, Wd, heads);
}

// ---- the text tower's two row kernels ---------------------------------------------------------------------------------------------
// out[n, t, :] = table[ids[n, t]] + pos[t]: one thread per four columns, one fp32 add per element, 16-byte accesses.  The host
// validates the ids before upload; the kernel still forces an id into [0, V) so that no launch reads outside the table.
__global__ __launch_bounds__(256) void clip_text_tokens_kernel(const int *__restrict__ ids, const float *__restrict__ table,
                                                               const float *__restrict__ pos, float *__restrict__ out, int64_t total,
                                                               int T, int V, int C4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;                // over [N T][C / 4]
    if (i >= total) return;
    const int64_t row = i / C4;
    const int c = (int)(i % C4), t = (int)(row % T);
    const int id = min(max(ids[row], 0), V - 1);
    const float4 a = reinterpret_cast<const float4 *>(table)[(int64_t)id * C4 + c];
    const float4 d = reinterpret_cast<const float4 *>(pos)[(int64_t)t * C4 + c];
    reinterpret_cast<float4 *>(out)[i] = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
}

// The stem of a ViT without ln_pre (DINOv2): out[n, 0, :] = cls + pos[0], out[n, t, :] = patches[n, t - 1, :] + pos[t].  The
// element -> thread map and the one fp32 add of clip_text_tokens_kernel.
__global__ __launch_bounds__(256) void vit_tokens_kernel(const float *__restrict__ patches, const float *__restrict__ cls,
                                                         const float *__restrict__ pos, float *__restrict__ out, int64_t total, int T,
                                                         int C4) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;                // over [N T][C / 4]
    if (i >= total) return;
    const int64_t row = i / C4, n = row / T;
    const int c = (int)(i % C4), t = (int)(row % T);
    const float4 a = t == 0 ? reinterpret_cast<const float4 *>(cls)[c]
                            : reinterpret_cast<const float4 *>(patches)[(n * (T - 1) + (t - 1)) * C4 + c];
    const float4 d = reinterpret_cast<const float4 *>(pos)[(int64_t)t * C4 + c];
    reinterpret_cast<float4 *>(out)[i] = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
}

// LayerNorm of the rows idx[r] of in (rows of C floats, compact) -> out [R, C]: clip_layernorm_kernel with the row number read
// from idx, the same loads into the same registers and the same cl_layernorm_row, so the same bits as that kernel on the rows
// gathered contiguously.  Neither the entry (idx is device memory, and there is no row count) nor the kernel can bound an index
// from above: the host checks idx against the rows of `in` before upload, and an index past them reads out of bounds.
__global__ __launch_bounds__(256) void clip_layernorm_rows_kernel(const float *__restrict__ in, const int *__restrict__ idx,
                                                                  const float *__restrict__ w, const float *__restrict__ b,
                                                                  float *__restrict__ out, int R, int C, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;                                     // wave-uniform
    const float *p = in + (int64_t)max(idx[row], 0) * C;
    float4 x[CL_MAXJ];
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        x[j] = c < C ? *reinterpret_cast<const float4 *>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    cl_layernorm_row(x, C, lane, w, b, eps, out + (int64_t)row * C);
}

// ---- QuickGELU as a kernel of its own, and its derivative -----------------------------------------------------------------------
// The differentiable forward keeps the pre-activation u, so c_fc runs with the identity epilogue and this kernel follows: the
// same five fp32 operations as the act = 1 epilogue of rick_inc_conv_lin_f32 (inc_quickgelu, inception.hip), the same bits.
__device__ __forceinline__ float cl_sigmoid1702(float u) { return __fdiv_rn(1.f, __fadd_rn(1.f, expf(-__fmul_rn(1.702f, u)))); }

__global__ __launch_bounds__(256) void clip_quickgelu_kernel(const float *u, float *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = __fmul_rn(u[i], cl_sigmoid1702(u[i]));
}

// out = g * d/du (u s(u)) = g * (s + 1.702 u s (1 - s)); out may be g
__global__ __launch_bounds__(256) void clip_quickgelu_bwd_kernel(const float *__restrict__ u, const float *g, float *out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = u[i], s = cl_sigmoid1702(v);
    out[i] = g[i] * (s + 1.702f * v * s * (1.f - s));
}

// ---- LayerNorm, data gradient ---------------------------------------------------------------------------------------------------
// The row's mean and rstd are recomputed from the stored input in cl_layernorm_row's order.  With xhat = (x - mean) rstd and
// gw = g w: m1 = sum gw / C (lane order as pass 1), m2 = sum gw xhat / C (one fmaf chain per lane), then
// dx = rstd (gw - m1 - xhat m2) [+ add].  add may be out (read and written by the same thread).
__device__ __forceinline__ void cl_layernorm_bwd_row(const float4 (&x)[CL_MAXJ], int C, int lane, const float *__restrict__ w,
                                                     const float *__restrict__ g, const float *add, float eps, float *out) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++)
        if (4 * lane + 256 * j < C) {
            s += x[j].x;
            s += x[j].y;
            s += x[j].z;
            s += x[j].w;
        }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++)
        if (4 * lane + 256 * j < C) {
            const float dx = x[j].x - mean, dy = x[j].y - mean, dz = x[j].z - mean, dw = x[j].w - mean;
            q = fmaf(dx, dx, q);
            q = fmaf(dy, dy, q);
            q = fmaf(dz, dz, q);
            q = fmaf(dw, dw, q);
        }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)C + eps);
    float4 gw[CL_MAXJ];
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        gw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const float4 wv = *reinterpret_cast<const float4 *>(w + c), gv = *reinterpret_cast<const float4 *>(g + c);
            gw[j] = make_float4(gv.x * wv.x, gv.y * wv.y, gv.z * wv.z, gv.w * wv.w);
            a += gw[j].x;
            a += gw[j].y;
            a += gw[j].z;
            a += gw[j].w;
            b = fmaf(gw[j].x, (x[j].x - mean) * rstd, b);
            b = fmaf(gw[j].y, (x[j].y - mean) * rstd, b);
            b = fmaf(gw[j].z, (x[j].z - mean) * rstd, b);
            b = fmaf(gw[j].w, (x[j].w - mean) * rstd, b);
        }
    }
    const float m1 = wave_sum(a) / (float)C, m2 = wave_sum(b) / (float)C;
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        if (c < C) {
            float4 d;
            d.x = rstd * (gw[j].x - m1 - (x[j].x - mean) * rstd * m2);
            d.y = rstd * (gw[j].y - m1 - (x[j].y - mean) * rstd * m2);
            d.z = rstd * (gw[j].z - m1 - (x[j].z - mean) * rstd * m2);
            d.w = rstd * (gw[j].w - m1 - (x[j].w - mean) * rstd * m2);
            if (add) {
                const float4 r = *reinterpret_cast<const float4 *>(add + c);
                d = make_float4(d.x + r.x, d.y + r.y, d.z + r.z, d.w + r.w);
            }
            *reinterpret_cast<float4 *>(out + c) = d;
        }
    }
}

// rows x [R, C] (stride ldx), g [R, C] (stride ldg) -> out [R, C] (stride ldo; add laid out like out).  One wave per row.
__global__ __launch_bounds__(256) void clip_layernorm_bwd_kernel(const float *__restrict__ in, int64_t ldx, const float *__restrict__ w,
                                                                 const float *__restrict__ g, int64_t ldg, const float *add,
                                                                 float *out, int64_t ldo, int R, int C, float eps) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= R) return;                                     // wave-uniform
    const float *p = in + (int64_t)row * ldx;
    float4 x[CL_MAXJ];
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        x[j] = c < C ? *reinterpret_cast<const float4 *>(p + c) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    cl_layernorm_bwd_row(x, C, lane, w, g + (int64_t)row * ldg, add ? add + (int64_t)row * ldo : nullptr, eps, out + (int64_t)row * ldo);
}

// The adjoint of clip_tokens_kernel with respect to the patches: ln_pre's data gradient on [patches + pos] rows t >= 1,
// g [N, T, C] -> out [N, T - 1, C].  The class row's gradient has no consumer (the class embedding is frozen).
__global__ __launch_bounds__(256) void clip_tokens_bwd_kernel(const float *__restrict__ patches, const float *__restrict__ pos,
                                                              const float *__restrict__ w, const float *__restrict__ g,
                                                              float *__restrict__ out, int N, int T, int C, float eps) {
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= (int64_t)N * (T - 1)) return;                  // wave-uniform
    const int t = (int)(row % (T - 1)) + 1;
    const int64_t n = row / (T - 1);
    const float *p = patches + row * C, *e = pos + (int64_t)t * C;
    float4 x[CL_MAXJ];
#pragma unroll
    for (int j = 0; j < CL_MAXJ; j++) {
        const int c = 4 * lane + 256 * j;
        x[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < C) {
            const float4 a = *reinterpret_cast<const float4 *>(p + c), d = *reinterpret_cast<const float4 *>(e + c);
            x[j] = make_float4(a.x + d.x, a.y + d.y, a.z + d.z, a.w + d.w);
        }
    }
    cl_layernorm_bwd_row(x, C, lane, w, g + (n * T + t) * C, nullptr, eps, out + row * C);
}

// ---- attention, data gradient ---------------------------------------------------------------------------------------------------
// FlashAttention-2's split, nothing of size T x T in memory, every sum in a fixed order.  With p = softmax row i (recomputed
// with clip_attention_kernel's chain: the same bits), dP_ij = go_i . v_j (fmaf chain over c ascending), delta_i = sum_j p_ij
// dP_ij (per lane over its keys ascending, then the butterfly) and dS_ij = p_ij (dP_ij - delta_i):
//   launch one, a wave per query row, K and V of the head in LDS: dQ_i = scale sum_j dS_ij k_j (fmaf chain, j ascending); the
//     row's maximum, denominator and delta go to stats [N, heads, T, 3];
//   launch two, a wave per key row, Q and go of the head in LDS (and the head's stats): p_ij = expf(s_ij - max_i) / den_i, the
//     same bits again; dV_j = sum_i p_ij go_i and dK_j = scale sum_i dS_ij q_i, fmaf chains with i ascending.
// Both row strides are D + 1.  LDS at T = 257, D = 64: 138 KB and 145 KB.
static size_t cl_attention_bwd_q_lds(int T, int D) { return sizeof(float) * (2 * (size_t)T * (D + 1) + 4 * (size_t)((T + 3) & ~3)); }
static size_t cl_attention_bwd_kv_lds(int T, int D) {
    return sizeof(float) * (2 * (size_t)T * (D + 1) + 3 * (size_t)T + 8 * (size_t)((T + 3) & ~3));
}

template <int D>
__global__ __launch_bounds__(256) void clip_attention_bwd_q_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
                                                                   float *__restrict__ stats, float *__restrict__ gqkv, int T,
                                                                   int Wd, int heads) {
    extern __shared__ __attribute__((aligned(16))) float cl_lds[];
    constexpr int KS = D + 1;
    constexpr float scale = D == 16 ? 0.25f : D == 64 ? 0.125f : 0.17677669529663687f;      // 1 / sqrt(D)
    const int Tp = (T + 3) & ~3;
    float *Vs = cl_lds, *Ks = Vs + T * KS, *Ps = Ks + T * KS;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads;
    const int64_t ld = 3 * (int64_t)Wd;
    const float *base = qkv + (int64_t)n * T * ld + h * D;
    const float *gbase = go + (int64_t)n * T * Wd + h * D;
    for (int i = t; i < T * (D / 4); i += 256) {
        const int k = i / (D / 4), c = 4 * (i % (D / 4));
        const float4 kv = *reinterpret_cast<const float4 *>(base + k * ld + Wd + c);
        const float4 vv = *reinterpret_cast<const float4 *>(base + k * ld + 2 * Wd + c);
        Ks[k * KS + c] = kv.x;
        Ks[k * KS + c + 1] = kv.y;
        Ks[k * KS + c + 2] = kv.z;
        Ks[k * KS + c + 3] = kv.w;
        Vs[k * KS + c] = vv.x;
        Vs[k * KS + c + 1] = vv.y;
        Vs[k * KS + c + 2] = vv.z;
        Vs[k * KS + c + 3] = vv.w;
    }
    __syncthreads();
    float *pw = Ps + w * Tp;
    for (int r0 = 0; r0 < T; r0 += 4) {
        const int row = r0 + w;
        const bool ok = row < T;                              // wave-uniform
        if (ok) {
            float4 q[D / 4], g[D / 4];
#pragma unroll
            for (int c = 0; c < D / 4; c++) {
                q[c] = *reinterpret_cast<const float4 *>(base + row * ld + 4 * c);
                g[c] = *reinterpret_cast<const float4 *>(gbase + (int64_t)row * Wd + 4 * c);
            }
            float s[CL_KEYS], dp[CL_KEYS], mx = -INFINITY;
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++) {
                const int k = lane + 64 * j;
                s[j] = -INFINITY;
                dp[j] = 0.f;
                if (k < T) {
                    const float *kr = Ks + k * KS, *vr = Vs + k * KS;
                    float a = 0.f, b = 0.f;
#pragma unroll
                    for (int c = 0; c < D / 4; c++) {
                        a = fmaf(q[c].x, kr[4 * c], a);
                        a = fmaf(q[c].y, kr[4 * c + 1], a);
                        a = fmaf(q[c].z, kr[4 * c + 2], a);
                        a = fmaf(q[c].w, kr[4 * c + 3], a);
                        b = fmaf(g[c].x, vr[4 * c], b);
                        b = fmaf(g[c].y, vr[4 * c + 1], b);
                        b = fmaf(g[c].z, vr[4 * c + 2], b);
                        b = fmaf(g[c].w, vr[4 * c + 3], b);
                    }
                    s[j] = a * scale;
                    dp[j] = b;
                }
                mx = fmaxf(mx, s[j]);
            }
            mx = cl_wave_max(mx);
            float den = 0.f;
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++) {
                s[j] = lane + 64 * j < T ? expf(s[j] - mx) : 0.f;
                den += s[j];
            }
            den = wave_sum(den);
            float dl = 0.f;
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++) {
                s[j] = s[j] / den;                            // p; 0 beyond T
                dl = fmaf(s[j], dp[j], dl);
            }
            dl = wave_sum(dl);
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++)
                if (lane + 64 * j < T) pw[lane + 64 * j] = s[j] * (dp[j] - dl);
            if (lane < 3) stats[(((int64_t)n * heads + h) * T + row) * 3 + lane] = lane == 0 ? mx : lane == 1 ? den : dl;
        }
        __syncthreads();
        if (ok && lane < D) {
            float o = 0.f;
            for (int k = 0; k < T; k++) o = fmaf(pw[k], Ks[k * KS + lane], o);
            gqkv[((int64_t)n * T + row) * ld + h * D + lane] = o * scale;
        }
        __syncthreads();
    }
}

template <int D>
__global__ __launch_bounds__(256) void clip_attention_bwd_kv_kernel(const float *__restrict__ qkv, const float *__restrict__ go,
                                                                    const float *__restrict__ stats, float *__restrict__ gqkv, int T,
                                                                    int Wd, int heads) {
    extern __shared__ __attribute__((aligned(16))) float cl_lds[];
    constexpr int KS = D + 1;
    constexpr float scale = D == 16 ? 0.25f : D == 64 ? 0.125f : 0.17677669529663687f;      // 1 / sqrt(D)
    const int Tp = (T + 3) & ~3;
    float *Qs = cl_lds, *Gs = Qs + T * KS, *St = Gs + T * KS, *Ps = St + 3 * T;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int n = blockIdx.x / heads, h = blockIdx.x % heads;
    const int64_t ld = 3 * (int64_t)Wd;
    const float *base = qkv + (int64_t)n * T * ld + h * D;
    const float *gbase = go + (int64_t)n * T * Wd + h * D;
    const float *sbase = stats + ((int64_t)n * heads + h) * T * 3;
    for (int i = t; i < T * (D / 4); i += 256) {
        const int k = i / (D / 4), c = 4 * (i % (D / 4));
        const float4 qv = *reinterpret_cast<const float4 *>(base + k * ld + c);
        const float4 gv = *reinterpret_cast<const float4 *>(gbase + (int64_t)k * Wd + c);
        Qs[k * KS + c] = qv.x;
        Qs[k * KS + c + 1] = qv.y;
        Qs[k * KS + c + 2] = qv.z;
        Qs[k * KS + c + 3] = qv.w;
        Gs[k * KS + c] = gv.x;
        Gs[k * KS + c + 1] = gv.y;
        Gs[k * KS + c + 2] = gv.z;
        Gs[k * KS + c + 3] = gv.w;
    }
    for (int i = t; i < 3 * T; i += 256) St[i] = sbase[i];
    __syncthreads();
    float *pw = Ps + w * 2 * Tp, *dw = pw + Tp;
    for (int r0 = 0; r0 < T; r0 += 4) {
        const int row = r0 + w;                               // the key row
        const bool ok = row < T;                              // wave-uniform
        if (ok) {
            float4 kk[D / 4], vv[D / 4];
#pragma unroll
            for (int c = 0; c < D / 4; c++) {
                kk[c] = *reinterpret_cast<const float4 *>(base + row * ld + Wd + 4 * c);
                vv[c] = *reinterpret_cast<const float4 *>(base + row * ld + 2 * Wd + 4 * c);
            }
#pragma unroll
            for (int j = 0; j < CL_KEYS; j++) {
                const int i = lane + 64 * j;                  // the query row
                if (i < T) {
                    const float *qr = Qs + i * KS, *gr = Gs + i * KS;
                    float a = 0.f, b = 0.f;
#pragma unroll
                    for (int c = 0; c < D / 4; c++) {
                        a = fmaf(qr[4 * c], kk[c].x, a);
                        a = fmaf(qr[4 * c + 1], kk[c].y, a);
                        a = fmaf(qr[4 * c + 2], kk[c].z, a);
                        a = fmaf(qr[4 * c + 3], kk[c].w, a);
                        b = fmaf(gr[4 * c], vv[c].x, b);
                        b = fmaf(gr[4 * c + 1], vv[c].y, b);
                        b = fmaf(gr[4 * c + 2], vv[c].z, b);
                        b = fmaf(gr[4 * c + 3], vv[c].w, b);
                    }
                    const float p = expf(a * scale - St[3 * i]) / St[3 * i + 1];
                    pw[i] = p;
                    dw[i] = p * (b - St[3 * i + 2]);
                }
            }
        }
        __syncthreads();
        if (ok && lane < D) {
            float gv = 0.f, gk = 0.f;
            for (int i = 0; i < T; i++) {
                gv = fmaf(pw[i], Gs[i * KS + lane], gv);
                gk = fmaf(dw[i], Qs[i * KS + lane], gk);
            }
            float *o = gqkv + ((int64_t)n * T + row) * ld + h * D + lane;
            o[Wd] = gk * scale;
            o[2 * Wd] = gv;
        }
        __syncthreads();
    }
}

// one RICK_LDS160_ONCE expansion site per kernel and D, as cl_attention_launch
template <int D>
static void cl_attention_bwd_launch(const float *qkv, const float *go, float *stats, float *gqkv, int N, int T, int Wd, int heads,
                                    hipStream_t st) {
    const size_t lq = cl_attention_bwd_q_lds(T, D), lkv = cl_attention_bwd_kv_lds(T, D);
    if (lq > 64 * 1024) RICK_LDS160_ONCE(clip_attention_bwd_q_kernel<D>);
    if (lkv > 64 * 1024) RICK_LDS160_ONCE(clip_attention_bwd_kv_kernel<D>);
    hipLaunchKernelGGL(clip_attention_bwd_q_kernel<D>, dim3((unsigned)(N * heads)), dim3(256), lq, st, qkv, go, stats, gqkv, T, Wd, heads);
    hipLaunchKernelGGL(clip_attention_bwd_kv_kernel<D>, dim3((unsigned)(N * heads)), dim3(256), lkv, st, qkv, go, (const float *)stats,
                       gqkv, T, Wd, heads);
}

// ---- input, adjoint ---------------------------------------------------------------------------------------------------------------
// Gather form of clip_input_kernel's adjoint: one thread per source pixel sums, in ascending destination order (rows, then
// columns), the destination pixels that tap it.  The floor of a destination's source coordinate is monotone in the
// destination, and destination d taps source i (border clamping included) exactly when i - 2 <= floor(s(d)) <= i + 1, so the
// destinations of a source are one interval per axis, found from an estimate and corrected with the forward's own arithmetic.
// The weight of (d -> i) is the sum of d's taps whose clamped index is i.  g is read in patch-row layout
// [N G^2][(ky, kx, c4)], G = S / P (the patch GEMM's data gradient), out is planar [N, 3, H, W].
__device__ __forceinline__ int cl_src_floor(int dst, float scale) {
    return (int)floorf(__fsub_rn(__fmul_rn(scale, (float)dst + 0.5f), 0.5f));
}
__device__ __forceinline__ int cl_first_dst(int src, float scale, int S) {       // the first d with floor(s(d)) >= src - 2
    int d = (int)fminf(fmaxf(floorf(((float)src - 1.5f) / scale - 0.5f), 0.f), (float)(S - 1));
    while (d > 0 && cl_src_floor(d - 1, scale) >= src - 2) d--;
    while (d < S && cl_src_floor(d, scale) < src - 2) d++;
    return d;
}
__device__ __forceinline__ float cl_tap_weight(int dst, float scale, int n_in, int src) {
    int idx[4];
    float w[4], s = 0.f;
    cl_cubic_taps(dst, scale, n_in, idx, w);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (idx[k] == src) s += w[k];
    return s;
}

__global__ __launch_bounds__(256) void clip_input_bwd_kernel(const float *__restrict__ g, float *__restrict__ out, int N, int H, int W,
                                                             int S, int P, float sh, float sw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * H * W) return;
    const int ix = (int)(i % W), iy = (int)((i / W) % H), n = (int)(i / ((int64_t)H * W));
    const int G = S / P;
    const int y0 = cl_first_dst(iy, sh, S), x0 = cl_first_dst(ix, sw, S);
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    for (int oy = y0; oy < S && cl_src_floor(oy, sh) <= iy + 1; oy++) {
        const float wy = cl_tap_weight(oy, sh, H, iy);
        const int64_t prow = ((int64_t)n * G + oy / P) * G;
        for (int ox = x0; ox < S && cl_src_floor(ox, sw) <= ix + 1; ox++) {
            const float wt = wy * cl_tap_weight(ox, sw, W, ix);
            const float4 v = *reinterpret_cast<const float4 *>(g + (((prow + ox / P) * P + oy % P) * P + ox % P) * 4);
            a0 = fmaf(wt, v.x, a0);
            a1 = fmaf(wt, v.y, a1);
            a2 = fmaf(wt, v.z, a2);
        }
    }
    // the affine's adjoint: g * 0.5 / std_c
    const int64_t hw = (int64_t)H * W, o = (int64_t)n * 3 * hw + (int64_t)iy * W + ix;
    out[o] = __fdiv_rn(__fmul_rn(a0, 0.5f), 0.26862954f);
    out[o + hw] = __fdiv_rn(__fmul_rn(a1, 0.5f), 0.26130258f);
    out[o + 2 * hw] = __fdiv_rn(__fmul_rn(a2, 0.5f), 0.27577711f);
}

// ---- entries ------------------------------------------------------------------------------------------------------------------
static bool cl_aligned16(const void *a, const void *b = nullptr, const void *c = nullptr, const void *d = nullptr) {
    return (((uintptr_t)a | (uintptr_t)b | (uintptr_t)c | (uintptr_t)d) % 16) == 0;
}

static int cl_input_entry(const float *x, float *out, int N, int H, int W, int S, const cl_affine &k, void *stream) {
    if (!x || !out || N < 0 || H <= 0 || W <= 0 || S <= 0 || !cl_aligned16(out)) return RICK_EINVAL;
    if ((int64_t)H * W > 0x7fffffff / 4 || (int64_t)N * S * S > ((int64_t)1 << 36)) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(clip_input_kernel, dim3((unsigned)cdiv64((int64_t)N * S * S, 256)), dim3(256), 0, (hipStream_t)stream, x, out,
                       N, H, W, S, (float)H / (float)S, (float)W / (float)S, k);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_input_f32(const float *x, float *out, int N, int H, int W, int S, void *stream) {
    return cl_input_entry(x, out, N, H, W, S, cl_affine{{0.48145466f, 0.4578275f, 0.40821073f}, {0.26862954f, 0.26130258f, 0.27577711f}},
                          stream);
}

extern "C" int rick_vit_input_f32(const float *x, float *out, int N, int H, int W, int S, float mean0, float mean1, float mean2,
                                  float std0, float std1, float std2, void *stream) {
    const cl_affine k{{mean0, mean1, mean2}, {std0, std1, std2}};
    for (int c = 0; c < 3; c++)
        if (!(fabsf(k.mean[c]) <= FLT_MAX) || !(k.std[c] > 0.f && k.std[c] <= FLT_MAX)) return RICK_EINVAL;     // finite, std > 0
    return cl_input_entry(x, out, N, H, W, S, k, stream);
}

extern "C" int rick_clip_layernorm_f32(const float *in, int64_t ldx, const float *w, const float *b, float *out, int R, int C,
                                       float eps, void *stream) {
    if (!in || !w || !b || !out || R < 0 || C <= 0 || (C & 3) || C > CL_MAXC || ldx < C || (ldx & 3) || !(eps >= 0.f) ||
        !cl_aligned16(in, w, b, out))
        return RICK_EINVAL;
    if (R == 0) return 0;
    hipLaunchKernelGGL(clip_layernorm_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, in, ldx, w, b, out, R, C,
                       eps);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_tokens_f32(const float *patches, const float *cls, const float *pos, const float *w, const float *b,
                                    float *out, int N, int T, int C, float eps, void *stream) {
    if (!patches || !cls || !pos || !w || !b || !out || N < 0 || T < 2 || T > CL_MAXT || C <= 0 || (C & 3) || C > CL_MAXC ||
        !(eps >= 0.f) || !cl_aligned16(patches, cls, pos, w) || !cl_aligned16(b, out))
        return RICK_EINVAL;
    if (N == 0) return 0;
    if ((int64_t)N * T > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(clip_tokens_kernel, dim3((unsigned)cdiv64((int64_t)N * T, 4)), dim3(256), 0, (hipStream_t)stream, patches, cls,
                       pos, w, b, out, N, T, C, eps);
    RICK_LAUNCH_STATUS();
}

template <bool CAUSAL>
static int cl_attention_entry(const float *qkv, float *out, int N, int T, int heads, int D, void *stream) {
    if (!qkv || !out || N < 0 || T < 1 || T > CL_MAXT || heads < 1 || heads > 1024 || (D != 16 && D != 32 && D != 64) ||
        !cl_aligned16(qkv, out))
        return RICK_EINVAL;
    if (N == 0) return 0;
    if ((int64_t)N * heads > 0x7fffffff || cl_attention_lds(T, D) > 160 * 1024) return RICK_EINVAL;
    const int Wd = heads * D;
    hipStream_t st = (hipStream_t)stream;
    if (D == 16) cl_attention_launch<16, CAUSAL>(qkv, out, N, T, Wd, heads, st);
    else if (D == 32) cl_attention_launch<32, CAUSAL>(qkv, out, N, T, Wd, heads, st);
    else cl_attention_launch<64, CAUSAL>(qkv, out, N, T, Wd, heads, st);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_text_tokens_f32(const int32_t *ids, const float *table, const float *pos, float *out, int N, int T, int V,
                                         int C, void *stream) {
    if (!ids || !table || !pos || !out || N < 0 || T < 1 || T > CL_MAXT || V < 1 || C <= 0 || (C & 3) || C > CL_MAXC ||
        ((uintptr_t)ids & 3) || !cl_aligned16(table, pos, out))
        return RICK_EINVAL;
    if (N == 0) return 0;
    const int64_t total = (int64_t)N * T * (C / 4);
    if (cdiv64(total, 256) > 0x7fffffff) return RICK_EINVAL;                  // the grid's x extent
    hipLaunchKernelGGL(clip_text_tokens_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, ids, table, pos,
                       out, total, T, V, C / 4);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_vit_tokens_f32(const float *patches, const float *cls, const float *pos, float *out, int N, int T, int C,
                                   void *stream) {
    if (!patches || !cls || !pos || !out || N < 0 || T < 2 || T > CL_MAXT || C <= 0 || (C & 3) || C > CL_MAXC ||
        !cl_aligned16(patches, cls, pos, out))
        return RICK_EINVAL;
    if (N == 0) return 0;
    const int64_t total = (int64_t)N * T * (C / 4);
    if (cdiv64(total, 256) > 0x7fffffff) return RICK_EINVAL;                  // the grid's x extent
    hipLaunchKernelGGL(vit_tokens_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, patches, cls, pos, out,
                       total, T, C / 4);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_layernorm_rows_f32(const float *in, const int32_t *idx, const float *w, const float *b, float *out, int R,
                                            int C, float eps, void *stream) {
    if (!in || !idx || !w || !b || !out || R < 0 || C <= 0 || (C & 3) || C > CL_MAXC || !(eps >= 0.f) || ((uintptr_t)idx & 3) ||
        !cl_aligned16(in, w, b, out))
        return RICK_EINVAL;
    if (R == 0) return 0;
    hipLaunchKernelGGL(clip_layernorm_rows_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, in, idx, w, b, out, R,
                       C, eps);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_attention_f32(const float *qkv, float *out, int N, int T, int heads, int D, void *stream) {
    return cl_attention_entry<false>(qkv, out, N, T, heads, D, stream);
}

extern "C" int rick_clip_attention_causal_f32(const float *qkv, float *out, int N, int T, int heads, int D, void *stream) {
    return cl_attention_entry<true>(qkv, out, N, T, heads, D, stream);
}

extern "C" int rick_clip_quickgelu_f32(const float *u, float *out, int64_t n, void *stream) {
    if (!u || !out || n < 0 || n > ((int64_t)1 << 38)) return RICK_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(clip_quickgelu_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, u, out, n);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_quickgelu_bwd_f32(const float *u, const float *g, float *out, int64_t n, void *stream) {
    if (!u || !g || !out || n < 0 || n > ((int64_t)1 << 38)) return RICK_EINVAL;
    if (n == 0) return 0;
    hipLaunchKernelGGL(clip_quickgelu_bwd_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, u, g, out, n);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_layernorm_bwd_f32(const float *x, int64_t ldx, const float *w, const float *g, int64_t ldg, const float *add,
                                           float *out, int64_t ldo, int R, int C, float eps, void *stream) {
    if (!x || !w || !g || !out || R < 0 || C <= 0 || (C & 3) || C > CL_MAXC || ldx < C || (ldx & 3) || ldg < C || (ldg & 3) ||
        ldo < C || (ldo & 3) || !(eps >= 0.f) || !cl_aligned16(x, w, g, out) || !cl_aligned16(add))
        return RICK_EINVAL;
    if (R == 0) return 0;
    hipLaunchKernelGGL(clip_layernorm_bwd_kernel, dim3((unsigned)cdiv(R, 4)), dim3(256), 0, (hipStream_t)stream, x, ldx, w, g, ldg, add,
                       out, ldo, R, C, eps);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_tokens_bwd_f32(const float *patches, const float *pos, const float *w, const float *g, float *out, int N,
                                        int T, int C, float eps, void *stream) {
    if (!patches || !pos || !w || !g || !out || N < 0 || T < 2 || T > CL_MAXT || C <= 0 || (C & 3) || C > CL_MAXC || !(eps >= 0.f) ||
        !cl_aligned16(patches, pos, w, g) || !cl_aligned16(out))
        return RICK_EINVAL;
    if (N == 0) return 0;
    if ((int64_t)N * T > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(clip_tokens_bwd_kernel, dim3((unsigned)cdiv64((int64_t)N * (T - 1), 4)), dim3(256), 0, (hipStream_t)stream,
                       patches, pos, w, g, out, N, T, C, eps);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_attention_bwd_f32(const float *qkv, const float *g_out, float *stats, float *g_qkv, int N, int T, int heads,
                                           int D, void *stream) {
    if (!qkv || !g_out || !stats || !g_qkv || N < 0 || T < 1 || T > CL_MAXT || heads < 1 || heads > 1024 ||
        (D != 16 && D != 32 && D != 64) || !cl_aligned16(qkv, g_out, g_qkv))
        return RICK_EINVAL;
    if (N == 0) return 0;
    if ((int64_t)N * heads > 0x7fffffff || cl_attention_bwd_q_lds(T, D) > 160 * 1024 || cl_attention_bwd_kv_lds(T, D) > 160 * 1024)
        return RICK_EINVAL;
    const int Wd = heads * D;
    hipStream_t st = (hipStream_t)stream;
    if (D == 16) cl_attention_bwd_launch<16>(qkv, g_out, stats, g_qkv, N, T, Wd, heads, st);
    else if (D == 32) cl_attention_bwd_launch<32>(qkv, g_out, stats, g_qkv, N, T, Wd, heads, st);
    else cl_attention_bwd_launch<64>(qkv, g_out, stats, g_qkv, N, T, Wd, heads, st);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_clip_input_bwd_f32(const float *g, float *out, int N, int H, int W, int S, int P, void *stream) {
    if (!g || !out || N < 0 || H <= 0 || W <= 0 || S <= 0 || P <= 0 || S % P || !cl_aligned16(g)) return RICK_EINVAL;
    if ((int64_t)H * W > 0x7fffffff / 4 || (int64_t)N * S * S > ((int64_t)1 << 36) || (int64_t)N * H * W > ((int64_t)1 << 36))
        return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(clip_input_bwd_kernel, dim3((unsigned)cdiv64((int64_t)N * H * W, 256)), dim3(256), 0, (hipStream_t)stream, g, out,
                       N, H, W, S, P, (float)H / (float)S, (float)W / (float)S);
    RICK_LAUNCH_STATUS();
}
