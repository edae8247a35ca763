// LPIPS (VGG16 backbone, lpips 0.1) kernels for on-device intra-cluster LPIPS — include/rick_hip.h "LPIPS".
//
// The 13 convolutions of the trunk run on rick_inc_conv_f32 (inception.hip).  This file holds what is specific to LPIPS:
// the input (uint8 round trip of the reference's PNG files + the scaling layer), the 2x2 max pool, the per-position inverse
// channel norm at each tap, and the pair distances over stored taps.  Activations are NHWC fp32.  No atomics: every output
// element has one writer and a fixed summation order.
#include "common.h"

// The input arithmetic must be the reference's fp32 operations one by one (torchvision save_image / ToTensor / Normalize,
// lpips' ScalingLayer), and the pair kernel's a*ia - b*ib must not become fma(a, ia, -b*ib), which is not antisymmetric.
#pragma clang fp contract(off)

#define LP_TILE 16             // images per tile side: a block computes 16 x 16 pairs, one per thread
#define LP_KC 256              // feature elements per LDS stage (per image)
#define LP_LD (LP_KC + 4)      // LDS row stride: the 16 B shift per row keeps the 16 rows' float4 reads on distinct banks
#define LP_MAXC 1024

// lpips ScalingLayer (fp32 buffers): (x - shift) / scale
__constant__ float lp_shift[3] = {-.030f, -.088f, -.188f};
__constant__ float lp_scale[3] = {.458f, .448f, .450f};

// ---- input: planar [N, 3, H, W] -> NHWC4 (channel 3 = 0) ---------------------------------------------------------------
// mode 0: float x, scaling layer only.  mode 1: float x through the PNG round trip q = uint8(clamp((x / 2 + 0.5) * 255 + 0.5,
// 0, 255)) (q optionally written to u8out, planar), then t = q / 255, (t - 0.5) / 0.5, scaling layer.  mode 2: uint8 input q.
__global__ __launch_bounds__(256) void lp_input_kernel(const float *__restrict__ x, const uint8_t *__restrict__ xq,
                                                       float *__restrict__ out, uint8_t *__restrict__ u8out, int N, int HW,
                                                       int mode) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * HW) return;
    const int64_t n = i / HW, p = i - n * HW;
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const int64_t src = (n * 3 + c) * HW + p;
        float v;
        if (mode == 0) {
            v = x[src];
        } else {
            float q;
            if (mode == 1) {
                float s = __fadd_rn(__fmul_rn(__fadd_rn(__fdiv_rn(x[src], 2.f), 0.5f), 255.f), 0.5f);
                s = fminf(fmaxf(s, 0.f), 255.f);
                const int qi = (int)s;                                 // truncation, as the uint8 cast does
                if (u8out) u8out[src] = (uint8_t)qi;
                q = (float)qi;
            } else {
                q = (float)xq[src];
            }
            v = __fdiv_rn(__fsub_rn(__fdiv_rn(q, 255.f), 0.5f), 0.5f);
        }
        r[c] = __fdiv_rn(__fsub_rn(v, lp_shift[c]), lp_scale[c]);
    }
    reinterpret_cast<float4 *>(out)[i] = make_float4(r[0], r[1], r[2], 0.f);
}

// ---- 2x2 stride-2 max pool, floor: [N, IH, IW, C] -> [N, IH/2, IW/2, C] ----------------------------------------------------
__global__ __launch_bounds__(256) void lp_maxpool2_kernel(const float *__restrict__ in, float *__restrict__ out, int N, int IH,
                                                          int IW, int C) {
    const int OH = IH / 2, OW = IW / 2, C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * OH * OW * C4) return;
    const int c = (int)(i % C4) * 4;
    const int64_t p = i / C4;
    const int ox = (int)(p % OW), oy = (int)((p / OW) % OH);
    const int64_t n = p / ((int64_t)OW * OH);
    const float *b = in + ((n * IH + 2 * oy) * IW + 2 * ox) * C + c;
    const float4 v0 = *reinterpret_cast<const float4 *>(b), v1 = *reinterpret_cast<const float4 *>(b + C);
    const float4 v2 = *reinterpret_cast<const float4 *>(b + (int64_t)IW * C), v3 = *reinterpret_cast<const float4 *>(b + (int64_t)IW * C + C);
    reinterpret_cast<float4 *>(out)[i] = make_float4(fmaxf(fmaxf(v0.x, v1.x), fmaxf(v2.x, v3.x)), fmaxf(fmaxf(v0.y, v1.y), fmaxf(v2.y, v3.y)),
                                                     fmaxf(fmaxf(v0.z, v1.z), fmaxf(v2.z, v3.z)), fmaxf(fmaxf(v0.w, v1.w), fmaxf(v2.w, v3.w)));
}

// ---- inverse channel norm: out[p] = 1 / (sqrt(sum_c f[p, c]^2) + 1e-10), 0 where the sum is 0 -------------------------------
// One wave per position: lane l sums channels 4 l + 256 j (j ascending), then a fixed butterfly; lane 0 writes.
__global__ __launch_bounds__(256) void lp_invnorm_kernel(const float *__restrict__ in, float *__restrict__ out, int64_t P, int C) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;                                                // wave-uniform
    const float *row = in + p * C;
    float s = 0.f;
    for (int c = 4 * lane; c < C; c += 256) {
        const float4 v = *reinterpret_cast<const float4 *>(row + c);
        s = fmaf(v.x, v.x, s);
        s = fmaf(v.y, v.y, s);
        s = fmaf(v.z, v.z, s);
        s = fmaf(v.w, v.w, s);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) out[p] = s > 0.f ? __fdiv_rn(1.f, __fadd_rn(__fsqrt_rn(s), 1e-10f)) : 0.f;
}

// ---- pair partials of one tap ----------------------------------------------------------------------------------------------
// part[slice][i][j] = sum over positions of the slice, channels ascending, of w_c (a_ic ia_i - b_jc ib_j)^2  (fp64 out).
// Block = (slice, A tile, B tile).  A slice of positions x all channels is a contiguous span of every image's tap: each stage
// copies LP_KC elements of 16 A and 16 B images into LDS, normalised, and every thread runs its pair over the stage in element
// order (fp32), adding the stage sum to an fp64 accumulator.  The order of every sum depends on (position, channel) only:
// d(x, x) = 0, D(A, B) = D(B, A)^T and a pair's value does not depend on the other images of the call.
__device__ __forceinline__ void lp_stage(float *dst, const float *f, const float *inv, int n, int i0, int64_t img_stride, int HW,
                                         int C, int64_t e0, int kc, int pos0, int t) {
#pragma unroll
    for (int it = 0; it < 4; it++) {
        const int idx = t + 256 * it, r = idx / (LP_KC / 4), k = 4 * (idx % (LP_KC / 4));
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i0 + r < n && k < kc) {
            const int64_t e = (int64_t)pos0 * C + e0 + k;              // element of the image's tap
            const int64_t img = i0 + r;
            const float s = inv[img * HW + e / C];
            const float4 a = *reinterpret_cast<const float4 *>(f + img * img_stride + e);
            v = make_float4(a.x * s, a.y * s, a.z * s, a.w * s);
        }
        *reinterpret_cast<float4 *>(dst + r * LP_LD + k) = v;
    }
}

__global__ __launch_bounds__(256) void lp_pair_kernel(const float *__restrict__ fa, const float *__restrict__ ia, int na,
                                                      const float *__restrict__ fb, const float *__restrict__ ib, int nb,
                                                      const float *__restrict__ w, int HW, int C, int pps,
                                                      double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[LP_TILE * LP_LD];
    __shared__ __attribute__((aligned(16))) float Bs[LP_TILE * LP_LD];
    __shared__ __attribute__((aligned(16))) float Ws[LP_MAXC];
    const int t = threadIdx.x, ti = t >> 4, tj = t & 15;
    const int slice = blockIdx.x, i0 = blockIdx.y * LP_TILE, j0 = blockIdx.z * LP_TILE;
    const int pos0 = slice * pps, npos = min(pps, HW - pos0);
    const int64_t L = (int64_t)npos * C, stride = (int64_t)HW * C;
    for (int c = t; c < C; c += 256) Ws[c] = w[c];
    double acc = 0.0;
    for (int64_t e0 = 0; e0 < L; e0 += LP_KC) {
        const int kc = (int)min((int64_t)LP_KC, L - e0);
        __syncthreads();
        lp_stage(As, fa, ia, na, i0, stride, HW, C, e0, kc, pos0, t);
        lp_stage(Bs, fb, ib, nb, j0, stride, HW, C, e0, kc, pos0, t);
        __syncthreads();
        const float *a = As + ti * LP_LD, *b = Bs + tj * LP_LD;
        int c = (int)(e0 % C);
        float s = 0.f;
        for (int k = 0; k < kc; k += 4) {
            const float4 av = *reinterpret_cast<const float4 *>(a + k), bv = *reinterpret_cast<const float4 *>(b + k);
            const float4 wv = *reinterpret_cast<const float4 *>(Ws + c);
            float d = av.x - bv.x;
            s = fmaf(wv.x, d * d, s);
            d = av.y - bv.y;
            s = fmaf(wv.y, d * d, s);
            d = av.z - bv.z;
            s = fmaf(wv.z, d * d, s);
            d = av.w - bv.w;
            s = fmaf(wv.w, d * d, s);
            c += 4;
            if (c == C) c = 0;
        }
        acc += (double)s;
    }
    const int i = i0 + ti, j = j0 + tj;
    if (i < na && j < nb) part[((int64_t)slice * na + i) * nb + j] = acc;
}

// ---- paired partials of one tap: image i of fa against image i of fb only --------------------------------------------------------
// part[slice][i] = what lp_pair_kernel writes to part[slice][i][i], bit for bit, for n pairs instead of n^2.  The pair kernel's
// value is fixed by three orders: inside a stage of LP_KC elements one fp32 chain s = fma(w_c, (a ia - b ib)^2, s) in element
// order from 0, the stage sums added to an fp64 accumulator in stage order, the slices added by lp_reduce_kernel.  Block =
// (slice, pair): all 256 threads stream the slice of both images once and leave q = (a ia - b ib)^2 in LDS (the same three fp32
// roundings as lp_stage + the pair loop: two products, one difference, one square — fp contraction is off in this file), then
// thread k < 32 runs stage k's chain over its LDS row (row stride LP_LD: the 32 rows' float4 reads fall on distinct banks), and
// thread 0 adds the stage sums in order.  A slice holds at most LP_PSTAGES stages (pps * C <= 8192, checked by the entry).
#define LP_PSTAGES 32

// (a sa - b sb)^2 as four scalar-lane instructions, each one correctly rounded fp32 operation like the compiler's own v_mul_f32 /
// v_sub_f32 in lp_stage and lp_pair_kernel; written out because the compiler pairs the four channels of a float4 into
// v_pk_mul_f32 / v_pk_add_f32 here, and the build keeps this file's distance kernels scalar (tools/check_isa.py)
__device__ __forceinline__ float lp_sqdiff(float a, float sa, float b, float sb) {
    float u, v, d, q;
    asm("v_mul_f32 %0, %1, %2" : "=v"(u) : "v"(a), "v"(sa));
    asm("v_mul_f32 %0, %1, %2" : "=v"(v) : "v"(b), "v"(sb));
    asm("v_sub_f32 %0, %1, %2" : "=v"(d) : "v"(u), "v"(v));
    asm("v_mul_f32 %0, %1, %2" : "=v"(q) : "v"(d), "v"(d));
    return q;
}

__global__ __launch_bounds__(256) void lp_paired_kernel(const float *__restrict__ fa, const float *__restrict__ ia, int64_t sa,
                                                        const float *__restrict__ fb, const float *__restrict__ ib, int64_t sb,
                                                        int n, const float *__restrict__ w, int HW, int C, int pps, int nsl,
                                                        double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float Qs[LP_PSTAGES * LP_LD];
    __shared__ __attribute__((aligned(16))) float Ws[LP_MAXC];
    __shared__ float Ss[LP_PSTAGES];
    const int t = threadIdx.x;
    const int slice = (int)(blockIdx.x % (unsigned)nsl);
    const int64_t i = blockIdx.x / (unsigned)nsl;
    const int pos0 = slice * pps, npos = min(pps, HW - pos0);
    const int L = npos * C;                                            // <= LP_PSTAGES * LP_KC
    const float *a = fa + (i * sa * HW + pos0) * C, *b = fb + (i * sb * HW + pos0) * C;
    const float *na = ia + i * sa * HW + pos0, *nb = ib + i * sb * HW + pos0;
    for (int c = t; c < C; c += 256) Ws[c] = w[c];
    for (int e = 4 * t; e < L; e += 1024) {
        const int p = e / C;
        const float s1 = na[p], s2 = nb[p];
        const float4 x = *reinterpret_cast<const float4 *>(a + e), y = *reinterpret_cast<const float4 *>(b + e);
        const float4 q = make_float4(lp_sqdiff(x.x, s1, y.x, s2), lp_sqdiff(x.y, s1, y.y, s2), lp_sqdiff(x.z, s1, y.z, s2),
                                     lp_sqdiff(x.w, s1, y.w, s2));
        *reinterpret_cast<float4 *>(Qs + (e / LP_KC) * LP_LD + (e % LP_KC)) = q;
    }
    __syncthreads();
    const int nst = (L + LP_KC - 1) / LP_KC;
    if (t < nst) {
        const int e0 = t * LP_KC, kc = min(LP_KC, L - e0);
        const float *q = Qs + t * LP_LD;
        int c = e0 % C;
        float s = 0.f;
        for (int k = 0; k < kc; k += 4) {
            const float4 qv = *reinterpret_cast<const float4 *>(q + k), wv = *reinterpret_cast<const float4 *>(Ws + c);
            s = fmaf(wv.x, qv.x, s);
            s = fmaf(wv.y, qv.y, s);
            s = fmaf(wv.z, qv.z, s);
            s = fmaf(wv.w, qv.w, s);
            c += 4;
            if (c == C) c = 0;
        }
        Ss[t] = s;
    }
    __syncthreads();
    if (t == 0) {
        double acc = 0.0;
        for (int k = 0; k < nst; k++) acc += (double)Ss[k];
        part[(int64_t)slice * n + i] = acc;
    }
}

// ---- second stage: out[i][j] = sum over taps (in order) of (sum over slices, in order) / HW_l --------------------------------
__global__ __launch_bounds__(256) void lp_reduce_kernel(const double *__restrict__ part, float *__restrict__ out, int na, int nb,
                                                        rick_lpips_layers d) {
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x, npair = (int64_t)na * nb;
    if (q >= npair) return;
    const double *p = part + q;
    double tot = 0.0;
    for (int l = 0; l < d.nlayers; l++) {
        double s = 0.0;
        for (int k = 0; k < d.nslices[l]; k++, p += npair) s += *p;
        tot += s / (double)d.hw[l];
    }
    out[q] = (float)tot;
}

// ---- backward of one tap's distance with respect to the image's features ------------------------------------------------------
// g = d/da of go (1 / HW) sum_p sum_c w_c (a_c ia - t_c it)^2.  One wave per position; lane l owns channels 4 l + 256 j and adds
// its r_c a_c in that order (fma chain), then the wave_sum butterfly.  The target is image n of nt == n images or the one image.
__global__ __launch_bounds__(256) void lp_tap_bwd_kernel(const float *__restrict__ a, const float *__restrict__ ia,
                                                         const float *__restrict__ t, const float *__restrict__ it, int nt,
                                                         const float *__restrict__ w, const float *__restrict__ go, int HW, int C,
                                                         int relu, float *__restrict__ g, int64_t P) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;                                                // wave-uniform
    const int64_t n = p / HW, pt = nt == 1 ? p - n * HW : p;
    const float *ar = a + p * C, *tr = t + pt * C;
    float *gr = g + p * C;
    const float sa = ia[p], st = it[pt];
    if (!(sa > 0.f)) {                                                 // an all-zero position: the distance does not depend on it
        for (int c = 4 * lane; c < C; c += 256) *reinterpret_cast<float4 *>(gr + c) = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const float gs = __fdiv_rn(go[n], (float)HW);
    float4 av[LP_MAXC / 256], rv[LP_MAXC / 256];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < LP_MAXC / 256; j++) {
        const int c = 4 * lane + 256 * j;
        if (c >= C) break;
        const float4 x = *reinterpret_cast<const float4 *>(ar + c), y = *reinterpret_cast<const float4 *>(tr + c);
        const float4 wv = *reinterpret_cast<const float4 *>(w + c);
        float4 r;
        r.x = 2.f * wv.x * (x.x * sa - y.x * st) * gs;
        r.y = 2.f * wv.y * (x.y * sa - y.y * st) * gs;
        r.z = 2.f * wv.z * (x.z * sa - y.z * st) * gs;
        r.w = 2.f * wv.w * (x.w * sa - y.w * st) * gs;
        s = fmaf(r.x, x.x, s);
        s = fmaf(r.y, x.y, s);
        s = fmaf(r.z, x.z, s);
        s = fmaf(r.w, x.w, s);
        av[j] = x;
        rv[j] = r;
    }
    s = wave_sum(s);
    const float na = __fsub_rn(__fdiv_rn(1.f, sa), 1e-10f);            // |a|, undoing the epsilon of the inverse norm
    const float q = na > 0.f ? __fdiv_rn(s * sa * sa, na) : 0.f;
#pragma unroll
    for (int j = 0; j < LP_MAXC / 256; j++) {
        const int c = 4 * lane + 256 * j;
        if (c >= C) break;
        const float4 x = av[j], r = rv[j];
        float4 o = make_float4(sa * r.x - x.x * q, sa * r.y - x.y * q, sa * r.z - x.z * q, sa * r.w - x.w * q);
        if (relu) o = make_float4(x.x > 0.f ? o.x : 0.f, x.y > 0.f ? o.y : 0.f, x.z > 0.f ? o.z : 0.f, x.w > 0.f ? o.w : 0.f);
        *reinterpret_cast<float4 *>(gr + c) = o;
    }
}

// ---- 2x2 max-pool backward, gather form, fused with the tap gradient and the ReLU mask of the pooled activation ---------------
// One thread per pre-pool position and 4 channels.  The window's maximum goes to its first position in (dy, dx) scan order
// (torch's max_pool2d rule); positions the floor leaves outside every window only pass `add` on.
__device__ __forceinline__ float lp_pool_pick(float v0, float v1, float v2, float v3, int k, float gp) {
    const float m = fmaxf(fmaxf(v0, v1), fmaxf(v2, v3));
    const int first = v0 == m ? 0 : v1 == m ? 1 : v2 == m ? 2 : 3;
    return first == k ? gp : 0.f;
}
__global__ __launch_bounds__(256) void lp_maxpool2_bwd_kernel(const float *__restrict__ act, const float *__restrict__ add,
                                                              const float *__restrict__ gpool, float *__restrict__ out, int N,
                                                              int IH, int IW, int C) {
    const int OH = IH / 2, OW = IW / 2, C4 = C / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * IH * IW * C4) return;
    const int c = (int)(i % C4) * 4;
    const int64_t p = i / C4;
    const int x = (int)(p % IW), y = (int)((p / IW) % IH);
    const int64_t n = p / ((int64_t)IW * IH);
    const float4 v = *reinterpret_cast<const float4 *>(act + p * C + c);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (add) o = *reinterpret_cast<const float4 *>(add + p * C + c);
    const int oy = y >> 1, ox = x >> 1;
    if (oy < OH && ox < OW) {
        const float *b = act + ((n * IH + 2 * oy) * IW + 2 * ox) * C + c;
        const float4 v0 = *reinterpret_cast<const float4 *>(b), v1 = *reinterpret_cast<const float4 *>(b + C);
        const float4 v2 = *reinterpret_cast<const float4 *>(b + (int64_t)IW * C), v3 = *reinterpret_cast<const float4 *>(b + (int64_t)IW * C + C);
        const float4 gp = *reinterpret_cast<const float4 *>(gpool + ((n * OH + oy) * OW + ox) * C + c);
        const int k = 2 * (y & 1) + (x & 1);
        o.x += lp_pool_pick(v0.x, v1.x, v2.x, v3.x, k, gp.x);
        o.y += lp_pool_pick(v0.y, v1.y, v2.y, v3.y, k, gp.y);
        o.z += lp_pool_pick(v0.z, v1.z, v2.z, v3.z, k, gp.z);
        o.w += lp_pool_pick(v0.w, v1.w, v2.w, v3.w, k, gp.w);
    }
    reinterpret_cast<float4 *>(out)[i] = make_float4(v.x > 0.f ? o.x : 0.f, v.y > 0.f ? o.y : 0.f, v.z > 0.f ? o.z : 0.f,
                                                     v.w > 0.f ? o.w : 0.f);
}

// ---- input backward (mode 0): NHWC4 gradient -> planar [N, 3, H, W], through the scaling layer's division ----------------------
__global__ __launch_bounds__(256) void lp_input_bwd_kernel(const float *__restrict__ g, float *__restrict__ out, int N, int HW) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * HW) return;
    const int64_t n = i / HW, p = i - n * HW;
    const float4 v = reinterpret_cast<const float4 *>(g)[i];
    out[(n * 3 + 0) * HW + p] = __fdiv_rn(v.x, lp_scale[0]);
    out[(n * 3 + 1) * HW + p] = __fdiv_rn(v.y, lp_scale[1]);
    out[(n * 3 + 2) * HW + p] = __fdiv_rn(v.z, lp_scale[2]);
}

static unsigned lp_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int rick_lpips_input_f32(const float *x, const uint8_t *xq, float *out, uint8_t *u8out, int N, int H, int W,
                                    int mode, void *stream) {
    if (!out || N < 0 || H <= 0 || W <= 0 || mode < 0 || mode > 2 || ((uintptr_t)out % 16)) return RICK_EINVAL;
    if ((mode == 2 && !xq) || (mode != 2 && !x) || (u8out && mode != 1)) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(lp_input_kernel, dim3(lp_grid((int64_t)N * H * W)), dim3(256), 0, (hipStream_t)stream, x, xq, out, u8out,
                       N, H * W, mode);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_maxpool2_f32(const float *in, float *out, int N, int IH, int IW, int C, void *stream) {
    if (!in || !out || N < 0 || IH < 2 || IW < 2 || C <= 0 || (C & 3) || (((uintptr_t)in | (uintptr_t)out) % 16)) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(lp_maxpool2_kernel, dim3(lp_grid((int64_t)N * (IH / 2) * (IW / 2) * (C / 4))), dim3(256), 0,
                       (hipStream_t)stream, in, out, N, IH, IW, C);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_invnorm_f32(const float *in, float *out, int64_t P, int C, void *stream) {
    if (!in || !out || P < 0 || C <= 0 || (C & 3) || ((uintptr_t)in % 16)) return RICK_EINVAL;
    if (P == 0) return 0;
    hipLaunchKernelGGL(lp_invnorm_kernel, dim3((unsigned)cdiv64(P, 4)), dim3(256), 0, (hipStream_t)stream, in, out, P, C);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_pair_f32(const float *fa, const float *ia, int na, const float *fb, const float *ib, int nb,
                                   const float *w, int HW, int C, int pps, double *part, void *stream) {
    if (!fa || !ia || !fb || !ib || !w || !part || na < 0 || nb < 0 || HW <= 0 || C <= 0 || (C & 3) || C > LP_MAXC || pps <= 0)
        return RICK_EINVAL;
    if (((uintptr_t)fa | (uintptr_t)fb) % 16) return RICK_EINVAL;
    if (na == 0 || nb == 0) return 0;
    const int64_t nsl = cdiv64(HW, pps);
    if (nsl > 0x7fffffff || cdiv64(na, LP_TILE) > 65535 || cdiv64(nb, LP_TILE) > 65535) return RICK_EINVAL;
    const dim3 grid((unsigned)nsl, (unsigned)cdiv64(na, LP_TILE), (unsigned)cdiv64(nb, LP_TILE));
    hipLaunchKernelGGL(lp_pair_kernel, grid, dim3(256), 0, (hipStream_t)stream, fa, ia, na, fb, ib, nb, w, HW, C, pps, part);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_paired_f32(const float *fa, const float *ia, int sa, const float *fb, const float *ib, int sb, int n,
                                     const float *w, int HW, int C, int pps, double *part, void *stream) {
    if (!fa || !ia || !fb || !ib || !w || !part || sa < 1 || sb < 1 || n < 0 || HW <= 0 || C <= 0 || (C & 3) || C > LP_MAXC || pps <= 0)
        return RICK_EINVAL;
    if ((((uintptr_t)fa | (uintptr_t)fb) % 16) || ((uintptr_t)part % 8)) return RICK_EINVAL;
    if ((int64_t)(pps < HW ? pps : HW) * C > LP_PSTAGES * LP_KC) return RICK_EINVAL;     // a slice must fit the LDS rows
    if (n == 0) return 0;
    const int64_t nsl = cdiv64(HW, pps);
    if (nsl * n > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(lp_paired_kernel, dim3((unsigned)(nsl * n)), dim3(256), 0, (hipStream_t)stream, fa, ia, (int64_t)sa, fb, ib,
                       (int64_t)sb, n, w, HW, C, pps, (int)nsl, part);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_reduce_f32(const double *part, float *out, int na, int nb, const rick_lpips_layers *d, void *stream) {
    if (!part || !out || !d || na < 0 || nb < 0 || d->nlayers < 1 || d->nlayers > 8) return RICK_EINVAL;
    for (int l = 0; l < d->nlayers; l++)
        if (d->nslices[l] <= 0 || d->hw[l] <= 0) return RICK_EINVAL;
    if (na == 0 || nb == 0) return 0;
    hipLaunchKernelGGL(lp_reduce_kernel, dim3(lp_grid((int64_t)na * nb)), dim3(256), 0, (hipStream_t)stream, part, out, na, nb, *d);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_tap_bwd_f32(const float *a, const float *ia, const float *t, const float *it, int n, int nt,
                                      const float *w, const float *go, int HW, int C, int relu, float *g, void *stream) {
    if (!a || !ia || !t || !it || !w || !go || !g || n < 0 || (nt != n && nt != 1) || HW <= 0 || C <= 0 || (C & 3) || C > LP_MAXC)
        return RICK_EINVAL;
    if (((uintptr_t)a | (uintptr_t)t | (uintptr_t)w | (uintptr_t)g) % 16) return RICK_EINVAL;
    if (n == 0) return 0;
    const int64_t P = (int64_t)n * HW;
    if (cdiv64(P, 4) > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(lp_tap_bwd_kernel, dim3((unsigned)cdiv64(P, 4)), dim3(256), 0, (hipStream_t)stream, a, ia, t, it, nt, w, go,
                       HW, C, relu, g, P);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_maxpool2_bwd_f32(const float *act, const float *add, const float *gpool, float *out, int N, int IH,
                                           int IW, int C, void *stream) {
    if (!act || !gpool || !out || N < 0 || IH < 2 || IW < 2 || C <= 0 || (C & 3)) return RICK_EINVAL;
    if (((uintptr_t)act | (uintptr_t)add | (uintptr_t)gpool | (uintptr_t)out) % 16) return RICK_EINVAL;
    if (N == 0) return 0;
    const int64_t total = (int64_t)N * IH * IW * (C / 4);
    if (cdiv64(total, 256) > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(lp_maxpool2_bwd_kernel, dim3(lp_grid(total)), dim3(256), 0, (hipStream_t)stream, act, add, gpool, out, N,
                       IH, IW, C);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_lpips_input_bwd_f32(const float *g, float *out, int N, int H, int W, void *stream) {
    if (!g || !out || N < 0 || H <= 0 || W <= 0 || ((uintptr_t)g % 16)) return RICK_EINVAL;
    if (N == 0) return 0;
    if (cdiv64((int64_t)N * H * W, 256) > 0x7fffffff) return RICK_EINVAL;
    hipLaunchKernelGGL(lp_input_bwd_kernel, dim3(lp_grid((int64_t)N * H * W)), dim3(256), 0, (hipStream_t)stream, g, out, N, H * W);
    RICK_LAUNCH_STATUS();
}
