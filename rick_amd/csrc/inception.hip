// InceptionV3 (torchvision layout, up to pool3) inference kernels for on-device FID — include/rick_hip.h "Inception".
//
// Activations are NHWC fp32.  Every BasicConv2d (conv -> BatchNorm -> ReLU) runs as an implicit GEMM on the f32-input MFMA
// (v_mfma_f32_32x32x2_f32): exact fp32 products, one rounding per product, nothing to split and nothing that can saturate.
// The BN is folded into the packed weights and a per-column bias on the host (rick_amd/inception.py).  Every output element
// is written by exactly one thread with a fixed k order: no atomics, run-to-run bit-identical.
#include "common.h"

typedef float inc_f32x16 __attribute__((ext_vector_type(16)));

#define IC_BM 128        // GEMM rows (output positions) per block
#define IC_BK 32         // K per LDS stage
#define IC_AS (IC_BM + 1)  // A tile row stride in floats: the [k][row] transpose writes hit 32 distinct banks

// ---- input: bilinear resize (F.interpolate, align_corners=False, no antialias) + ImageNet affine, NCHW -> NHWC4 ------------
// AFFINE = false (the Inception Score's network, which sees the images as they are): no affine, and a plain copy where the
// output size is the input size (the interpolation formula would turn -0 into +0).
template <bool AFFINE>
__global__ __launch_bounds__(256) void inc_input_kernel(const float *__restrict__ x, float *__restrict__ out, int N, int H, int W,
                                                        int OH, int OW, float sh, float sw) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t total = (int64_t)N * OH * OW;
    if (i >= total) return;
    const int ox = (int)(i % OW), oy = (int)((i / OW) % OH), n = (int)(i / ((int64_t)OW * OH));
    // area_pixel_compute_source_index (align_corners=False): (dst + 0.5) * scale - 0.5, clamped at 0
    float fy = fmaxf((oy + 0.5f) * sh - 0.5f, 0.f), fx = fmaxf((ox + 0.5f) * sw - 0.5f, 0.f);
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
    const float ly = fy - y0, lx = fx - x0, hy = 1.f - ly, hx = 1.f - lx;
    const float mul[3] = {0.229f / 0.5f, 0.224f / 0.5f, 0.225f / 0.5f};
    const float add[3] = {(0.485f - 0.5f) / 0.5f, (0.456f - 0.5f) / 0.5f, (0.406f - 0.5f) / 0.5f};
    float r[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const float *p = x + ((int64_t)n * 3 + c) * H * W;
        if (!AFFINE && OH == H && OW == W) {
            r[c] = p[oy * W + ox];
            continue;
        }
        const float v = hy * (hx * p[y0 * W + x0] + lx * p[y0 * W + x1]) + ly * (hx * p[y1 * W + x0] + lx * p[y1 * W + x1]);
        r[c] = AFFINE ? v * mul[c] + add[c] : v;
    }
    reinterpret_cast<float4 *>(out)[i] = make_float4(r[0], r[1], r[2], 0.f);
}

// ---- implicit-GEMM convolution + bias + ReLU, columns routed to channel slices ---------------------------------------------
// C[m, col] = relu(sum_k A[m, k] * B[k, col] + bias[col]),  m = (n, oy, ox),  k = (ky, kx, ci),  B = packed weights [Kp][Cop]
// (zero rows beyond K, zero columns beyond Co).  Block: 128 rows x BN = 64 NT columns, four waves as 2 x 2, each wave
// 64 x 32 NT through 2 x NT accumulators of v_mfma_f32_32x32x2_f32.  One LDS stage; the next stage's global loads are in
// flight while the current one is multiplied.
__device__ __forceinline__ float4 inc_ld_a(const float *rowp, int iy, int ix, int c, bool kok, int IH, int IW, int Ci) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (kok && iy >= 0 && iy < IH && ix >= 0 && ix < IW)
        v = *reinterpret_cast<const float4 *>(rowp + ((int64_t)iy * IW + ix) * Ci + c);
    return v;
}
__device__ __forceinline__ void inc_st_a(float *p, const float4 v) {     // 4 consecutive k of one row: column of the [k][row] tile
    p[0] = v.x;
    p[IC_AS] = v.y;
    p[2 * IC_AS] = v.z;
    p[3 * IC_AS] = v.w;
}
template <int BN>
__device__ __forceinline__ float4 inc_ld_b(const float *wpk, int k0, int idx, int Cop, int n0) {   // item idx of the [32][BN] tile
    return *reinterpret_cast<const float4 *>(wpk + (int64_t)(k0 + idx / (BN / 4)) * Cop + n0 + 4 * (idx % (BN / 4)));
}
// BWD = true is the data gradient of a 3x3 stride-1 pad-1 convolution (rick_inc_conv_bwd_f32): the same GEMM over the
// transposed, rotated filter with the epilogue out = (mask > 0) ? acc + add : 0 in place of bias + ReLU; one destination.
// LIN != 0 is the linear epilogue (rick_inc_conv_lin_f32): out = act(acc + bias) [+ res], act the identity (LIN = 1) or
// QuickGELU (LIN = 2), res (the `add` argument) laid out like the one destination and possibly the destination itself.
// QuickGELU in fp32, each operation rounded on its own: u * (1 / (1 + expf(-(1.702f * u)))).
__device__ __forceinline__ float inc_quickgelu(float u) {
    return __fmul_rn(u, __fdiv_rn(1.f, __fadd_rn(1.f, expf(-__fmul_rn(1.702f, u)))));
}
// LIN >= 3 is the ViT epilogue (rick_inc_conv_vit_f32): out = act(acc + bias) [* scale[col]] [+ res], act the identity (LIN = 3)
// or the exact GELU (LIN = 4), scale (LayerScale, the `mask` argument) one float per column, res as above.  Every operation
// is rounded on its own.  The exact GELU: 0.5f * u * (1.f + erff(u * 0.70710678118654752f)), in that order.  erff saturates
// to +-1 from |x| = 4 on, so u >= 6 comes back as u and u <= -6 as -0.
__device__ __forceinline__ float inc_gelu(float u) {
    return __fmul_rn(__fmul_rn(0.5f, u), __fadd_rn(1.f, erff(__fmul_rn(u, 0.70710678118654752f))));
}
template <int NT, bool BWD = false, int LIN = 0>
__global__ __launch_bounds__(256) void inc_conv_kernel(const float *__restrict__ in, const float *__restrict__ wpk,
                                                       const float *__restrict__ bias, rick_inc_conv a,
                                                       const float *__restrict__ mask, const float *__restrict__ add) {
    constexpr int BN = 64 * NT;
    __shared__ float As[IC_BK * IC_AS];
    __shared__ __attribute__((aligned(16))) float Bs[IC_BK * BN];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w & 1, wn = w >> 1;
    const int M = a.N * a.OH * a.OW, K = a.KH * a.KW * a.Ci, Kp = (K + IC_BK - 1) / IC_BK * IC_BK;
    const int m0 = blockIdx.x * IC_BM, n0 = blockIdx.y * BN;

    // A staging: thread = (4 consecutive k: k4, rows r + 32 j)
    const int k4 = t & 7, r = t >> 3;
    const float *rowp[4];
    int iy0[4], ix0[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        int m = m0 + r + 32 * j;
        const bool ok = m < M;
        m = ok ? m : 0;
        const int ox = m % a.OW, oy = (m / a.OW) % a.OH, n = m / (a.OW * a.OH);
        rowp[j] = in + (int64_t)n * a.IH * a.IW * a.Ci;
        iy0[j] = ok ? oy * a.SH - a.PH : -(1 << 20);          // invalid rows read as padding
        ix0[j] = ox * a.SW - a.PW;
    }
    float4 ra0, ra1, ra2, ra3, rb[4] = {};
#define IC_LOAD(k0_)                                                                                                         \
    do {                                                                                                                     \
        const int k = (k0_) + 4 * k4;                                                                                        \
        const int tap = k / a.Ci, c = k - tap * a.Ci, ky = tap / a.KW, kx = tap - ky * a.KW;                                 \
        ra0 = inc_ld_a(rowp[0], iy0[0] + ky, ix0[0] + kx, c, k < K, a.IH, a.IW, a.Ci);                                                      \
        ra1 = inc_ld_a(rowp[1], iy0[1] + ky, ix0[1] + kx, c, k < K, a.IH, a.IW, a.Ci);                                                      \
        ra2 = inc_ld_a(rowp[2], iy0[2] + ky, ix0[2] + kx, c, k < K, a.IH, a.IW, a.Ci);                                                      \
        ra3 = inc_ld_a(rowp[3], iy0[3] + ky, ix0[3] + kx, c, k < K, a.IH, a.IW, a.Ci);                                                      \
        rb[0] = inc_ld_b<BN>(wpk, (k0_), t, a.Cop, n0);                                                                      \
        rb[1] = inc_ld_b<BN>(wpk, (k0_), t + 256, a.Cop, n0);                                                                \
        if (NT == 2) {                                                                                                       \
            rb[2] = inc_ld_b<BN>(wpk, (k0_), t + 512, a.Cop, n0);                                                            \
            rb[3] = inc_ld_b<BN>(wpk, (k0_), t + 768, a.Cop, n0);                                                            \
        }                                                                                                                    \
    } while (0)
    inc_f32x16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;

    const int h = lane >> 5, l32 = lane & 31;
    IC_LOAD(0);
    for (int k0 = 0; k0 < Kp; k0 += IC_BK) {
        __syncthreads();
        inc_st_a(As + (4 * k4) * IC_AS + r, ra0);
        inc_st_a(As + (4 * k4) * IC_AS + r + 32, ra1);
        inc_st_a(As + (4 * k4) * IC_AS + r + 64, ra2);
        inc_st_a(As + (4 * k4) * IC_AS + r + 96, ra3);
#pragma unroll
        for (int i = 0; i < NT * 2; i++) {
            const int idx = t + 256 * i, kr = idx / (BN / 4), c4 = idx % (BN / 4);
            *reinterpret_cast<float4 *>(Bs + kr * BN + 4 * c4) = rb[i];
        }
        __syncthreads();
        if (k0 + IC_BK < Kp) IC_LOAD(k0 + IC_BK);
#pragma unroll
        for (int s = 0; s < IC_BK / 2; s++) {
            const int kk = 2 * s + h;
            float av[2], bv[NT];
#pragma unroll
            for (int i = 0; i < 2; i++) av[i] = As[kk * IC_AS + wm * 64 + 32 * i + l32];
#pragma unroll
            for (int j = 0; j < NT; j++) bv[j] = Bs[kk * BN + wn * 32 * NT + 32 * j + l32];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int j = 0; j < NT; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
    }

    // epilogue: D[row = (e & 3) + 8 (e >> 2) + 4 h][col = l32]; the column picks its destination slice
#pragma unroll
    for (int j = 0; j < NT; j++) {
        const int col = n0 + wn * 32 * NT + 32 * j + l32;
        if (col >= a.Co) continue;
        if constexpr (BWD) {
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int m = m0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (m >= M) continue;
                    const int64_t o = (int64_t)m * a.ldc[0] + col;
                    float v = acc[i][j][e];
                    if (add) v += add[o];
                    if (mask) v = mask[o] > 0.f ? v : 0.f;
                    a.dst[0][o] = v;
                }
            continue;
        }
        if constexpr (LIN >= 3) {
            float *dst = a.dst[0] + a.c0[0] + col;
            // the in-place residual is read through the destination pointer: `add` is __restrict__
            const float *res = add == a.dst[0] ? a.dst[0] : add;
            if (res) res += a.c0[0] + col;
            const float b = bias[col], sc = mask ? mask[col] : 1.f;
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int m = m0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (m >= M) continue;
                    const int64_t o = (int64_t)m * a.ldc[0];
                    float v = __fadd_rn(acc[i][j][e], b);
                    if (LIN == 4) v = inc_gelu(v);
                    if (mask) v = __fmul_rn(v, sc);
                    if (res) v = __fadd_rn(v, res[o]);
                    dst[o] = v;
                }
            continue;
        }
        if constexpr (LIN != 0) {
            float *dst = a.dst[0] + a.c0[0] + col;
            // the in-place residual is read through the destination pointer: `add` is __restrict__
            const float *res = add == a.dst[0] ? a.dst[0] : add;
            if (res) res += a.c0[0] + col;
            const float b = bias[col];
#pragma unroll
            for (int i = 0; i < 2; i++)
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    const int m = m0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                    if (m >= M) continue;
                    const int64_t o = (int64_t)m * a.ldc[0];
                    float v = acc[i][j][e] + b;
                    if (LIN == 2) v = inc_quickgelu(v);
                    if (res) v += res[o];
                    dst[o] = v;
                }
            continue;
        }
        const int sg = (col >= a.seg_start[1]) + (col >= a.seg_start[2]) + (col >= a.seg_start[3]);
        float *dst;
        int ldc;
        if (sg == 0) { dst = a.dst[0]; ldc = a.ldc[0]; }
        else if (sg == 1) { dst = a.dst[1]; ldc = a.ldc[1]; }
        else if (sg == 2) { dst = a.dst[2]; ldc = a.ldc[2]; }
        else { dst = a.dst[3]; ldc = a.ldc[3]; }
        const int cs = sg == 0 ? a.seg_start[0] : sg == 1 ? a.seg_start[1] : sg == 2 ? a.seg_start[2] : a.seg_start[3];
        const int c0 = sg == 0 ? a.c0[0] : sg == 1 ? a.c0[1] : sg == 2 ? a.c0[2] : a.c0[3];
        dst += c0 + (col - cs);
        const float b = bias[col];
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const int m = m0 + wm * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (m < M) dst[(int64_t)m * ldc] = fmaxf(acc[i][j][e] + b, 0.f);
            }
    }
}

// ---- pools -------------------------------------------------------------------------------------------------------------
// max 3x3 stride 2, no padding; writes channels [c0, c0 + C) of a pixel stride ldc (a concat slice)
__global__ __launch_bounds__(256) void inc_maxpool_kernel(const float *__restrict__ in, float *__restrict__ out, int N, int IH,
                                                          int IW, int C, int OH, int OW, int ldc, int c0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C4 = C / 4;
    if (i >= (int64_t)N * OH * OW * C4) return;
    const int c = (int)(i % C4) * 4;
    const int64_t p = i / C4;
    const int ox = (int)(p % OW), oy = (int)((p / OW) % OH), n = (int)(p / ((int64_t)OW * OH));
    const float *b = in + (((int64_t)n * IH + 2 * oy) * IW + 2 * ox) * C + c;
    float4 m = *reinterpret_cast<const float4 *>(b);
#pragma unroll
    for (int dy = 0; dy < 3; dy++)
#pragma unroll
        for (int dx = 0; dx < 3; dx++) {
            const float4 v = *reinterpret_cast<const float4 *>(b + ((int64_t)dy * IW + dx) * C);
            m = make_float4(fmaxf(m.x, v.x), fmaxf(m.y, v.y), fmaxf(m.z, v.z), fmaxf(m.w, v.w));
        }
    float *o = out + p * ldc + c0 + c;
    o[0] = m.x;
    o[1] = m.y;
    o[2] = m.z;
    o[3] = m.w;
}

// average 3x3 stride 1 pad 1, count_include_pad (divisor 9 everywhere), row-major tap order
__global__ __launch_bounds__(256) void inc_avgpool_kernel(const float *__restrict__ in, float *__restrict__ out, int N, int H, int W,
                                                          int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int C4 = C / 4;
    if (i >= (int64_t)N * H * W * C4) return;
    const int c = (int)(i % C4) * 4;
    const int64_t p = i / C4;
    const int x = (int)(p % W), y = (int)((p / W) % H), n = (int)(p / ((int64_t)W * H));
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int dy = -1; dy <= 1; dy++)
        for (int dx = -1; dx <= 1; dx++) {
            const int yy = y + dy, xx = x + dx;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const float4 v = *reinterpret_cast<const float4 *>(in + (((int64_t)n * H + yy) * W + xx) * C + c);
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
    reinterpret_cast<float4 *>(out)[i] = make_float4(s.x / 9.f, s.y / 9.f, s.z / 9.f, s.w / 9.f);
}

// global average over H*W: one thread per (n, c), pixels summed in order
__global__ __launch_bounds__(256) void inc_mean_kernel(const float *__restrict__ in, float *__restrict__ out, int N, int HW, int C) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)N * C) return;
    const int c = (int)(i % C), n = (int)(i / C);
    const float *p = in + (int64_t)n * HW * C + c;
    float s = 0.f;
    for (int q = 0; q < HW; q++) s += p[(int64_t)q * C];
    out[i] = s / (float)HW;
}

// ---- Inception Score: softmax rows and the streamed statistic -----------------------------------------------------------
// same butterfly as wave_sum (common.h): every lane ends with the same bits
__device__ __forceinline__ float is_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ double is_wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wave per row.  Lane l owns the classes l, l + 64, ... and adds them in ascending order; lanes past C hold the identity
// (-inf for the max, 0 for the sums).  p = expf(x - max) / (fp32 sum), s = sum p and h = sum q log q (q = p / s) in fp64.
__global__ __launch_bounds__(256) void is_rows_kernel(const float *__restrict__ logits, float *__restrict__ p, double *__restrict__ s,
                                                      double *__restrict__ h, int M, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= M) return;                                     // wave-uniform
    const float *x = logits + (int64_t)row * C;
    float *pr = p + (int64_t)row * C;
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, x[c]);
    mx = is_wave_max(mx);
    float den = 0.f;
    for (int c = lane; c < C; c += 64) den += expf(x[c] - mx);
    den = wave_sum(den);
    double sv = 0.0;
    for (int c = lane; c < C; c += 64) {
        const float v = expf(x[c] - mx) / den;
        pr[c] = v;
        sv += (double)v;
    }
    sv = is_wave_sum_f64(sv);
    double hv = 0.0;
    for (int c = lane; c < C; c += 64) {
        const float v = pr[c];                                // this thread's own store
        if (v > 0.f) {
            const double q = (double)v / sv;
            hv += q * log(q);
        }
    }
    hv = is_wave_sum_f64(hv);
    if (lane == 0) {
        s[row] = sv;
        h[row] = hv;
    }
}

// One thread per accumulator (split k, column j) of acc [S][2C + 1]: j < C the class sum of p, j < 2C the class sum of
// q = p / s, j = 2C the sum of h.  Global row g = row0 + i belongs to split g / per; the thread adds its split's rows of this
// call in ascending order onto the stored value, so the chain of additions is the same however the sample is cut into calls.
__global__ __launch_bounds__(256) void is_accum_kernel(const float *__restrict__ p, const double *__restrict__ s,
                                                       const double *__restrict__ h, double *__restrict__ acc, int M, int C, int S,
                                                       int64_t row0, int64_t per) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int W = 2 * C + 1;
    if (i >= (int64_t)S * W) return;
    const int j = (int)(i % W);
    const int64_t k = i / W;
    const int64_t lo = k * per > row0 ? k * per - row0 : 0;
    const int64_t hi = (k + 1) * per - row0 < M ? (k + 1) * per - row0 : M;
    if (lo >= hi) return;
    double a = acc[i];
    for (int64_t r = lo; r < hi; r++) {
        if (j < C) a += (double)p[r * C + j];
        else if (j < 2 * C) a += (double)p[r * C + (j - C)] / s[r];
        else a += h[r];
    }
    acc[i] = a;
}

static unsigned inc_grid(int64_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int rick_inc_input_f32(const float *x, float *out, int N, int H, int W, int OH, int OW, void *stream) {
    if (!x || !out || N < 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || ((uintptr_t)out % 16)) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(inc_input_kernel<true>, dim3(inc_grid((int64_t)N * OH * OW)), dim3(256), 0, (hipStream_t)stream, x, out, N,
                       H, W, OH, OW, (float)H / (float)OH, (float)W / (float)OW);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_input_raw_f32(const float *x, float *out, int N, int H, int W, int OH, int OW, void *stream) {
    if (!x || !out || N < 0 || H <= 0 || W <= 0 || OH <= 0 || OW <= 0 || ((uintptr_t)out % 16)) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(inc_input_kernel<false>, dim3(inc_grid((int64_t)N * OH * OW)), dim3(256), 0, (hipStream_t)stream, x, out, N,
                       H, W, OH, OW, (float)H / (float)OH, (float)W / (float)OW);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_conv_f32(const float *in, const float *wpk, const float *bias, const rick_inc_conv *a, void *stream) {
    if (!in || !wpk || !bias || !a) return RICK_EINVAL;
    const rick_inc_conv g = *a;
    if (g.N < 0 || g.IH <= 0 || g.IW <= 0 || g.Ci <= 0 || (g.Ci & 3) || g.KH <= 0 || g.KW <= 0 || g.SH <= 0 || g.SW <= 0 ||
        g.PH < 0 || g.PW < 0 || g.Co <= 0 || g.nseg < 1 || g.nseg > 4 || (g.bn != 64 && g.bn != 128) || g.Cop % g.bn ||
        g.Cop < g.Co)
        return RICK_EINVAL;
    if (g.OH != (g.IH + 2 * g.PH - g.KH) / g.SH + 1 || g.OW != (g.IW + 2 * g.PW - g.KW) / g.SW + 1 || g.OH <= 0 || g.OW <= 0)
        return RICK_EINVAL;
    if (((uintptr_t)in | (uintptr_t)wpk) % 16) return RICK_EINVAL;
    if (g.seg_start[0] != 0) return RICK_EINVAL;
    for (int s = 0; s < 4; s++) {
        if (s < g.nseg) {
            const int end = s + 1 < g.nseg ? g.seg_start[s + 1] : g.Co;
            if (!g.dst[s] || end <= g.seg_start[s] || g.c0[s] < 0 || g.c0[s] + (end - g.seg_start[s]) > g.ldc[s]) return RICK_EINVAL;
        } else if (g.seg_start[s] < g.Co) {
            return RICK_EINVAL;          // unused slots must start at or beyond Co
        }
    }
    if (g.N == 0) return 0;
    const int64_t M = (int64_t)g.N * g.OH * g.OW;
    if (M > 0x7fffffff || (int64_t)g.N * g.IH * g.IW * g.Ci > ((int64_t)1 << 40)) return RICK_EINVAL;
    const dim3 grid((unsigned)cdiv64(M, IC_BM), (unsigned)(g.Cop / g.bn));
    if (g.bn == 128)
        hipLaunchKernelGGL(inc_conv_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, in, wpk, bias, g, nullptr, nullptr);
    else
        hipLaunchKernelGGL(inc_conv_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, in, wpk, bias, g, nullptr, nullptr);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_conv_bwd_f32(const float *gout, const float *wt, const float *mask, const float *add,
                                     const rick_inc_conv *a, void *stream) {
    if (!gout || !wt || !a) return RICK_EINVAL;
    const rick_inc_conv g = *a;
    if (g.N < 0 || g.IH <= 0 || g.IW <= 0 || g.Ci <= 0 || (g.Ci & 3) || g.KH != 3 || g.KW != 3 || g.SH != 1 || g.SW != 1 ||
        g.PH != 1 || g.PW != 1 || g.OH != g.IH || g.OW != g.IW || g.Co <= 0 || g.nseg != 1 || (g.bn != 64 && g.bn != 128) ||
        g.Cop % g.bn || g.Cop < g.Co)
        return RICK_EINVAL;
    if (g.seg_start[0] != 0 || g.seg_start[1] < g.Co || g.seg_start[2] < g.Co || g.seg_start[3] < g.Co || !g.dst[0] ||
        g.c0[0] != 0 || g.ldc[0] != g.Co)
        return RICK_EINVAL;                  // mask and add share the output's [M, Co] layout
    if (((uintptr_t)gout | (uintptr_t)wt) % 16) return RICK_EINVAL;
    if (g.N == 0) return 0;
    const int64_t M = (int64_t)g.N * g.OH * g.OW;
    if (M > 0x7fffffff || (int64_t)g.N * g.IH * g.IW * g.Ci > ((int64_t)1 << 40)) return RICK_EINVAL;
    const dim3 grid((unsigned)cdiv64(M, IC_BM), (unsigned)(g.Cop / g.bn));
    if (g.bn == 128)
        hipLaunchKernelGGL((inc_conv_kernel<2, true>), grid, dim3(256), 0, (hipStream_t)stream, gout, wt, nullptr, g, mask, add);
    else
        hipLaunchKernelGGL((inc_conv_kernel<1, true>), grid, dim3(256), 0, (hipStream_t)stream, gout, wt, nullptr, g, mask, add);
    RICK_LAUNCH_STATUS();
}

// what the one-destination epilogues (rick_inc_conv_lin_f32, rick_inc_conv_vit_f32) accept of a descriptor and its operands
static int inc_lin_domain(const float *in, const float *wpk, const rick_inc_conv &g) {
    if (g.N < 0 || g.IH <= 0 || g.IW <= 0 || g.Ci <= 0 || (g.Ci & 3) || g.KH <= 0 || g.KW <= 0 || g.SH <= 0 || g.SW <= 0 ||
        g.PH < 0 || g.PW < 0 || g.Co <= 0 || g.nseg != 1 || (g.bn != 64 && g.bn != 128) || g.Cop % g.bn || g.Cop < g.Co)
        return RICK_EINVAL;
    if (g.OH != (g.IH + 2 * g.PH - g.KH) / g.SH + 1 || g.OW != (g.IW + 2 * g.PW - g.KW) / g.SW + 1 || g.OH <= 0 || g.OW <= 0)
        return RICK_EINVAL;
    if (((uintptr_t)in | (uintptr_t)wpk) % 16) return RICK_EINVAL;
    if (g.seg_start[0] != 0 || g.seg_start[1] < g.Co || g.seg_start[2] < g.Co || g.seg_start[3] < g.Co || !g.dst[0] ||
        g.c0[0] < 0 || g.c0[0] + g.Co > g.ldc[0])
        return RICK_EINVAL;
    if ((int64_t)g.N * g.OH * g.OW > 0x7fffffff || (int64_t)g.N * g.IH * g.IW * g.Ci > ((int64_t)1 << 40)) return RICK_EINVAL;
    return 0;
}
static dim3 inc_lin_grid(const rick_inc_conv &g) {
    return dim3((unsigned)cdiv64((int64_t)g.N * g.OH * g.OW, IC_BM), (unsigned)(g.Cop / g.bn));
}

extern "C" int rick_inc_conv_lin_f32(const float *in, const float *wpk, const float *bias, const float *res, int act,
                                     const rick_inc_conv *a, void *stream) {
    if (!in || !wpk || !bias || !a || (act != 0 && act != 1)) return RICK_EINVAL;
    const rick_inc_conv g = *a;
    if (inc_lin_domain(in, wpk, g)) return RICK_EINVAL;
    if (g.N == 0) return 0;
    const dim3 grid = inc_lin_grid(g);
    hipStream_t st = (hipStream_t)stream;
    if (g.bn == 128 && act)
        hipLaunchKernelGGL((inc_conv_kernel<2, false, 2>), grid, dim3(256), 0, st, in, wpk, bias, g, nullptr, res);
    else if (g.bn == 128)
        hipLaunchKernelGGL((inc_conv_kernel<2, false, 1>), grid, dim3(256), 0, st, in, wpk, bias, g, nullptr, res);
    else if (act)
        hipLaunchKernelGGL((inc_conv_kernel<1, false, 2>), grid, dim3(256), 0, st, in, wpk, bias, g, nullptr, res);
    else
        hipLaunchKernelGGL((inc_conv_kernel<1, false, 1>), grid, dim3(256), 0, st, in, wpk, bias, g, nullptr, res);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_conv_vit_f32(const float *in, const float *wpk, const float *bias, const float *scale, const float *res,
                                     int act, const rick_inc_conv *a, void *stream) {
    if (!in || !wpk || !bias || !a || (act != 0 && act != 1)) return RICK_EINVAL;
    const rick_inc_conv g = *a;
    if (inc_lin_domain(in, wpk, g)) return RICK_EINVAL;
    if (g.N == 0) return 0;
    const dim3 grid = inc_lin_grid(g);
    hipStream_t st = (hipStream_t)stream;
    if (g.bn == 128 && act)
        hipLaunchKernelGGL((inc_conv_kernel<2, false, 4>), grid, dim3(256), 0, st, in, wpk, bias, g, scale, res);
    else if (g.bn == 128)
        hipLaunchKernelGGL((inc_conv_kernel<2, false, 3>), grid, dim3(256), 0, st, in, wpk, bias, g, scale, res);
    else if (act)
        hipLaunchKernelGGL((inc_conv_kernel<1, false, 4>), grid, dim3(256), 0, st, in, wpk, bias, g, scale, res);
    else
        hipLaunchKernelGGL((inc_conv_kernel<1, false, 3>), grid, dim3(256), 0, st, in, wpk, bias, g, scale, res);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_maxpool_f32(const float *in, float *out, int N, int IH, int IW, int C, int ldc, int c0, void *stream) {
    if (!in || !out || N < 0 || IH < 3 || IW < 3 || C <= 0 || (C & 3) || c0 < 0 || c0 + C > ldc) return RICK_EINVAL;
    if ((uintptr_t)in % 16) return RICK_EINVAL;
    const int OH = (IH - 3) / 2 + 1, OW = (IW - 3) / 2 + 1;
    if (N == 0) return 0;
    hipLaunchKernelGGL(inc_maxpool_kernel, dim3(inc_grid((int64_t)N * OH * OW * (C / 4))), dim3(256), 0, (hipStream_t)stream, in,
                       out, N, IH, IW, C, OH, OW, ldc, c0);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_avgpool_f32(const float *in, float *out, int N, int H, int W, int C, void *stream) {
    if (!in || !out || N < 0 || H <= 0 || W <= 0 || C <= 0 || (C & 3) || (((uintptr_t)in | (uintptr_t)out) % 16)) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(inc_avgpool_kernel, dim3(inc_grid((int64_t)N * H * W * (C / 4))), dim3(256), 0, (hipStream_t)stream, in,
                       out, N, H, W, C);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_inc_mean_f32(const float *in, float *out, int N, int HW, int C, void *stream) {
    if (!in || !out || N < 0 || HW <= 0 || C <= 0) return RICK_EINVAL;
    if (N == 0) return 0;
    hipLaunchKernelGGL(inc_mean_kernel, dim3(inc_grid((int64_t)N * C)), dim3(256), 0, (hipStream_t)stream, in, out, N, HW, C);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_is_rows_f32(const float *logits, float *p, double *s, double *h, int M, int C, void *stream) {
    if (!logits || !p || !s || !h || M < 0 || C < 1) return RICK_EINVAL;
    if (M == 0) return 0;
    hipLaunchKernelGGL(is_rows_kernel, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, (hipStream_t)stream, logits, p, s, h, M, C);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_is_accum_f64(const float *p, const double *s, const double *h, double *acc, int M, int C, int S, int64_t row0,
                                 int64_t per, void *stream) {
    if (!p || !s || !h || !acc || M < 0 || C < 1 || C > (1 << 29) || S < 1 || row0 < 0 || per < 1) return RICK_EINVAL;
    if (M == 0) return 0;
    hipLaunchKernelGGL(is_accum_kernel, dim3(inc_grid((int64_t)S * (2 * C + 1))), dim3(256), 0, (hipStream_t)stream, p, s, h, acc, M,
                       C, S, row0, per);
    RICK_LAUNCH_STATUS();
}
