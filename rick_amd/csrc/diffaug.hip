// Differentiable Augmentation (color, translation, cutout) — include/rick_hip.h "DiffAugment".  Per image, with the draws b, s, c,
// (tr, tc) and the cut rectangle in a device parameter block:
//     y = Cut . Shift . (L x + b 1),      L x = (c s) x + c (1 - s) mean_ch(x) + (1 - c) mean_all(x)
// (brightness, saturation and contrast collapse to this one affine map; L is self-adjoint), and its adjoint
//     gx = L . Shift^T . Cut . gy.
// Either direction is two launches: the per-image sum behind mean_all (fp64 partials, fixed order), then one elementwise pass
// that writes every output element once.  No atomics; an image's result depends on that image alone.
#include "common.h"

#define DA_CHUNK 4096          // elements of an image's 3 H W per 256-thread block of the sum launch (as EWC_CHUNK, ewc.hip)
#define DA_PIX 1024            // pixels per 256-thread block of the elementwise launch: four per thread, three channels each
#define DA_MAXDIM (1 << 14)    // H, W <= 16384: 3 H W fits an int

// An image's geometry with every field forced into the image: whatever the parameter block holds, no index leaves [0, H) x [0, W)
// (rick_diffaug_check_params rejects such a block on the host; the kernels stay memory-safe without it).
struct da_geom {
    int tr, tc, r0, r1, c0, c1;
};

__device__ __forceinline__ da_geom da_load_geom(const rick_diffaug_param &p, int H, int W) {
    da_geom g;
    g.tr = max(-H, min(H, p.tr));
    g.tc = max(-W, min(W, p.tc));
    g.r0 = max(0, min(H, p.r0));
    g.r1 = max(0, min(H, p.r1));
    g.c0 = max(0, min(W, p.c0));
    g.c1 = max(0, min(W, p.c1));
    return g;
}

// Is (r, q) of the OUTPUT of the forward map live: its source (r + tr, q + tc) inside the image and (r, q) outside the cut.
// The same predicate says which elements of gy the adjoint reads.
__device__ __forceinline__ bool da_live(const da_geom &g, int r, int q, int H, int W) {
    const bool inb = (unsigned)(r + g.tr) < (unsigned)H && (unsigned)(q + g.tc) < (unsigned)W;
    const bool cut = r >= g.r0 && r < g.r1 && q >= g.c0 && q < g.c1;
    return inb && !cut;
}

// Launch 1: partials[n * nb + b] = the fp64 sum of block b's elements of image n — all of them (forward), or the live ones
// (ADJ: the sum of Shift^T Cut gy).  Block b owns the elements [b DA_CHUNK, min(3 H W, (b + 1) DA_CHUNK)) of the image: a function
// of H and W alone.  vec: groups of four with 16-byte loads (group k to thread k % 256), else element j to thread j % 256; a thread
// adds its elements in ascending index order.
template <bool ADJ>
__global__ __launch_bounds__(256) void da_sum_kernel(const float *__restrict__ x, const rick_diffaug_param *__restrict__ params,
                                                     double *__restrict__ partials, int H, int W, int vec) {
    __shared__ double red[4];
    const int n = blockIdx.y, P = H * W, total = 3 * P;
    const int s = blockIdx.x * DA_CHUNK;
    const int len = min(DA_CHUNK, total - s);
    const float *xi = x + (int64_t)n * total + s;
    da_geom g = {};
    if (ADJ) g = da_load_geom(params[n], H, W);
    double acc = 0.0;
    if (vec) {                                   // W % 4 == 0: total and s are multiples of four, a group lies in one row
        const int ngroups = len >> 2;
#pragma unroll 4
        for (int k = threadIdx.x; k < ngroups; k += 256) {
            const float4 v = *reinterpret_cast<const float4 *>(xi + 4 * k);
            if (ADJ) {
                const int pix = (s + 4 * k) % P;
                const int r = pix / W, q = pix - r * W;
                if (da_live(g, r, q, H, W)) acc += (double)v.x;
                if (da_live(g, r, q + 1, H, W)) acc += (double)v.y;
                if (da_live(g, r, q + 2, H, W)) acc += (double)v.z;
                if (da_live(g, r, q + 3, H, W)) acc += (double)v.w;
            } else {
                acc += (double)v.x;
                acc += (double)v.y;
                acc += (double)v.z;
                acc += (double)v.w;
            }
        }
    } else {
        for (int j = threadIdx.x; j < len; j += 256) {
            if (ADJ) {
                const int pix = (s + j) % P;
                const int r = pix / W, q = pix - r * W;
                if (!da_live(g, r, q, H, W)) continue;
            }
            acc += (double)xi[j];
        }
    }
    acc = block_sum_256_f64(acc, red);
    if (threadIdx.x == 0) partials[(int64_t)n * gridDim.x + blockIdx.x] = acc;
}

// One pixel, three channels.  THE PINNED ORDER (the tests' error bound is derived from it):
//     m   = ((v0 + v1) + v2) / 3                       fp32, three roundings
//     out = fma(c s, v_ch, fma(c (1 - s), m, t))       fp32, two roundings;  c s and c (1 - s) are fp32 products (1 - s is exact
//                                                      to one rounding), t is rounded once from fp64
__device__ __forceinline__ void da_pixel(float v0, float v1, float v2, float cs, float c1s, float t, float &o0, float &o1,
                                         float &o2) {
#pragma clang fp contract(off)
    const float m = ((v0 + v1) + v2) / 3.0f;
    const float base = __builtin_fmaf(c1s, m, t);
    o0 = __builtin_fmaf(cs, v0, base);
    o1 = __builtin_fmaf(cs, v1, base);
    o2 = __builtin_fmaf(cs, v2, base);
}

// Launch 2.  Thread 0 of every block re-adds its image's nb partials in ascending order, forms mean = sum / (3 H W) and
// t = (1 - c) * mean + b in fp64 (b only in the forward with bias) and rounds t once to fp32.  Then every output element is written
// exactly once:
//   forward   out[ch, r, q] = live(r, q) ? pixel(x[:, r + tr, q + tc])[ch] : 0          (the fill and the cut are exact zeros)
//   ADJ       gx[ch, r, q]  = pixel(live(r - tr, q - tc) ? gy[:, r - tr, q - tc] : 0)[ch]
// vec (W % 4 == 0, 16-byte aligned images): a thread owns four consecutive pixels of a row, stores three float4 and loads three
// float4 when the column shift is a multiple of four (the group is then inside or outside the image as a whole), single floats
// otherwise; without vec a thread owns the pixels tid, tid + 256, ... of the block's DA_PIX.
template <bool ADJ>
__global__ __launch_bounds__(256) void da_apply_kernel(const float *__restrict__ in, const rick_diffaug_param *__restrict__ params,
                                                       const double *__restrict__ partials, float *__restrict__ out, int H, int W,
                                                       int nb, int bias, int vec) {
    __shared__ float t_sh;
    __shared__ double part_sh[256];
    const int n = blockIdx.y, P = H * W;
    const rick_diffaug_param prm = params[n];
    const da_geom g = da_load_geom(prm, H, W);
    // the partials come through LDS 256 at a time (one load per thread, all in flight together); the ADDITIONS are thread 0's alone
    double sum = 0.0;
    for (int k0 = 0; k0 < nb; k0 += 256) {
        if (k0 + (int)threadIdx.x < nb) part_sh[threadIdx.x] = partials[(int64_t)n * nb + k0 + threadIdx.x];
        __syncthreads();
        if (threadIdx.x == 0) {
            const int cnt = min(256, nb - k0);
#pragma unroll 8
            for (int k = 0; k < cnt; ++k) sum += part_sh[k];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
#pragma clang fp contract(off)
        const double mean = sum / (3.0 * (double)P);
        double t = (1.0 - (double)prm.c) * mean;
        if (!ADJ && bias) t = t + (double)prm.b;
        t_sh = (float)t;
    }
    __syncthreads();
    const float t = t_sh;
    const float cs = prm.c * prm.s, c1s = prm.c * (1.0f - prm.s);
    const int dr = ADJ ? -g.tr : g.tr, dc = ADJ ? -g.tc : g.tc;          // source = destination + (dr, dc)
    const float *in0 = in + (int64_t)n * 3 * P;
    float *out0 = out + (int64_t)n * 3 * P;
    if (vec) {
        const int p0 = (blockIdx.x * 256 + threadIdx.x) * 4;
        if (p0 >= P) return;
        const int r = p0 / W, q = p0 - r * W;
        const int sr = r + dr, sq = q + dc;
        float v[3][4], o[3][4];
        const bool row_in = (unsigned)sr < (unsigned)H;
        if ((dc & 3) == 0) {
            if (row_in && (unsigned)sq < (unsigned)W) {
                const int so = sr * W + sq;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) {
                    const float4 f = *reinterpret_cast<const float4 *>(in0 + ch * P + so);
                    v[ch][0] = f.x, v[ch][1] = f.y, v[ch][2] = f.z, v[ch][3] = f.w;
                }
            } else {
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][0] = v[ch][1] = v[ch][2] = v[ch][3] = 0.f;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = row_in && (unsigned)(sq + e) < (unsigned)W;
                const int so = ok ? sr * W + sq + e : 0;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) v[ch][e] = ok ? in0[ch * P + so] : 0.f;
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (ADJ) {                           // the source pixel of gy must be live in gy's own coordinates
                if (!da_live(g, sr, sq + e, H, W)) v[0][e] = v[1][e] = v[2][e] = 0.f;
            }
            da_pixel(v[0][e], v[1][e], v[2][e], cs, c1s, t, o[0][e], o[1][e], o[2][e]);
            if (!ADJ) {
                if (!da_live(g, r, q + e, H, W)) o[0][e] = o[1][e] = o[2][e] = 0.f;
            }
        }
#pragma unroll
        for (int ch = 0; ch < 3; ++ch)
            *reinterpret_cast<float4 *>(out0 + ch * P + p0) = make_float4(o[ch][0], o[ch][1], o[ch][2], o[ch][3]);
        return;
    }
    const int pend = min(P, (int)(blockIdx.x + 1) * DA_PIX);
    for (int p = blockIdx.x * DA_PIX + threadIdx.x; p < pend; p += 256) {
        const int r = p / W, q = p - r * W;
        const int sr = r + dr, sq = q + dc;
        bool ok = (unsigned)sr < (unsigned)H && (unsigned)sq < (unsigned)W;
        if (ADJ) ok = ok && da_live(g, sr, sq, H, W);
        const int so = ok ? sr * W + sq : 0;
        const float v0 = ok ? in0[so] : 0.f, v1 = ok ? in0[P + so] : 0.f, v2 = ok ? in0[2 * P + so] : 0.f;
        float o0, o1, o2;
        da_pixel(v0, v1, v2, cs, c1s, t, o0, o1, o2);
        if (!ADJ) {
            if (!da_live(g, r, q, H, W)) o0 = o1 = o2 = 0.f;
        }
        out0[p] = o0;
        out0[P + p] = o1;
        out0[2 * P + p] = o2;
    }
}

static int da_blocks(int H, int W) { return cdiv(3 * H * W, DA_CHUNK); }

static int da_check_args(const void *a, const void *prm, const void *ws, const void *b, int N, int H, int W) {
    if (!a || !prm || !ws || !b || N < 1 || H < 1 || W < 1 || H > DA_MAXDIM || W > DA_MAXDIM || N > 65535) return RICK_EINVAL;
    if (((uintptr_t)a % 4) || ((uintptr_t)b % 4) || ((uintptr_t)prm % 4) || ((uintptr_t)ws % 8)) return RICK_EINVAL;
    return 0;
}

template <bool ADJ>
static int da_launch(const float *in, const rick_diffaug_param *params, void *ws, float *out, int N, int H, int W, int bias,
                     void *stream) {
    if (int e = da_check_args(in, params, ws, out, N, H, W)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int nb = da_blocks(H, W);
    // an image is 3 H W floats: with W % 4 == 0 every image, plane, row and group of four starts on a 16-byte boundary
    const int vec = (W % 4 == 0) && ((uintptr_t)in % 16 == 0) && ((uintptr_t)out % 16 == 0);
    hipLaunchKernelGGL(da_sum_kernel<ADJ>, dim3((unsigned)nb, (unsigned)N), dim3(256), 0, st, in, params, (double *)ws, H, W, vec);
    hipLaunchKernelGGL(da_apply_kernel<ADJ>, dim3((unsigned)cdiv(H * W, DA_PIX), (unsigned)N), dim3(256), 0, st, in, params,
                       (const double *)ws, out, H, W, nb, bias, vec);
    RICK_LAUNCH_STATUS();
}

extern "C" int64_t rick_diffaug_workspace_bytes(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || H > DA_MAXDIM || W > DA_MAXDIM) return -1;
    return (int64_t)N * da_blocks(H, W) * (int64_t)sizeof(double);
}

extern "C" int rick_diffaug_check_params(const rick_diffaug_param *host_params, int N, int H, int W) {
    if (!host_params || N < 1 || H < 1 || W < 1) return RICK_EINVAL;
    for (int n = 0; n < N; ++n) {
        const rick_diffaug_param &p = host_params[n];
        if (!(p.b == p.b && p.s == p.s && p.c == p.c)) return RICK_EINVAL;
        if (p.tr <= -H || p.tr >= H || p.tc <= -W || p.tc >= W) return RICK_EINVAL;
        if (p.r0 < 0 || p.r0 > H || p.r1 < 0 || p.r1 > H || p.c0 < 0 || p.c0 > W || p.c1 < 0 || p.c1 > W) return RICK_EINVAL;
    }
    return 0;
}

extern "C" int rick_diffaug_fwd_f32(const float *x, const rick_diffaug_param *params, void *ws, float *out, int N, int H, int W,
                                    int bias, void *stream) {
    return da_launch<false>(x, params, ws, out, N, H, W, bias, stream);
}

extern "C" int rick_diffaug_adj_f32(const float *gy, const rick_diffaug_param *params, void *ws, float *gx, int N, int H, int W,
                                    void *stream) {
    return da_launch<true>(gy, params, ws, gx, N, H, W, 0, stream);
}
