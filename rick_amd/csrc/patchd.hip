// The patch-level discriminator head — include/rick_hip.h "Patch head".  CDC's patch discriminator (rick_amd/patchd.py) puts a
// 3x3 convolution to ONE output channel, a bias and a LeakyReLU on a 512-channel feature map of 16^2 or 32^2 pixels.  As an
// implicit GEMM that is an output tile with one live column, a second launch for the activation and three for the backward
// pass; here it is a dot product per pixel over 9 C values, read as they lie in the channels-last map: one launch forward, one
// pass over x and a small second stage backward.  No atomics: every output element has one writer and a fixed summation order.
#include "common.h"

#define PH_MAXC 2048
#define PH_FWD_PIX 8           // output pixels per forward block: two per wave
#define PH_SLAB0 32            // pixels per backward slab at small maps: eight per wave
#define PH_MAX_SLABS 512       // above 32 * 512 pixels the slabs grow instead (the second stage adds them serially)
#define PH_CHUNK 256           // channels per backward block: one float4 per lane

// Slab length (a multiple of 32 pixels) and count: functions of the pixel count N H W alone.
__host__ __device__ static inline int64_t ph_slab_len(int64_t npix) { return PH_SLAB0 * cdiv64(npix, (int64_t)PH_SLAB0 * PH_MAX_SLABS); }
static inline int64_t ph_nslabs(int64_t npix) { return cdiv64(npix, ph_slab_len(npix)); }
static inline int ph_nchunks(int C) { return cdiv(C, PH_CHUNK); }

// ---- forward: out[p] = gain * lrelu(b + sum_t sum_c (wscale w[c][t]) x[p + tap t][c]) ------------------------------------------
// One wave per output pixel.  Lane l owns the channels 4 l + 256 k + {0, 1, 2, 3} (k ascending) and keeps one fp32 FMA chain per
// tap over them in that order; the lane adds its nine chains in ascending tap order (a tap outside the image loads nothing and
// contributes its chain's initial zero), the 32, 16, ..., 1 xor butterfly adds the lanes, then the bias.  The order is a function
// of C and of the pixel's position in ITS image: an image's output depends neither on N nor on where the image lies in the batch.
// The 9 C scaled weights are staged once per block in LDS as sw[t][c] (dynamic, 36 C bytes: the only LDS of the kernel, so its
// base is 16-byte aligned) and read back with ds_read_b128.
__global__ __launch_bounds__(256) void patch_head_fwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ b, float *__restrict__ out, int64_t npix,
                                                             int H, int W, int C, float wscale, float slope, float gain) {
    extern __shared__ __attribute__((aligned(16))) float sw[];
    // w[c][t] lies at 9 c + t: 9 C / 4 16-byte loads, several in flight per thread (scalar v_mul_f32: tools/check_isa.py gates
    // this kernel, so the loop is kept away from the vectoriser)
#pragma clang loop vectorize(disable) interleave(disable) unroll_count(5)
    for (int i4 = threadIdx.x; i4 < 9 * C / 4; i4 += 256) {
        const float4 v = *reinterpret_cast<const float4 *>(w + 4 * i4);
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int i = 4 * i4 + j, c = i / 9, t = i - 9 * c;
            sw[t * C + c] = wscale * e[j];
        }
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float bias = b[0];
    const int64_t p0 = (int64_t)blockIdx.x * PH_FWD_PIX;
#pragma unroll
    for (int k = 0; k < PH_FWD_PIX / 4; k++) {              // (unrolled: both pixels' loads are in flight together)
        const int64_t p = p0 + wave + 4 * k;
        if (p >= npix) continue;                            // wave-uniform
        const int xx = (int)(p % W), yy = (int)((p / W) % H);
        bool in[9];
        float a[9];
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
            in[t] = iy >= 0 && iy < H && ix >= 0 && ix < W;                // wave-uniform
            a[t] = 0.f;
        }
        const float *xp = x + p * C;
        for (int c = 4 * lane; c < C; c += 256) {                          // nine independent 16-byte loads in flight per round
#pragma unroll
            for (int t = 0; t < 9; t++) {
                if (!in[t]) continue;
                // (an inside tap lies in the same image: its pixel index is p + dy W + dx)
                const float4 v = *reinterpret_cast<const float4 *>(xp + ((int64_t)(t / 3 - 1) * W + (t % 3 - 1)) * C + c);
                const float4 u = *reinterpret_cast<const float4 *>(sw + t * C + c);
                a[t] = fmaf(u.x, v.x, a[t]);
                a[t] = fmaf(u.y, v.y, a[t]);
                a[t] = fmaf(u.z, v.z, a[t]);
                a[t] = fmaf(u.w, v.w, a[t]);
            }
        }
        float s = a[0];
#pragma unroll
        for (int t = 1; t < 9; t++) s += a[t];
        s = wave_sum(s);
        if (lane == 0) {
            const float z = bias + s;
            out[p] = gain * (z > 0.f ? z : slope * z);
        }
    }
}

// ---- backward, first stage: one pass over x ------------------------------------------------------------------------------------
// Block (slab, chunk): the pixels [slab L, (slab + 1) L) of the flattened N H W map, the channels [256 chunk, 256 chunk + 256).
// Lane l owns the four channels 256 chunk + 4 l + {0, 1, 2, 3} and holds their 36 weights in registers; wave v takes the pixels
// slab L + v + 4 k, k ascending.  For an input pixel (n, u, v) the nine neighbours gz[n][u - ky + 1][v - kx + 1] (zero outside
// the image) are formed from g and the stored output on the fly: gz = g * gain * (out > 0 ? 1 : slope).  Then
//   gX[n][u][v][c]  = sum_t (wscale w[c][t]) gz_t       one fp32 chain, taps ascending; depends on image n alone
//   acc[t][c]      += gz_t x[n][u][v][c]                one fp32 FMA chain per (tap, channel) and wave, pixels ascending
//   gb             += gz[n][u][v]                       (chunk 0 only; one fp64 chain per wave)
// and the four waves are added ((w0 + w1) + w2) + w3 into part[slab][t C + c] (fp32) and part_b[slab] (fp64).  No lane sums.
// ws = part_b [nslabs] doubles, then part [nslabs][9 C] floats.
__device__ __forceinline__ float ph_gz(const float *__restrict__ g, const float *__restrict__ out, int64_t p, float slope, float gain) {
    return g[p] * (gain * (out[p] > 0.f ? 1.f : slope));
}

template <bool WANT_GX>
__global__ __launch_bounds__(256) void patch_head_bwd_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                             const float *__restrict__ g, const float *__restrict__ out,
                                                             float *__restrict__ gx, double *__restrict__ part_b,
                                                             float *__restrict__ part, int64_t npix, int64_t slab_len, int H, int W,
                                                             int C, float wscale, float slope, float gain) {
    __shared__ __attribute__((aligned(16))) float red[4][9][PH_CHUNK];
    __shared__ double redb[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * PH_CHUNK + 4 * lane;
    const bool live = c < C;                               // C % 4 == 0: a lane's four channels are all inside or all outside
    float sw[9][4];
    if (WANT_GX && live) {                                 // w[c .. c + 3][0 .. 8]: 36 consecutive floats, 16-byte aligned
        float4 raw[9];
#pragma unroll
        for (int k = 0; k < 9; k++) raw[k] = *reinterpret_cast<const float4 *>(w + 9 * (int64_t)c + 4 * k);
        const float *r = reinterpret_cast<const float *>(raw);
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int t = 0; t < 9; t++) sw[t][j] = wscale * r[9 * j + t];
    }
    float4 acc[9];
#pragma unroll
    for (int t = 0; t < 9; t++) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    double accb = 0.0;
    const int64_t p0 = (int64_t)blockIdx.x * slab_len, p1 = min(npix, p0 + slab_len);
#pragma unroll 4
    for (int64_t p = p0 + wave; p < p1; p += 4) {           // (unrolled: the loads of four pixels are in flight together)
        const int xx = (int)(p % W), yy = (int)((p / W) % H);
        float gz[9];
#pragma unroll
        for (int t = 0; t < 9; t++) {
            const int oy = yy - (t / 3 - 1), ox = xx - (t % 3 - 1);
            const bool in = oy >= 0 && oy < H && ox >= 0 && ox < W;       // wave-uniform
            gz[t] = in ? ph_gz(g, out, p - (int64_t)(t / 3 - 1) * W - (t % 3 - 1), slope, gain) : 0.f;
        }
        accb += (double)gz[4];
        if (live) {
            const float4 v = *reinterpret_cast<const float4 *>(x + p * C + c);
#pragma unroll
            for (int t = 0; t < 9; t++) {
                acc[t].x = fmaf(gz[t], v.x, acc[t].x);
                acc[t].y = fmaf(gz[t], v.y, acc[t].y);
                acc[t].z = fmaf(gz[t], v.z, acc[t].z);
                acc[t].w = fmaf(gz[t], v.w, acc[t].w);
            }
            if (WANT_GX) {
                float4 o = make_float4(sw[0][0] * gz[0], sw[0][1] * gz[0], sw[0][2] * gz[0], sw[0][3] * gz[0]);
#pragma unroll
                for (int t = 1; t < 9; t++) {
                    o.x = fmaf(sw[t][0], gz[t], o.x);
                    o.y = fmaf(sw[t][1], gz[t], o.y);
                    o.z = fmaf(sw[t][2], gz[t], o.z);
                    o.w = fmaf(sw[t][3], gz[t], o.w);
                }
                *reinterpret_cast<float4 *>(gx + p * C + c) = o;
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 9; t++) *reinterpret_cast<float4 *>(&red[wave][t][4 * lane]) = acc[t];
    if (lane == 0) redb[wave] = accb;
    __syncthreads();
    const int nc = min(PH_CHUNK, C - blockIdx.y * PH_CHUNK);              // live channels of this chunk
    float *row = part + (int64_t)blockIdx.x * 9 * C;
    for (int i = threadIdx.x; i < 9 * PH_CHUNK; i += 256) {
        const int t = i / PH_CHUNK, j = i - t * PH_CHUNK;
        if (j < nc) row[(int64_t)t * C + blockIdx.y * PH_CHUNK + j] = ((red[0][t][j] + red[1][t][j]) + red[2][t][j]) + red[3][t][j];
    }
    if (blockIdx.y == 0 && threadIdx.x == 0) part_b[blockIdx.x] = ((redb[0] + redb[1]) + redb[2]) + redb[3];
}

// ---- backward, second stage: gw[c][t] = wscale * sum over slabs, ascending, in fp64; gb likewise -------------------------------
// Thread i < 9 C takes (t, c) = (i / C, i % C): the threads of a wave read neighbouring floats of every slab's row.
__global__ __launch_bounds__(256) void patch_head_finish_kernel(const double *__restrict__ part_b, const float *__restrict__ part,
                                                                int64_t nslabs, int C, float wscale, float *__restrict__ gw,
                                                                float *__restrict__ gb) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i > 9 * C) return;
    double s = 0.0;
    if (i == 9 * C) {
#pragma unroll 8
        for (int64_t k = 0; k < nslabs; k++) s += part_b[k];
        gb[0] = (float)s;
        return;
    }
#pragma unroll 8
    for (int64_t k = 0; k < nslabs; k++) s += (double)part[k * 9 * C + i];
    const int t = i / C, c = i - t * C;
    gw[9 * c + t] = (float)((double)wscale * s);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
static inline bool ph_shape_ok(int N, int H, int W, int C) {
    return N >= 1 && H >= 1 && W >= 1 && C >= 4 && C <= PH_MAXC && (C & 3) == 0 &&
           (int64_t)N * H * W * C < ((int64_t)1 << 31);
}

extern "C" int64_t rick_patch_head_workspace_bytes(int N, int H, int W, int C) {
    if (!ph_shape_ok(N, H, W, C)) return -1;
    return ph_nslabs((int64_t)N * H * W) * (9 * (int64_t)C * (int64_t)sizeof(float) + (int64_t)sizeof(double));
}

extern "C" int rick_patch_head_fwd_f32(const float *x, const float *w, const float *b, float *out, int N, int H, int W, int C,
                                       float wscale, float slope, float gain, void *stream) {
    if (!x || !w || !b || !out || !ph_shape_ok(N, H, W, C) || (((uintptr_t)x | (uintptr_t)w) % 16) ||
        (((uintptr_t)b | (uintptr_t)out) % 4))
        return RICK_EINVAL;
    const int64_t npix = (int64_t)N * H * W;
    const size_t lds = (size_t)9 * C * sizeof(float);
    if (lds > 64 * 1024) RICK_LDS160_ONCE(patch_head_fwd_kernel);
    hipLaunchKernelGGL(patch_head_fwd_kernel, dim3((unsigned)cdiv64(npix, PH_FWD_PIX)), dim3(256), lds, (hipStream_t)stream, x, w, b,
                       out, npix, H, W, C, wscale, slope, gain);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_patch_head_bwd_f32(const float *x, const float *w, const float *g, const float *out, float *gx, void *ws, int N,
                                       int H, int W, int C, float wscale, float slope, float gain, void *stream) {
    if (!x || !w || !g || !out || !ws || !ph_shape_ok(N, H, W, C) || (((uintptr_t)x | (uintptr_t)w | (uintptr_t)gx) % 16) ||
        (((uintptr_t)g | (uintptr_t)out) % 4) || ((uintptr_t)ws % 8) || gx == x)
        return RICK_EINVAL;
    const int64_t npix = (int64_t)N * H * W, slab_len = ph_slab_len(npix);
    const dim3 grid((unsigned)ph_nslabs(npix), (unsigned)ph_nchunks(C));
    double *part_b = (double *)ws;
    float *part = (float *)(part_b + grid.x);
    if (gx)
        hipLaunchKernelGGL(patch_head_bwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, w, g, out, gx, part_b, part, npix,
                           slab_len, H, W, C, wscale, slope, gain);
    else
        hipLaunchKernelGGL(patch_head_bwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, w, g, out, gx, part_b, part, npix,
                           slab_len, H, W, C, wscale, slope, gain);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_patch_head_bwd_finish_f32(const void *ws, float *gw, float *gb, int N, int H, int W, int C, float wscale,
                                              void *stream) {
    if (!ws || !gw || !gb || !ph_shape_ok(N, H, W, C) || ((uintptr_t)ws % 8) || (((uintptr_t)gw | (uintptr_t)gb) % 4)) return RICK_EINVAL;
    const int64_t nslabs = ph_nslabs((int64_t)N * H * W);
    hipLaunchKernelGGL(patch_head_finish_kernel, dim3((unsigned)cdiv(9 * C + 1, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const double *)ws, (const float *)((const double *)ws + nslabs), nslabs, C, wscale, gw, gb);
    RICK_LAUNCH_STATUS();
}
