// Adaptive discriminator augmentation (non_leaking.py:316-398) as a fixed list of four static-shape kernels: two for the
// forward map and two for its adjoint.
//
// With the per-sample affine G and colour matrix C fixed, the image path of the reference
//     y = C o crop o down12 o warp o up12 o reflect(x)
// is linear in x (plus the colour offset).  The composed path (rick_amd/augment.py) materialises a reflect-padded canvas, a
// 2x up-sampled canvas and a warped canvas whose sizes depend on the batch-maximum pads; here nothing but a warped region of
// static size (2H+10) x (2W+10) per channel is written:
//
//   A   (warp)  for every warped pixel the down FIR of the crop can read, the bilinear sample of the up-sampled, reflect-padded
//               source, evaluated on the fly: each of the 4 bilinear corners is one polyphase 6x6 tap set of the 12x12 sym6
//               FIR over reflect-indexed source pixels;
//   B   (down)  the 12x12 down-2 FIR over A's region, the crop, and the 3x4 colour matrix as an epilogue;
//   Bt          colour transpose and FIR transpose, in gather form (one thread per region pixel);
//   At          gather form: for each source pixel and each of its reflected copies, the 12x12 canvas taps it feeds; the
//               warped pixels whose bilinear corners land there lie in the preimage parallelogram of that canvas box, whose
//               bounding box is enumerated in a fixed order with the forward's own coordinate and floor computation.
//
// No float atomics: every output element is written by one thread that sums in a fixed order, so results are bit-identical
// from run to run.  The zero regions of the reference are reproduced: upfirdn2d pad 0 at the padded-canvas edge (never reached:
// the up FIR only reads inside the padded canvas) and grid_sample(padding_mode='zeros', align_corners=False) at the up-sampled
// canvas edge (a corner outside [0, W2) x [0, H2) contributes 0).  Warp coordinates are evaluated in fp64 (4 FMAs per warped
// pixel), so floor decisions do not depend on fp32 rounding of canvas coordinates of up to ~6H.
//
// Per-call parameters live in DEVICE memory (rick_aug_param[N], include/rick_hip.h): a captured graph replays with new
// transforms after one host-to-device copy into the block.  The pads are per sample: one launch pair serves the D step's
// cat(fake, real), i.e. two reference calls with their own batch-maximum pads.
//
// Layout: planar NCHW fp32, contiguous — the generator's output image (models.py: `skip.contiguous()`), the data batch of
// rick_image_batch_f32 ([B, 3, H, W]) and what the discriminator's input layer reads.
#include "common.h"

// sym6 decomposition low-pass (non_leaking.py:9-22); k2 = outer(taps, taps) rounded to fp32 exactly as torch.outer does
__constant__ float c_sym6[12] = {0.015404109327027373f, 0.0034907120842174702f, -0.11799011114819057f, -0.048311742585633f,
                                 0.4910559419267466f,   0.787641141030194f,     0.3379294217276218f,   -0.07263752278646252f,
                                 -0.021060292512300564f, 0.04472490177066578f,  0.0017677118642428036f, -0.007800708325034148f};

namespace {

constexpr int KT = 12;          // FIR taps per axis
constexpr int PADK = 6;         // (KT + 1) / 2: the reference's extra reflect pad on every side

__device__ __forceinline__ float k2(int a, int b) { return __fmul_rn(c_sym6[a], c_sym6[b]); }

// reflect-index a padded-canvas coordinate (t = u - pad - PADK) into [0, n); pads < n are checked on the host, the clamp only
// keeps a bad parameter block from reading outside the image
__device__ __forceinline__ int reflect_idx(int t, int n) {
    t = t < 0 ? -t : t;
    t = t > n - 1 ? 2 * (n - 1) - t : t;
    return min(max(t, 0), n - 1);
}

// up-sampled canvas coordinates of the bilinear sample of warped region pixel (r, c) — the ONE place they are computed, shared by
// the forward (A) and the adjoint (At) so that both take the same floor decisions
struct WarpPt {
    int x0, y0;
    float fx, fy;
};
__device__ __forceinline__ WarpPt warp_point(const rick_aug_param &p, int r, int c) {
    const double ix = fma(p.a[0], (double)c, fma(p.a[1], (double)r, p.a[2]));
    const double iy = fma(p.a[3], (double)c, fma(p.a[4], (double)r, p.a[5]));
    // |coordinates| beyond 2^30 cannot index a canvas: park them far outside (every corner then fails the bounds test)
    const double fx0 = floor(fmin(fmax(ix, -1e9), 1e9)), fy0 = floor(fmin(fmax(iy, -1e9), 1e9));
    WarpPt w;
    w.x0 = (int)fx0;
    w.y0 = (int)fy0;
    w.fx = (float)(ix - fx0);
    w.fy = (float)(iy - fy0);
    return w;
}

// one value of the 2x up-sampled canvas, 3 channels: up[Y, X] = sum_{a,b} padded[(Y+a)/2, (X+b)/2] k2[a][b] over the taps with
// Y+a, X+b even (6 x 6 polyphase set); rows / cols y-outer, x-inner
__device__ __forceinline__ void up_value(const float *__restrict__ x, int64_t plane, int H, int W, const rick_aug_param &p, int Y, int X,
                                         float v[3]) {
    const int a0 = Y & 1, b0 = X & 1;
    int sx[6];
#pragma unroll
    for (int j = 0; j < 6; j++) sx[j] = reflect_idx((X + b0 + 2 * j) / 2 - p.px1 - PADK, W);
    v[0] = v[1] = v[2] = 0.f;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const int a = a0 + 2 * i;
        const int sy = reflect_idx((Y + a) / 2 - p.py1 - PADK, H);
        const float *row = x + (int64_t)sy * W;
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const float t = k2(a, b0 + 2 * j);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) v[ch] = fmaf(row[ch * plane + sx[j]], t, v[ch]);
        }
    }
}

// A: warped region [N, 3, RH, RW], RH = 2H + 10, RW = 2W + 10; region pixel (r, c) is warped-canvas pixel (2 py1 + r, 2 px1 + c)
__global__ __launch_bounds__(256) void aug_warp_fwd_kernel(const float *__restrict__ x, const rick_aug_param *__restrict__ prm,
                                                           float *__restrict__ wout, int N, int H, int W) {
    const int RH = 2 * H + 10, RW = 2 * W + 10;
    const int64_t total = (int64_t)N * RH * RW, rplane = (int64_t)RH * RW, plane = (int64_t)H * W;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i / rplane);
    const int64_t q = i - (int64_t)n * rplane;
    const int r = (int)(q / RW), c = (int)(q - (int64_t)r * RW);
    const rick_aug_param p = prm[n];
    const int H2 = 2 * p.hp - 11, W2 = 2 * p.wp - 11;
    const WarpPt w = warp_point(p, r, c);
    const float *xs = x + (int64_t)n * 3 * plane;
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int dy = 0; dy < 2; dy++) {
        const int Y = w.y0 + dy;
        if (Y < 0 || Y >= H2) continue;
        const float wy = dy ? w.fy : 1.f - w.fy;
#pragma unroll
        for (int dx = 0; dx < 2; dx++) {
            const int X = w.x0 + dx;
            if (X < 0 || X >= W2) continue;
            const float wt = wy * (dx ? w.fx : 1.f - w.fx);
            float v[3];
            up_value(xs, plane, H, W, p, Y, X, v);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) acc[ch] = fmaf(wt, v[ch], acc[ch]);
        }
    }
    float *o = wout + (int64_t)n * 3 * rplane + q;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch * rplane] = acc[ch];
}

// B: out[n, :, i, j] = col[:, :3] @ (sum_{a,b} warped[2i+a, 2j+b] k2[11-a][11-b]) (+ col[:, 3] when `bias`)
__global__ __launch_bounds__(256) void aug_down_fwd_kernel(const float *__restrict__ win, const rick_aug_param *__restrict__ prm,
                                                           float *__restrict__ out, int N, int H, int W, int bias) {
    const int RH = 2 * H + 10, RW = 2 * W + 10;
    const int64_t plane = (int64_t)H * W, rplane = (int64_t)RH * RW, total = (int64_t)N * plane;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i / plane);
    const int64_t q = i - (int64_t)n * plane;
    const int oy = (int)(q / W), ox = (int)(q - (int64_t)oy * W);
    const float *src = win + (int64_t)n * 3 * rplane + (int64_t)(2 * oy) * RW + 2 * ox;
    float d[3] = {0.f, 0.f, 0.f};
    for (int a = 0; a < KT; a++) {
        const float *row = src + (int64_t)a * RW;
#pragma unroll
        for (int b = 0; b < KT; b++) {
            const float t = k2(KT - 1 - a, KT - 1 - b);
#pragma unroll
            for (int ch = 0; ch < 3; ch++) d[ch] = fmaf(row[ch * rplane + b], t, d[ch]);
        }
    }
    const float *m = prm[n].col;
    float *o = out + (int64_t)n * 3 * plane + q;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float v = bias ? m[ch * 4 + 3] : 0.f;
        v = fmaf(m[ch * 4 + 0], d[0], v);
        v = fmaf(m[ch * 4 + 1], d[1], v);
        v = fmaf(m[ch * 4 + 2], d[2], v);
        o[ch * plane] = v;
    }
}

// Bt: g_region[n, c, r, s] = sum_c' col[c'][c] sum_{i,j: a = r-2i, b = s-2j in [0,12)} gy[n, c', i, j] k2[11-a][11-b]
__global__ __launch_bounds__(256) void aug_down_adj_kernel(const float *__restrict__ gy, const rick_aug_param *__restrict__ prm,
                                                           float *__restrict__ gw, int N, int H, int W) {
    const int RH = 2 * H + 10, RW = 2 * W + 10;
    const int64_t plane = (int64_t)H * W, rplane = (int64_t)RH * RW, total = (int64_t)N * rplane;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i / rplane);
    const int64_t q = i - (int64_t)n * rplane;
    const int r = (int)(q / RW), s = (int)(q - (int64_t)r * RW);
    const float *g = gy + (int64_t)n * 3 * plane;
    // rows i with 0 <= r - 2i <= 11 and 0 <= i < H (likewise columns): at most 6 each
    const int i0 = max(0, (r - KT + 2) / 2), i1 = min(H - 1, r / 2);
    const int j0 = max(0, (s - KT + 2) / 2), j1 = min(W - 1, s / 2);
    float acc[3] = {0.f, 0.f, 0.f};
    for (int ii = i0; ii <= i1; ii++) {
        const int a = r - 2 * ii;
        const float *row = g + (int64_t)ii * W;
        for (int jj = j0; jj <= j1; jj++) {
            const float t = k2(KT - 1 - a, KT - 1 - (s - 2 * jj));
#pragma unroll
            for (int ch = 0; ch < 3; ch++) acc[ch] = fmaf(row[ch * plane + jj], t, acc[ch]);
        }
    }
    const float *m = prm[n].col;
    float *o = gw + (int64_t)n * 3 * rplane + q;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) {
        float v = m[0 * 4 + ch] * acc[0];
        v = fmaf(m[1 * 4 + ch], acc[1], v);
        v = fmaf(m[2 * 4 + ch], acc[2], v);
        o[ch * rplane] = v;
    }
}

// padded-canvas positions u in [0, n + lo + hi + 2*PADK) whose reflect index is s (at most 3: direct, mirrored low, mirrored high)
__device__ __forceinline__ int reflect_copies(int s, int n, int lo, int hi, int u[3]) {
    int k = 0;
    const int lim_lo = -(lo + PADK), lim_hi = n - 1 + hi + PADK;
    u[k++] = s + lo + PADK;
    if (s > 0 && -s >= lim_lo) u[k++] = -s + lo + PADK;
    if (s < n - 1 && 2 * (n - 1) - s <= lim_hi) u[k++] = 2 * (n - 1) - s + lo + PADK;
    return k;
}

// At: gx[n, :, sy, sx] = sum over reflected copies (u, v) of the source pixel, over up-sampled canvas pixels (Y, X) with
// a = 2u - Y, b = 2v - X in [0, 12) inside the canvas, of k2[a][b] * (bilinear weight of (Y, X) in warped pixel P) * g_region[P]
__global__ __launch_bounds__(256) void aug_warp_adj_kernel(const float *__restrict__ gw, const rick_aug_param *__restrict__ prm,
                                                           float *__restrict__ gx, int N, int H, int W) {
    const int RH = 2 * H + 10, RW = 2 * W + 10;
    const int64_t plane = (int64_t)H * W, rplane = (int64_t)RH * RW, total = (int64_t)N * plane;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int n = (int)(i / plane);
    const int64_t q = i - (int64_t)n * plane;
    const int sy = (int)(q / W), sx = (int)(q - (int64_t)sy * W);
    const rick_aug_param p = prm[n];
    const int H2 = 2 * p.hp - 11, W2 = 2 * p.wp - 11;
    const int py2 = p.hp - H - p.py1 - 2 * PADK, px2 = p.wp - W - p.px1 - 2 * PADK;
    int us[3], vs[3];
    const int nu = reflect_copies(sy, H, p.py1, py2, us), nv = reflect_copies(sx, W, p.px1, px2, vs);
    const float *g = gw + (int64_t)n * 3 * rplane;
    float acc[3] = {0.f, 0.f, 0.f};
    for (int cu = 0; cu < nu; cu++) {
        const int Ylo = max(0, 2 * us[cu] - (KT - 1)), Yhi = min(H2 - 1, 2 * us[cu]);
        if (Ylo > Yhi) continue;
        for (int cv = 0; cv < nv; cv++) {
            const int Xlo = max(0, 2 * vs[cv] - (KT - 1)), Xhi = min(W2 - 1, 2 * vs[cv]);
            if (Xlo > Xhi) continue;
            // warped pixels with a corner in [Xlo, Xhi] x [Ylo, Yhi] sample at ix in [Xlo-1, Xhi+1), iy in [Ylo-1, Yhi+1): the
            // bounding box of that rectangle's preimage (+1 pixel of margin for rounding), clipped to the region
            double cmin = 1e30, cmax = -1e30, rmin = 1e30, rmax = -1e30;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const double ex = ((k & 1) ? Xhi + 1 : Xlo - 1) - p.a[2], ey = ((k & 2) ? Yhi + 1 : Ylo - 1) - p.a[5];
                const double cc = p.ainv[0] * ex + p.ainv[1] * ey, rr = p.ainv[2] * ex + p.ainv[3] * ey;
                cmin = fmin(cmin, cc); cmax = fmax(cmax, cc);
                rmin = fmin(rmin, rr); rmax = fmax(rmax, rr);
            }
            const int c0 = (int)fmax(floor(cmin) - 1, 0.0), c1 = (int)fmin(ceil(cmax) + 1, (double)(RW - 1));
            const int r0 = (int)fmax(floor(rmin) - 1, 0.0), r1 = (int)fmin(ceil(rmax) + 1, (double)(RH - 1));
            for (int r = r0; r <= r1; r++) {
                for (int c = c0; c <= c1; c++) {
                    const WarpPt w = warp_point(p, r, c);
                    if (w.y0 + 1 < Ylo || w.y0 > Yhi || w.x0 + 1 < Xlo || w.x0 > Xhi) continue;
                    float wsum = 0.f;          // sum over the corners that land in the tap box of (bilinear weight * k2)
#pragma unroll
                    for (int dy = 0; dy < 2; dy++) {
                        const int Y = w.y0 + dy;
                        if (Y < Ylo || Y > Yhi) continue;
                        const float wy = dy ? w.fy : 1.f - w.fy;
#pragma unroll
                        for (int dx = 0; dx < 2; dx++) {
                            const int X = w.x0 + dx;
                            if (X < Xlo || X > Xhi) continue;
                            const float wt = wy * (dx ? w.fx : 1.f - w.fx);
                            wsum = fmaf(wt, k2(2 * us[cu] - Y, 2 * vs[cv] - X), wsum);
                        }
                    }
                    const int64_t o = (int64_t)r * RW + c;
#pragma unroll
                    for (int ch = 0; ch < 3; ch++) acc[ch] = fmaf(wsum, g[ch * rplane + o], acc[ch]);
                }
            }
        }
    }
    float *o = gx + (int64_t)n * 3 * plane + q;
#pragma unroll
    for (int ch = 0; ch < 3; ch++) o[ch * plane] = acc[ch];
}

int check_args(const void *a, const void *prm, const void *ws, const void *b, int N, int H, int W) {
    // the reference needs H, W > pad + 6 for its reflect pad; a 7-pixel image is the smallest that admits a zero pad
    if (!a || !prm || !ws || !b || N < 1 || H < PADK + 1 || W < PADK + 1 || H > (1 << 14) || W > (1 << 14)) return RICK_EINVAL;
    return 0;
}

}  // namespace

extern "C" int64_t rick_augment_workspace_floats(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return -1;
    return (int64_t)N * 3 * (2 * H + 10) * (2 * W + 10);
}

extern "C" int rick_augment_fwd_f32(const float *x, const rick_aug_param *params, float *ws, float *out, int N, int H, int W, int bias,
                                    void *stream) {
    if (int e = check_args(x, params, ws, out, N, H, W)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nr = rick_augment_workspace_floats(N, H, W) / 3, no = (int64_t)N * H * W;
    hipLaunchKernelGGL(aug_warp_fwd_kernel, dim3((unsigned)cdiv64(nr, 256)), dim3(256), 0, st, x, params, ws, N, H, W);
    hipLaunchKernelGGL(aug_down_fwd_kernel, dim3((unsigned)cdiv64(no, 256)), dim3(256), 0, st, ws, params, out, N, H, W, bias);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_augment_adj_f32(const float *gy, const rick_aug_param *params, float *ws, float *gx, int N, int H, int W,
                                    void *stream) {
    if (int e = check_args(gy, params, ws, gx, N, H, W)) return e;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nr = rick_augment_workspace_floats(N, H, W) / 3, no = (int64_t)N * H * W;
    hipLaunchKernelGGL(aug_down_adj_kernel, dim3((unsigned)cdiv64(nr, 256)), dim3(256), 0, st, gy, params, ws, N, H, W);
    hipLaunchKernelGGL(aug_warp_adj_kernel, dim3((unsigned)cdiv64(no, 256)), dim3(256), 0, st, ws, params, gx, N, H, W);
    RICK_LAUNCH_STATUS();
}
