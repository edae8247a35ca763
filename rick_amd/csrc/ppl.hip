// Perceptual path length: the latent path points — include/rick_hip.h "PPL", rick_amd/ppl.py.
//
// One wave per pair (a_i, b_i): lane l holds elements l + 64 j (j ascending, at most 16 for L <= 1024) of both rows in registers
// and writes rows 2i (the point at t_i) and 2i + 1 (the point at t_i + eps) of the output.  Every sum is a per-lane FMA chain in
// j order followed by the fixed 32, 16, ..., 1 xor butterfly (wave_sum_f64): no atomics, run-to-run identical, and a pair's two
// rows depend on that pair alone.
//
// The arithmetic between the fp32 loads and the fp32 stores is fp64.  PPL divides the LPIPS of the two rows by eps^2, so what
// matters is the DIFFERENCE of the rows, eps (1e-4) times smaller than the rows: in fp32 the angle p = t acos(d) carries 1e-7 of
// itself into both rows, 1e-3 of their difference, and d near 1 (nearly parallel latents) loses half its digits in acos.  With
// 3 L fp64 FMAs per wave next to a launch the kernel is latency bound either way; each output is the correctly rounded fp32 of
// a value that is exact to ~1e-15.
#include "common.h"

#pragma clang fp contract(off)

#define PPL_MAXL 1024
#define PPL_PER (PPL_MAXL / 64)

__global__ __launch_bounds__(256) void ppl_latents_kernel(const float *__restrict__ a, const float *__restrict__ b,
                                                          const float *__restrict__ t, double eps, float *__restrict__ out, int B,
                                                          int L, int mode) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= B) return;                                                // wave-uniform
    const float *ar = a + i * L, *br = b + i * L;
    float *o0 = out + 2 * i * L, *o1 = o0 + L;
    const double t0 = (double)t[i], t1 = t0 + eps;
    double x[PPL_PER], y[PPL_PER];
#pragma unroll
    for (int j = 0; j < PPL_PER; j++) {
        const int k = lane + 64 * j;
        x[j] = k < L ? (double)ar[k] : 0.0;
        y[j] = k < L ? (double)br[k] : 0.0;
    }
    if (mode == 0) {                                                   // lerp: a + (b - a) t, both rows from the same fp32 d
#pragma unroll
        for (int j = 0; j < PPL_PER; j++) {
            const int k = lane + 64 * j;
            if (k < L) {
                const double d = (double)__fsub_rn((float)y[j], (float)x[j]);
                o0[k] = (float)fma(d, t0, x[j]);
                o1[k] = (float)fma(d, t1, x[j]);
            }
        }
        return;
    }
    // slerp (stylegan2-pytorch ppl.py): an = a / |a|, bn = b / |b|, d = clamp(an . bn), p = t acos(d),
    // c = normalize(bn - d an), out = normalize(an cos p + c sin p); normalize divides by max(norm, 1e-12)
    double saa = 0.0, sbb = 0.0;
#pragma unroll
    for (int j = 0; j < PPL_PER; j++) {
        saa = fma(x[j], x[j], saa);
        sbb = fma(y[j], y[j], sbb);
    }
    saa = wave_sum_f64(saa);
    sbb = wave_sum_f64(sbb);
    const double ra = 1.0 / fmax(sqrt(saa), 1e-12), rb = 1.0 / fmax(sqrt(sbb), 1e-12);
    double d = 0.0;
#pragma unroll
    for (int j = 0; j < PPL_PER; j++) {
        x[j] *= ra;
        y[j] *= rb;
        d = fma(x[j], y[j], d);
    }
    d = fmin(fmax(wave_sum_f64(d), -1.0), 1.0);
    double scc = 0.0;
#pragma unroll
    for (int j = 0; j < PPL_PER; j++) {
        y[j] = fma(-d, x[j], y[j]);                                    // y becomes c, the part of bn orthogonal to an
        scc = fma(y[j], y[j], scc);
    }
    const double rc = 1.0 / fmax(sqrt(wave_sum_f64(scc)), 1e-12);
    const double theta = acos(d);
    double s0, c0, s1, c1;
    sincos(t0 * theta, &s0, &c0);
    sincos(t1 * theta, &s1, &c1);
    s0 *= rc;
    s1 *= rc;
    double n0 = 0.0, n1 = 0.0;
    double u[PPL_PER];
#pragma unroll
    for (int j = 0; j < PPL_PER; j++) {
        u[j] = fma(y[j], s1, x[j] * c1);
        x[j] = fma(y[j], s0, x[j] * c0);
        n0 = fma(x[j], x[j], n0);
        n1 = fma(u[j], u[j], n1);
    }
    const double r0 = 1.0 / fmax(sqrt(wave_sum_f64(n0)), 1e-12), r1 = 1.0 / fmax(sqrt(wave_sum_f64(n1)), 1e-12);
#pragma unroll
    for (int j = 0; j < PPL_PER; j++) {
        const int k = lane + 64 * j;
        if (k < L) {
            o0[k] = (float)(x[j] * r0);
            o1[k] = (float)(u[j] * r1);
        }
    }
}

extern "C" int rick_ppl_latents_f32(const float *a, const float *b, const float *t, double eps, float *out, int B, int L, int mode,
                                    void *stream) {
    if (!a || !b || !t || !out || B < 0 || L < 1 || L > PPL_MAXL || !(eps > 0.0) || !(eps < INFINITY) || (mode != 0 && mode != 1))
        return RICK_EINVAL;
    if (B == 0) return 0;
    hipLaunchKernelGGL(ppl_latents_kernel, dim3((unsigned)cdiv64(B, 4)), dim3(256), 0, (hipStream_t)stream, a, b, t, eps, out, B, L,
                       mode);
    RICK_LAUNCH_STATUS();
}
