// Elastic weight consolidation on the flat parameter buffers — include/rick_hip.h "EWC".  The penalty
//     L = sum_i F_i (theta_i - theta*_i)^2,     d(weight L) / d theta_i = 2 weight F_i (theta_i - theta*_i)
// of rick_amd/ewc.py in ONE pass over four streams (theta, anchor, fisher read; grad read and written) plus the optimiser's mask:
// 20 B per element (+ 1 B with a mask), no temporaries.  The value is summed in fp64 in a fixed order, so it is bit-identical
// from run to run.  No atomics: every gradient element and every partial has one writer.
#include "common.h"

#define EWC_CHUNK 4096         // elements per 256-thread block (rick_ewc_blocks): four float4 per thread and stream

// One element: the three fp32 roundings of the gradient term (difference, product, FMA) and the fp64 term of the value.
// Products and sums stay separate operations (no contraction): the value is the sum of ROUNDED fp64 products.
__device__ __forceinline__ float ewc_elem(float th, float an, float fi, float g, float w2, double &acc) {
#pragma clang fp contract(off)
    const float d = th - an;
    const float t = fi * d;
    const double term = (double)fi * (double)d * (double)d;
    acc += term;
    return __builtin_fmaf(w2, t, g);
}

// Block b owns the elements [b EWC_CHUNK, min(n, (b + 1) EWC_CHUNK)) — a function of n alone, not of the grid or the device.
// Inside the block: `head` elements one by one (the elements in front of the first 16-byte boundary, 0 ... 3), then float4
// groups (group k of the block to thread k % 256), then the < 4 elements that are left, one by one.  A thread adds its terms
// in ascending index order.  hd < 0: the four streams do not share a 16-byte phase — everything is read element by element.
// MASK: a mask is given (the variant without one carries no mask loads and no per-element stores in its float4 loop).
template <bool MASK>
__global__ __launch_bounds__(256) void ewc_kernel(const float *__restrict__ theta, const float *__restrict__ anchor,
                                                  const float *__restrict__ fisher, float *__restrict__ grad,
                                                  const uint8_t *__restrict__ mask, int64_t n, float w2, int hd,
                                                  double *__restrict__ partials) {
    __shared__ double red[4];
    const int64_t s = (int64_t)blockIdx.x * EWC_CHUNK;
    const int len = (int)min((int64_t)EWC_CHUNK, n - s);
    const int head = hd < 0 ? len : min(hd, len);
    const int ngroups = (len - head) >> 2;
    const int tail0 = head + 4 * ngroups;
    theta += s;
    anchor += s;
    fisher += s;
    grad += s;
    if (MASK) mask += s;
    const bool mask4 = MASK && ((uintptr_t)(mask + head) % 4) == 0;
    double acc = 0.0;
    for (int j = threadIdx.x; j < head; j += 256) {
        if (MASK && (mask[j] & 3)) continue;
        grad[j] = ewc_elem(theta[j], anchor[j], fisher[j], grad[j], w2, acc);
    }
#pragma unroll 4
    for (int k = threadIdx.x; k < ngroups; k += 256) {
        const int j = head + 4 * k;
        const float4 th = *reinterpret_cast<const float4 *>(theta + j);
        const float4 an = *reinterpret_cast<const float4 *>(anchor + j);
        const float4 fi = *reinterpret_cast<const float4 *>(fisher + j);
        float4 g = *reinterpret_cast<const float4 *>(grad + j);
        if (MASK) {
            bool m0, m1, m2, m3;
            if (mask4) {                   // the group's four mask bytes in one load
                const uint32_t m = *reinterpret_cast<const uint32_t *>(mask + j);
                m0 = m & 0x3u, m1 = m & 0x300u, m2 = m & 0x30000u, m3 = m & 0x3000000u;
            } else {
                m0 = mask[j] & 3, m1 = mask[j + 1] & 3, m2 = mask[j + 2] & 3, m3 = mask[j + 3] & 3;
            }
            if (__builtin_expect(m0 | m1 | m2 | m3, 0)) {       // a masked element contributes nothing and its gradient is not written
                if (!m0) g.x = ewc_elem(th.x, an.x, fi.x, g.x, w2, acc);
                if (!m1) g.y = ewc_elem(th.y, an.y, fi.y, g.y, w2, acc);
                if (!m2) g.z = ewc_elem(th.z, an.z, fi.z, g.z, w2, acc);
                if (!m3) g.w = ewc_elem(th.w, an.w, fi.w, g.w, w2, acc);
                if (!m3) grad[j + 3] = g.w;
                if (!m2) grad[j + 2] = g.z;
                if (!m1) grad[j + 1] = g.y;
                if (!m0) grad[j] = g.x;
                continue;
            }
        }
        g.x = ewc_elem(th.x, an.x, fi.x, g.x, w2, acc);
        g.y = ewc_elem(th.y, an.y, fi.y, g.y, w2, acc);
        g.z = ewc_elem(th.z, an.z, fi.z, g.z, w2, acc);
        g.w = ewc_elem(th.w, an.w, fi.w, g.w, w2, acc);
        *reinterpret_cast<float4 *>(grad + j) = g;
    }
    for (int j = tail0 + threadIdx.x; j < len; j += 256) {
        if (MASK && (mask[j] & 3)) continue;
        grad[j] = ewc_elem(theta[j], anchor[j], fisher[j], grad[j], w2, acc);
    }
    acc = block_sum_256_f64(acc, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = acc;
}

// out[0] = sum of the partials: thread t adds partials[t], partials[t + 256], ... in ascending order, then the same butterfly and
// wave order (block_sum_256_f64, common.h) — a function of nblocks alone.
__global__ __launch_bounds__(256) void ewc_finish_kernel(const double *__restrict__ partials, int64_t nblocks,
                                                         double *__restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
#pragma unroll 8                // the loads of eight steps in flight; the additions keep their order
    for (int64_t k = threadIdx.x; k < nblocks; k += 256) acc += partials[k];
    acc = block_sum_256_f64(acc, red);
    if (threadIdx.x == 0) out[0] = acc;
}

extern "C" int64_t rick_ewc_blocks(int64_t n) { return n < 0 ? -1 : cdiv64(n, EWC_CHUNK); }

extern "C" int rick_ewc_f32(const float *theta, const float *anchor, const float *fisher, float *grad, const uint8_t *mask,
                            int64_t n, float weight, double *partials, void *stream) {
    if (!theta || !anchor || !fisher || !grad || !partials || n < 0) return RICK_EINVAL;
    if ((((uintptr_t)theta | (uintptr_t)anchor | (uintptr_t)fisher | (uintptr_t)grad) % 4) || ((uintptr_t)partials % 8))
        return RICK_EINVAL;
    const int64_t blocks = rick_ewc_blocks(n);
    if (blocks > 0x7fffffff) return RICK_EINVAL;
    if (blocks == 0) return 0;
    // the block starts are EWC_CHUNK * 4 bytes apart: every block sees the same 16-byte phase
    const unsigned ph = (unsigned)((uintptr_t)theta % 16);
    const bool same = (uintptr_t)anchor % 16 == ph && (uintptr_t)fisher % 16 == ph && (uintptr_t)grad % 16 == ph;
    const int hd = same ? (int)(((16 - ph) % 16) / 4) : -1;
    if (mask)
        hipLaunchKernelGGL(ewc_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, theta, anchor, fisher, grad,
                           mask, n, 2.f * weight, hd, partials);
    else
        hipLaunchKernelGGL(ewc_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, theta, anchor, fisher, grad,
                           mask, n, 2.f * weight, hd, partials);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_ewc_finish_f64(const double *partials, int64_t nblocks, double *out, void *stream) {
    if (!partials || !out || nblocks < 0 || ((uintptr_t)partials % 8) || ((uintptr_t)out % 8)) return RICK_EINVAL;
    hipLaunchKernelGGL(ewc_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partials, nblocks, out);
    RICK_LAUNCH_STATUS();
}
