// Gram matrix of a few very long rows and its adjoint — include/rick_hip.h "Gram".  The device side of the cross-domain
// distance-consistency loss (rick_amd/cdc.py): the cosine similarity of whole generator feature maps between the members of a
// batch needs G = X X^T of B <= 8 rows of up to 128 * 1024^2 floats, and its backward pass the row mix dX = (gG + gG^T) X.
// Both kernels stream every row once.  A row is an unordered bag of n values: any memory layout, as long as all rows share it.
// No atomics: every output element has one writer and a fixed summation order.
#include "common.h"

#define GR_MAXB 8
#define GR_SLICE0 4096         // elements of t per slice and row at small n: one float4 per thread
#define GR_MAX_SLICES 1024     // above 4096 * 1024 elements the slices grow instead (the second stage adds them serially)
#define GR_MIX_BLOCKS 4096

// Slice length (a multiple of 4096) and count: functions of n alone.
__host__ __device__ static inline int64_t gr_slice_len(int64_t n) { return GR_SLICE0 * cdiv64(n, (int64_t)GR_SLICE0 * GR_MAX_SLICES); }
static inline int64_t gr_nslices(int64_t n) { return cdiv64(n, gr_slice_len(n)); }

// ---- first stage: part[slice][p] = sum over the slice of x[i][t] x[j][t], p = (i, j >= i) in row-major triangle order -------
// Thread l of the block owns the elements t0 + 4 l + 1024 k + {0, 1, 2, 3} (k ascending) of EVERY row and keeps one fp32 FMA
// chain per pair over them in that order; then the wave_sum butterfly per pair, then the four waves in order.  The element ->
// thread map and the chain order depend on (n, t) only — not on B, not on the rows' addresses — so G[i][j] is a function of
// rows i and j alone.  VEC: every row is 16-byte aligned (base % 16 == 0 and n % 4 == 0) and is read with global_load_dwordx4;
// otherwise the same elements are read one by one, with the row's end checked per element.
template <int B, bool VEC>
__global__ __launch_bounds__(256) void gram_kernel(const float *__restrict__ x, int64_t n, int64_t slice_len,
                                                   float *__restrict__ part) {
    constexpr int NT = B * (B + 1) / 2;
    __shared__ float red[4][NT];
    float acc[NT];
#pragma unroll
    for (int p = 0; p < NT; p++) acc[p] = 0.f;
    const int64_t t0 = (int64_t)blockIdx.x * slice_len, t1 = min(n, t0 + slice_len);
#pragma unroll 2
    for (int64_t t = t0 + 4 * (int64_t)threadIdx.x; t < t1; t += 1024) {
        float4 v[B];
#pragma unroll
        for (int i = 0; i < B; i++) {
            const float *r = x + (int64_t)i * n + t;
            if (VEC) {
                v[i] = *reinterpret_cast<const float4 *>(r);
            } else {
                v[i].x = r[0];
                v[i].y = t + 1 < t1 ? r[1] : 0.f;
                v[i].z = t + 2 < t1 ? r[2] : 0.f;
                v[i].w = t + 3 < t1 ? r[3] : 0.f;
            }
        }
        int p = 0;
#pragma unroll
        for (int i = 0; i < B; i++)
#pragma unroll
            for (int j = i; j < B; j++, p++) {
                acc[p] = fmaf(v[i].x, v[j].x, acc[p]);
                acc[p] = fmaf(v[i].y, v[j].y, acc[p]);
                acc[p] = fmaf(v[i].z, v[j].z, acc[p]);
                acc[p] = fmaf(v[i].w, v[j].w, acc[p]);
            }
    }
#pragma unroll
    for (int p = 0; p < NT; p++) acc[p] = wave_sum(acc[p]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int p = 0; p < NT; p++) red[threadIdx.x >> 6][p] = acc[p];
    }
    __syncthreads();
    if (threadIdx.x < NT) {
        const int p = threadIdx.x;
        part[(int64_t)blockIdx.x * NT + p] = ((red[0][p] + red[1][p]) + red[2][p]) + red[3][p];
    }
}

// ---- second stage: G[i][j] = G[j][i] = sum over slices, ascending, in fp64 -----------------------------------------------
// One 64-lane block per pair: the lanes fetch the pair's <= 1024 slice sums into LDS side by side (a lone thread walking them
// pays a memory round trip per slice, 0.12 us each), then lane 0 adds them in ascending order.
__global__ __launch_bounds__(64) void gram_finish_kernel(const float *__restrict__ part, int nslices, int B,
                                                         double *__restrict__ G) {
    __shared__ float buf[GR_MAX_SLICES];
    const int NT = B * (B + 1) / 2, p = blockIdx.x;
#pragma unroll 16
    for (int k = threadIdx.x; k < nslices; k += 64) buf[k] = part[(int64_t)k * NT + p];
    __syncthreads();
    if (threadIdx.x != 0) return;
    int i = 0, q = p;
    while (q >= B - i) {
        q -= B - i;
        i++;
    }
    const int j = i + q;
    double s = 0.0;
    for (int k = 0; k < nslices; k++) s += (double)buf[k];
    G[i * B + j] = s;
    G[j * B + i] = s;
}

// ---- row mix: y[k][t] = sum_m A[k][m] x[m][t], one fp32 chain A[k][0] x[0] -> fma(A[k][1], x[1], .) -> ... per element -------
// A (B x B, device memory) is the same for every thread: it is read once into registers.  VEC as above (x and y).
template <int B, bool VEC>
__global__ __launch_bounds__(256) void rowmix_kernel(const float *__restrict__ A, const float *__restrict__ x,
                                                     float *__restrict__ y, int64_t n) {
    float a[B * B];
#pragma unroll
    for (int q = 0; q < B * B; q++) a[q] = A[q];
    const int64_t step = (int64_t)gridDim.x * 256, first = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (VEC) {
        const int64_t groups = n >> 2;
        for (int64_t g = first; g < groups; g += step) {
            float4 v[B];
#pragma unroll
            for (int m = 0; m < B; m++) v[m] = *reinterpret_cast<const float4 *>(x + (int64_t)m * n + 4 * g);
#pragma unroll
            for (int k = 0; k < B; k++) {
                float4 o = make_float4(a[k * B] * v[0].x, a[k * B] * v[0].y, a[k * B] * v[0].z, a[k * B] * v[0].w);
#pragma unroll
                for (int m = 1; m < B; m++) {
                    o.x = fmaf(a[k * B + m], v[m].x, o.x);
                    o.y = fmaf(a[k * B + m], v[m].y, o.y);
                    o.z = fmaf(a[k * B + m], v[m].z, o.z);
                    o.w = fmaf(a[k * B + m], v[m].w, o.w);
                }
                *reinterpret_cast<float4 *>(y + (int64_t)k * n + 4 * g) = o;
            }
        }
    } else {
        for (int64_t t = first; t < n; t += step) {
            float v[B];
#pragma unroll
            for (int m = 0; m < B; m++) v[m] = x[(int64_t)m * n + t];
#pragma unroll
            for (int k = 0; k < B; k++) {
                float o = a[k * B] * v[0];
#pragma unroll
                for (int m = 1; m < B; m++) o = fmaf(a[k * B + m], v[m], o);
                y[(int64_t)k * n + t] = o;
            }
        }
    }
}

extern "C" int64_t rick_gram_workspace_bytes(int B, int64_t n) {
    if (B < 1 || B > GR_MAXB || n < 1) return -1;
    return gr_nslices(n) * (B * (B + 1) / 2) * (int64_t)sizeof(float);
}

#define GR_DISPATCH(B_, LAUNCH) \
    switch (B_) {               \
        case 1: LAUNCH(1); break; \
        case 2: LAUNCH(2); break; \
        case 3: LAUNCH(3); break; \
        case 4: LAUNCH(4); break; \
        case 5: LAUNCH(5); break; \
        case 6: LAUNCH(6); break; \
        case 7: LAUNCH(7); break; \
        default: LAUNCH(8); break; \
    }

extern "C" int rick_gram_f32(const float *x, int B, int64_t n, void *ws, double *G, void *stream) {
    if (!x || !ws || !G || B < 1 || B > GR_MAXB || n < 1 || ((uintptr_t)x % 4) || ((uintptr_t)ws % 4) || ((uintptr_t)G % 8))
        return RICK_EINVAL;
    const int64_t slice_len = gr_slice_len(n), nslices = gr_nslices(n);
    const bool vec = ((uintptr_t)x % 16) == 0 && (n & 3) == 0;
    float *part = (float *)ws;
#define GR_LAUNCH(BB)                                                                                                       \
    do {                                                                                                                    \
        if (vec)                                                                                                            \
            hipLaunchKernelGGL((gram_kernel<BB, true>), dim3((unsigned)nslices), dim3(256), 0, (hipStream_t)stream, x, n,   \
                               slice_len, part);                                                                            \
        else                                                                                                                \
            hipLaunchKernelGGL((gram_kernel<BB, false>), dim3((unsigned)nslices), dim3(256), 0, (hipStream_t)stream, x, n,  \
                               slice_len, part);                                                                            \
    } while (0)
    GR_DISPATCH(B, GR_LAUNCH)
#undef GR_LAUNCH
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return 1000 + (int)e;
    hipLaunchKernelGGL(gram_finish_kernel, dim3(B * (B + 1) / 2), dim3(64), 0, (hipStream_t)stream, part, (int)nslices, B, G);
    RICK_LAUNCH_STATUS();
}

extern "C" int rick_rowmix_f32(const float *A, const float *x, float *y, int B, int64_t n, void *stream) {
    if (!A || !x || !y || x == y || B < 1 || B > GR_MAXB || n < 1 || (((uintptr_t)A | (uintptr_t)x | (uintptr_t)y) % 4))
        return RICK_EINVAL;
    const bool vec = (((uintptr_t)x | (uintptr_t)y) % 16) == 0 && (n & 3) == 0;
    const int64_t items = vec ? n >> 2 : n;
    const unsigned blocks = cdiv64(items, 256) < GR_MIX_BLOCKS ? (unsigned)cdiv64(items, 256) : GR_MIX_BLOCKS;     // grid-stride
#define GR_LAUNCH(BB)                                                                                                          \
    do {                                                                                                                       \
        if (vec)                                                                                                               \
            hipLaunchKernelGGL((rowmix_kernel<BB, true>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, A, x, y, n);        \
        else                                                                                                                   \
            hipLaunchKernelGGL((rowmix_kernel<BB, false>), dim3(blocks), dim3(256), 0, (hipStream_t)stream, A, x, y, n);       \
    } while (0)
    GR_DISPATCH(B, GR_LAUNCH)
#undef GR_LAUNCH
    RICK_LAUNCH_STATUS();
}
